"""The header reader behind the binding (src/g2048/_abi.py): what it derives from include/g2048.h against values written down here by hand
(taken from the hand-written ctypes tables the reader replaced, not computed with it), and what it refuses.  CPU only."""
import ctypes as C

import pytest

u32, i32, i64, u64, f32, f64, vp = C.c_uint32, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p

# C struct -> (Python name in native.py, sizeof, {field: offset} in declaration order)
STRUCT_PINS = {
    "g2048_gemm_job": ("GemmJob", 120, dict(x=0, ldx=16, w=32, ldw=48, k=64, bias=72, act=80, ldact=88, y=96, ldy=104, N=112, relu=116)),
    "g2048_reduce_job": ("ReduceJob", 40, dict(src=0, dst=8, part_stride=16, n=24, parts=28, src_bf16=32, transpose_rows=36)),
    "g2048_opt_chunk": ("OptChunk", 72, dict(param=0, offset=8, n=16, group=20, shadow=24, shadow_t=32, shadow_p=40, shadow_tp=48, e0=56,
                                             rows=60, cols=64, reserved=68)),
    "g2048_opt_group": ("OptGroup", 40, dict(lr=0, beta1=8, beta2=16, eps=24, weight_decay=32)),
    "g2048_lamb_group": ("LambGroup", 64, dict(lr=0, beta1=8, beta2=16, beta3=24, eps=32, weight_decay=40, bias_correction=48, adapt=52,
                                               trust_clip=56, reserved=60)),
    "g2048_tail_weights": ("TailWeights", 144, dict(wo=0, w1=8, w2=16, a1=24, a2=32, a3=40, c1=48, c2=56, c3=64, bo=72, b1=80, b2=88, ab1=96,
                                                    ab2=104, cb1=112, cb2=120, ln_g=128, ln_b=136)),
    "g2048_tail_weights_t": ("TailWeightsT", 80, dict(woT=0, w1T=8, w2T=16, a1T=24, a2T=32, a3=40, c1T=48, c2T=56, c3=64, ln_g=72)),
    "g2048_tail_saved": ("TailSaved", 104, dict(x_mid=0, mean=8, rstd=16, masks=24, oT=32, h2T=40, uT=48, featsT=56, a1T=64, a2T=72, c1T=80,
                                                c2T=88, ld=96)),
    "g2048_tail_grads": ("TailGrads", 80, dict(daoT=0, dzT=8, df2T=16, da1T=24, da2T=32, dlT=40, dc1T=48, dc2T=56, dvT=64, ln_partial=72)),
    "g2048_dw_job": ("DwJob", 40, dict(dyT=0, xT=8, dw=16, db=24, N=32, K=36)),
    "g2048_dwg_job": ("DwgJob", 72, dict(dy=0, x=8, parts=16, colsum=24, lddy=32, ldx=40, T=48, N=56, K=60, slices=64, parts_f32=68)),
}
# field types of the two structs that mix arrays, pointers and both integer widths (offsets alone cannot tell c_void_p from int64_t)
FIELD_TYPE_PINS = {
    "g2048_gemm_job": [vp * 2, i64 * 2, vp * 2, i64 * 2, i32 * 2, vp, vp, i64, vp, i64, i32, i32],
    "g2048_dwg_job": [vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, i32],
    "g2048_lamb_group": [f64] * 6 + [i32] * 4,
}
# entry point -> (restype, argtypes): every scalar type of the ABI and both return types
PROTOTYPE_PINS = {
    "g2048_abi_version": (i32, []),
    "g2048_policy_step": (i32, [u32] * 4 + [vp, vp, i32, i32, i64] + [vp] * 9 + [i64] * 3 + [i32, i32, vp, vp]),
    "g2048_gae_tb": (i32, [vp] * 5 + [i64, i64, f64, f64, vp]),
    "g2048_attn_fwd": (i32, [vp] * 5 + [i64, i32, i32] + [i64] * 6 + [f32, f32, u64, vp, vp]),
    "g2048_colsum_partial_rows": (i64, [i64, i32]),
    "g2048_opt_workspace_floats": (i64, [i32]),
    "g2048_dweight_jobs_plan": (i32, [vp, i32, i32, i32, vp]),
    "g2048_cls_tail_bwd": (i32, [vp] * 7 + [i64, f32, u64, vp, vp]),
}
CONSTANT_PINS = dict(G2048_ABI_VERSION=4, G2048_EINVAL=-1, G2048_RNG_LEGACY=0, G2048_RNG_PARTITIONABLE=1, G2048_POLICY_DRUL=0,
                     G2048_POLICY_RANDOM=1, G2048_MAX_FUSED_STEPS=128, G2048_F32SPLIT_BIAS=0, G2048_F32SPLIT_BIAS_RELU=1,
                     G2048_F32SPLIT_ADD_LN=2, G2048_F32SPLIT_ADD=3, G2048_GEMM_MAX_JOBS=8, G2048_COLSUM_MAX_GROUPS=512,
                     G2048_PPO_LOSS_MAX_BATCH=1048576, G2048_DWG_MAX_JOBS=16, G2048_REDUCE_MAX_JOBS=64, G2048_OPT_CHUNK=2048,
                     G2048_OPT_MAX_GROUPS=4, G2048_TAIL_MASK_TILES=96, G2048_DW_MAX_JOBS=16)
# the names the product, the benchmark and the tests import from native.py
PYTHON_CONSTANTS = ("RNG_LEGACY", "RNG_PARTITIONABLE", "POLICY_DRUL", "POLICY_RANDOM", "MAX_FUSED_STEPS", "F32SPLIT_BIAS", "F32SPLIT_BIAS_RELU",
                    "F32SPLIT_ADD_LN", "F32SPLIT_ADD", "GEMM_MAX_JOBS", "COLSUM_MAX_GROUPS", "DWG_MAX_JOBS", "OPT_CHUNK", "OPT_MAX_GROUPS",
                    "TAIL_MASK_TILES", "DW_MAX_JOBS")


def test_structs_of_the_header_have_the_pinned_layout():
    from src.g2048 import native as nv

    assert sorted(nv.STRUCTS) == sorted(STRUCT_PINS)
    for c_name, (py_name, size, offsets) in STRUCT_PINS.items():
        cls = nv.STRUCTS[c_name]
        assert getattr(nv, py_name) is cls and cls.__name__ == py_name and issubclass(cls, C.Structure)
        assert C.sizeof(cls) == size, c_name
        assert [(f, getattr(cls, f).offset) for f, _ in cls._fields_] == list(offsets.items()), c_name
    for c_name, types in FIELD_TYPE_PINS.items():
        assert [t for _, t in nv.STRUCTS[c_name]._fields_] == types, c_name
    assert nv.OPT_CHUNK_BYTES == 72


def test_prototypes_of_the_header_have_the_pinned_types():
    from src.g2048 import native as nv

    lib = nv.load()
    for name, (restype, argtypes) in PROTOTYPE_PINS.items():
        assert nv.PROTOTYPES[name] == (restype, argtypes), name
        assert nv.SIGNATURES[name] == argtypes
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    for name, (restype, argtypes) in nv.PROTOTYPES.items():
        assert restype in (i32, i64) and set(argtypes) <= {u32, i32, i64, u64, f32, f64, vp}, name


def test_constants_of_the_header_have_the_pinned_values():
    from src.g2048 import native as nv

    assert nv.CONSTANTS == CONSTANT_PINS
    for name in PYTHON_CONSTANTS:
        assert getattr(nv, name) == CONSTANT_PINS["G2048_" + name], name


@pytest.mark.parametrize("text,needle", [
    ("int g2048_f(const float *x,\n            size_t n, void *stream);", ":2: unknown type `size_t`"),    # an unknown type word
    ("int g2048_f(int64_t n, void (*done)(int), void *stream);", "(*done)"),                                # a function pointer
    ("typedef struct {\n    int32_t a;\n    struct { int32_t b; } in;\n} g2048_s;", ":3: nested struct"),
    ("typedef struct { int32_t a : 3; int32_t b; } g2048_s;", "declarator"),                                # a bitfield
    ("typedef struct { int32_t a; unsigned int b; } g2048_s;", "unsigned"),
    ("typedef struct { int32_t a; int32_t b } g2048_s;", "`;`"),
    ("#define G2048_OK 1\n#define G2048_X 1.5f", ":2: G2048_X is not an integer constant"),
    ("#define G2048_X (G2048_Y + 1)", "G2048_X is not an integer constant"),
    ("#define G2048_X(n) 4", "not an integer constant"),
    ("void g2048_f(int n);", "unknown return type `void`"),
    ("int g2048_f(int n) __attribute__((unused));", "g2048_f"),                                             # matched only in part
    ("static int g2048_f(int n);", "not a g2048_ prototype"),
    ("int g2048_f(int n, int64_t k[2]);", "declarator"),
    ("int g2048_f(int n,, int k);", "declaration"),
    ("int g2048_f(const g2048_missing *jobs, int n);", "unknown type `g2048_missing`"),
    ("int g2048_f(int n)\nint64_t g2048_g(int n);", "g2048_f"),                                             # a lost `;`
])
def test_the_reader_refuses_what_it_does_not_understand(text, needle):
    from src.g2048 import _abi
    from src.g2048 import native as nv

    with pytest.raises(nv.NativeError) as e:
        _abi.parse(text, "demo.h")
    assert str(e.value).startswith("demo.h:") and needle in str(e.value)


def test_prototype_over_several_lines_with_comments():
    from src.g2048 import _abi

    text = ("/* a demo; with (a semicolon), and a comma */\n"
            "int64_t g2048_demo(const float *x, /* rows, read in place */\n"
            "                   int64_t n, uint32_t key0,\n"
            "                   double gamma); // trailing; comment\n"
            "int g2048_none(void);\n")
    abi = _abi.parse(text)
    assert abi.prototypes == {"g2048_demo": (i64, [vp, i64, u32, f64]), "g2048_none": (i32, [])}
    assert abi.structs == {} and abi.constants == {}


def test_struct_and_define_grammar():
    from src.g2048 import _abi

    text = ("#ifndef G2048_H\n#define G2048_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
            "#define G2048_A 7 /* seven */\n#define G2048_B (-1)\n#define G2048_C -12\n"
            "typedef struct { const void *a, *b; float *c; } g2048_ptr_pair;\n"
            "typedef struct {\n    const void *x[2]; int32_t k[2];   /* arrays */\n    double g;\n} g2048_arr;\n"
            "typedef struct { int64_t ld; int32_t N, K; uint64_t seed; float eps; uint32_t key; } g2048_num_rec;\n"
            "int g2048_use(const g2048_arr *jobs, int n_jobs, void *stream);\n"
            "#ifdef __cplusplus\n}\n#endif\n#endif /* G2048_H */\n")
    abi = _abi.parse(text)
    assert abi.constants == dict(G2048_A=7, G2048_B=-1, G2048_C=-12)
    assert abi.prototypes == {"g2048_use": (i32, [vp, i32, vp])}
    assert list(abi.structs) == ["g2048_ptr_pair", "g2048_arr", "g2048_num_rec"]
    pair, arr, rec = abi.structs.values()
    assert pair._fields_ == [("a", vp), ("b", vp), ("c", vp)] and C.sizeof(pair) == 24 and pair.__name__ == "PtrPair"
    assert arr._fields_ == [("x", vp * 2), ("k", i32 * 2), ("g", f64)] and C.sizeof(arr) == 32 and arr.k.offset == 16
    assert rec._fields_ == [("ld", i64), ("N", i32), ("K", i32), ("seed", u64), ("eps", f32), ("key", u32)] and C.sizeof(rec) == 32
    assert tuple(arr((vp * 2)(1, 2), (i32 * 2)(3, 4), 0.5).k) == (3, 4)  # positional construction in header order


def test_missing_header_raises_with_its_path(tmp_path):
    from src.g2048 import _abi
    from src.g2048 import native as nv

    path = str(tmp_path / "include" / "g2048.h")
    with pytest.raises(nv.NativeError) as e:
        _abi.read(path)
    assert path in str(e.value)
    assert nv.HEADER_PATH.endswith("include/g2048.h") and _abi.read(nv.HEADER_PATH).constants == nv.CONSTANTS
