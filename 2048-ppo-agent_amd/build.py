"""Build libg2048.so (HIP, gfx950) in-tree: 2048-ppo-agent_amd/lib/libg2048.so.

hipcc cross-compiles without a GPU.  Every csrc/*.hip becomes an object under build/ (compiled in parallel, rebuilt only
when it or a header changed), then one link.  The .so is git-ignored but travels with the working tree.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["g2048.hip", "g2048_policy.hip", "g2048_attention.hip", "g2048_layernorm.hip", "g2048_ppo_loss.hip",
           "g2048_linear.hip", "g2048_optim.hip", "g2048_reduce.hip", "g2048_tail.hip", "g2048_dweight.hip", "g2048_rowgemm.hip", "g2048_mlp.hip",
           "g2048_lookahead.hip", "g2048_f32split.hip", "g2048_symmetry.hip", "g2048_symmetry_ensemble.hip", "g2048_mc.hip", "g2048_ntuple.hip",
           "g2048_ntuple_search.hip", "g2048_ntuple_frontier.hip", "g2048_ntuple_budget.hip", "g2048_ntuple_tc.hip", "g2048_ntuple_carousel.hip", "g2048_ntuple_delayed.hip", "g2048_ntuple_episodes.hip",
           "g2048_ntuple_search_episodes.hip", "g2048_distill.hip"]
# every header under csrc/ plus the ABI: a new header cannot be forgotten by the staleness check
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "g2048.h")]
OBJDIR = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "lib", "libg2048.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]
# per-file additions.  g2048_policy.hip: no NaN handling -- without it every fmaxf on an MFMA result gets a
# canonicalising v_max in front (32 extra vector instructions per attention head in the encoder's softmax).
# -amdgpu-mfma-vgpr-form: the encoder kernels run one wave per SIMD, and for such a function (512 registers) the compiler
# otherwise selects every MFMA in its AGPR form; each accumulator the vector ALU touches (scores, P.V, the projections awaiting
# packing, the linear1 chunk pair, bias tiles, the residual's LayerNorm) then costs a v_accvgpr copy per register and touch.
# With the VGPR form the accumulators live in arch VGPRs; the AGPR half keeps what is parked there on purpose (park_in_agpr: the
# normalised activations, the masking constants) and takes the allocator's VGPR spills instead of scratch.
# Static counts and timings: profiles/encoder_vgpr_accumulators.json.
ENCODER_VGPR_ACC = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
EXTRA = {"g2048_policy.hip": ["-fno-honor-nans", *ENCODER_VGPR_ACC]}


def _stale(target: str, deps) -> bool:
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    return _build(OUT, OBJDIR, EXTRA, force, verbose)


def build_encoder_agpr_acc(out: str, force: bool = False, verbose: bool = False) -> str:
    """The A/B arm of profiles/encoder_vgpr_accumulators.json: the same sources with the encoder's previous register placement
    (every MFMA in its AGPR form: ENCODER_VGPR_ACC left out), as a second library at `out` for G2048_LIB.  Never the product library:
    build() does not come here."""
    if os.path.abspath(out) == OUT:
        raise ValueError("the A/B arm is not built over the product library")
    extra = dict(EXTRA)
    extra["g2048_policy.hip"] = [f for f in EXTRA["g2048_policy.hip"] if f not in ENCODER_VGPR_ACC]
    return _build(os.path.abspath(out), os.path.abspath(out) + ".objs", extra, force, verbose)


def _build(out: str, objdir: str, extra: dict, force: bool, verbose: bool) -> str:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    me = os.path.abspath(__file__)
    jobs = []
    for name in SOURCES:
        src, obj = os.path.join(CSRC, name), os.path.join(objdir, name.replace(".hip", ".o"))
        if force or _stale(obj, [src, me] + HEADERS):
            jobs.append(["hipcc", *FLAGS, *extra.get(name, []), "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), 6)) as pool:
            list(pool.map(run, jobs))
    objs = [os.path.join(objdir, n.replace(".hip", ".o")) for n in SOURCES]
    if jobs or _stale(out, objs):
        run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs])
    return out


if __name__ == "__main__":
    # python build.py [--force] [--encoder-agpr-acc OUT.so]
    if "--encoder-agpr-acc" in sys.argv:
        print(build_encoder_agpr_acc(sys.argv[sys.argv.index("--encoder-agpr-acc") + 1], force="--force" in sys.argv, verbose=True))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
