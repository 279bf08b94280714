"""Reader of include/g2048.h: the prototypes, structs and integer #defines of the C ABI as ctypes, so that the binding keeps no copy
of the header.  It knows the small subset of C the header is written in and raises on anything else."""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple


class NativeError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}
_POINTEES = set(SCALARS) | {"void", "uint8_t"}  # and the structs declared so far; every pointer is bound as c_void_p

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DIRECTIVE = re.compile(r"^[ \t]*#[^\n]*", re.M)
_DEFINE = re.compile(r"\s*#[ \t]*define[ \t]+(G2048_\w+)(.*)")
_INTEGER = re.compile(r"\(\s*(-?\d+)\s*\)|(-?\d+)")
_STRUCT = re.compile(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_PROTOTYPE = re.compile(r"\s*(\w+)\s+(g2048_\w+)\s*\((.*)\)\s*", re.S)
_DECLARATION = re.compile(r"\s*(?:const\s+)?(\w+)\s*(.+)", re.S)  # a type word, then the declarators
_DECLARATOR = re.compile(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*")


class Abi(NamedTuple):
    prototypes: dict  # name -> (restype, [argtypes])
    structs: dict     # C name -> ctypes.Structure subclass
    constants: dict   # G2048_NAME -> int


def _blank(m) -> str:
    return re.sub(r"[^\n]", " ", m.group())  # what follows keeps its line number


def parse(text: str, where: str = "g2048.h") -> Abi:
    text = _COMMENT.sub(_blank, text)
    abi = Abi({}, {}, {})

    def refuse(pos: int, why: str):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        line = text.count("\n", 0, pos)
        raise NativeError(f"{where}:{line + 1}: {why}: `{text.splitlines()[line].strip()}`")

    def split(s: str, pos: int, sep: str):
        """The ``sep``-separated parts of ``s`` (which starts at ``pos`` of the header), each with its own position."""
        out = []
        for part in s.split(sep):
            out.append((part, pos))
            pos += len(part) + 1
        return out

    def declaration(decl: str, pos: int, field: bool):
        """`const void *a, *b` / `int32_t k[2]` / `int64_t n` -> [(name, ctype)]; a parameter is one declarator and no array."""
        m = _DECLARATION.fullmatch(decl)
        if not m:
            refuse(pos, "cannot read this declaration")
        out = []
        for d in m.group(2).split(","):
            dm = _DECLARATOR.fullmatch(d)
            if not dm or (not field and (dm.group(3) or out)):
                refuse(pos, "cannot read this declarator")
            ptr, name, count = dm.groups()
            if m.group(1) not in ((_POINTEES | set(abi.structs)) if ptr else SCALARS):
                refuse(pos, f"unknown type `{m.group(1)}`")
            ctype = C.c_void_p if ptr else SCALARS[m.group(1)]
            out.append((name, ctype * int(count) if count else ctype))
        return out

    def directive(m):
        dm = _DEFINE.fullmatch(m.group())
        if dm and dm.group(2).strip():  # an include guard has no body
            im = _INTEGER.fullmatch(dm.group(2).strip())
            if not im:
                refuse(m.start(), f"{dm.group(1)} is not an integer constant")
            abi.constants[dm.group(1)] = int(im.group(1) or im.group(2))
        return _blank(m)

    def struct(m):
        if "{" in m.group(1):
            refuse(m.start(1) + m.group(1).index("{"), "nested struct")
        *decls, (rest, pos) = split(m.group(1), m.start(1), ";")
        if rest.strip():
            refuse(pos, "field without a `;`")
        fields = [f for decl, pos in decls for f in declaration(decl, pos, True)]
        # named as the Python classes are (error messages print it): g2048_tail_weights_t -> TailWeightsT
        py_name = "".join(w.capitalize() for w in re.sub(r"^g2048_", "", m.group(2)).split("_"))
        abi.structs[m.group(2)] = type(py_name, (C.Structure,), {"_fields_": fields})
        return _blank(m)

    text = _DIRECTIVE.sub(directive, text)
    text = re.sub(r'extern\s+"C"\s*\{', _blank, text)
    text = _STRUCT.sub(struct, text)
    for m in re.finditer(r"[^;]+", text):
        if m.group().strip() in ("", "}"):  # the end of the file / of extern "C"
            continue
        pm = _PROTOTYPE.fullmatch(text, m.start(), m.end())
        if not pm:
            refuse(m.start(), "not a g2048_ prototype, a struct typedef or an integer #define")
        if pm.group(1) not in SCALARS:
            refuse(m.start(), f"unknown return type `{pm.group(1)}`")
        params = [] if pm.group(3).strip() == "void" else split(pm.group(3), pm.start(3), ",")
        args = [declaration(p, pos, False)[0][1] for p, pos in params]
        abi.prototypes[pm.group(2)] = (SCALARS[pm.group(1)], args)
    return abi


def read(path: str) -> Abi:
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise NativeError(f"g2048.h not found at {path} ({e.strerror}): the binding reads the C ABI from it at load time; it ships "
                          "beside the package as include/g2048.h.") from None
    return parse(text, path)
