"""ctypes binding of libhoisdf_hip.so, derived at import from include/hoisdf.h (the C ABI's one declaration).

The HIP library is the product path: there is NO CPU / PyTorch fallback.  ``lib()`` raises
``HoisdfLibraryError`` if the shared object is missing (run ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C hoisdf_amd/csrc``), and every call raises
``HoisdfError`` with the library's message on a non-zero status.

``parse_header`` reads the header's ``#define HOISDF_<NAME> <integer>`` limits, every ``typedef struct { ... } hoisdf_x;`` (-> the
``ctypes.Structure`` ``X`` in CamelCase: ``hoisdf_sdf_weights`` is ``SdfWeights``) and every ``hoisdf_*`` prototype (-> ``argtypes`` /
``restype``).  Adding an entry is: declare it in the header, define it in csrc/ - nothing here changes.  The parser knows this
header's dialect, not C, and raises ``HeaderError`` with the offending text on anything it cannot classify.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Set, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HOISDF_LIB", os.path.join(_HERE, "libhoisdf_hip.so"))   # override: A/B experiments
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hoisdf.h")


class HoisdfLibraryError(RuntimeError):
    pass


class HoisdfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libhoisdf_hip status {code}: {msg}")
        self.code = code


class HeaderError(ValueError):
    """a declaration of include/hoisdf.h that the binding cannot classify"""


_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "int32_t": C.c_int32,
            "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8}
_DIRECTIVES = r"\s*#\s*(include\s*<\w+\.h>|ifndef\s+HOISDF_H_|define\s+HOISDF_H_|endif)\s*"
_DECLARATION = re.compile(r"typedef\s+(struct|enum)\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}]+);")


def parse_header(text: str) -> Tuple[Dict[str, int], Dict[str, type], Dict[str, Tuple[List, object]], Set[str]]:
    """-> (constants by name without HOISDF_, Structure classes by C name, (argtypes, restype) by entry name, the names of the
    status entries: an int return and something to write through - a non-const pointer, be it only the stream)"""
    consts: Dict[str, int] = {}
    structs: Dict[str, type] = {}
    functions: Dict[str, Tuple[List, object]] = {}
    status: Set[str] = set()

    def ctype(spec: str, where: str, by_value: bool = False):
        """`spec` = a type without its declarator.  Any pointer is c_void_p (data_ptr(), addressof, byref and None all pass)."""
        words = spec.replace("*", " * ").split()
        base = [w for w in words if w not in ("const", "*")]
        known = _SCALARS.get(base[0]) or structs.get(base[0]) if len(base) == 1 else None
        if "*" in words and (known is not None or base in (["void"], ["char"])):
            return C.c_void_p
        if "*" in words or known is None or (known in structs.values() and not by_value):
            raise HeaderError(f"unknown type {spec.strip()!r} in: {where}")
        return known

    def bound(expr: str, where: str) -> int:
        """an array bound: a sum of integers and HOISDF_ constants"""
        try:
            n = sum(consts[t[len("HOISDF_"):]] if t.startswith("HOISDF_") else int(t) for t in (s.strip() for s in expr.split("+")))
        except (KeyError, ValueError):
            n = 0
        if n <= 0:
            raise HeaderError(f"array bound [{expr}] in: {where}")
        return n

    def struct(name: str, body: str) -> type:
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            m = re.fullmatch(r"((?:const )?\w+)\b(.*)", decl)                    # `const float *a, *b[4]`: base type, declarators
            for d in m[2].split(",") if m else [decl]:
                dm = m and re.fullmatch(r"([* ]*)(\w+)((?: ?\[[^\]]*\])*) ?", d)
                if not dm:
                    raise HeaderError(f"member of {name}: {decl}")
                t = ctype(m[1] + dm[1], decl, by_value=True)
                for b in reversed(re.findall(r"\[([^\]]*)\]", dm[3])):
                    t = t * bound(b, decl)
                fields.append((dm[2], t))
        camel = "".join(p.capitalize() for p in name[len("hoisdf_"):].split("_"))
        if not name.startswith("hoisdf_") or name in structs or not fields or len(dict(fields)) != len(fields):
            raise HeaderError(f"struct {name}")
        return type(camel, (C.Structure,), {"_fields_": fields, "__doc__": f"include/hoisdf.h {name}"})

    def function(decl: str) -> None:
        m = re.fullmatch(r"(.*?)\b(hoisdf_\w+) ?\((.*)\)", decl)
        if not m or m[2] in functions:
            raise HeaderError(f"prototype: {decl}")
        ret = m[1].replace(" ", "")
        restype = None if ret == "void" else C.c_char_p if ret == "constchar*" else ctype(m[1], decl)
        args, writes = [], False
        for p in [] if m[3].strip() == "void" else m[3].split(","):
            pm = re.fullmatch(r" ?(.*[ *])\w+ ?", p)
            if not pm:
                raise HeaderError(f"parameter {p.strip()!r} of: {decl}")
            args.append(ctype(pm[1], decl))
            writes |= "*" in pm[1] and not pm[1].startswith("const")
        functions[m[2]] = (args, restype)
        if ret == "int" and writes:
            status.add(m[2])

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)         # extern "C" { and its }
    for line in re.findall(r"^\s*#.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+HOISDF_(\w+)\s+(-?\d+)\s*", line)
        if m:
            consts[m[1]] = int(m[2])
        elif not re.fullmatch(_DIRECTIVES, line):
            raise HeaderError(f"directive: {line.strip()}")
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    pos = 0
    for m in _DECLARATION.finditer(text):
        if text[pos:m.start()].strip():
            break
        pos = m.end()
        if m[1] == "struct":
            structs[m[3]] = struct(m[3], m[2])
        elif m[1] is None:
            function(" ".join(m[4].split()))
        # an enum (hoisdf_status) names int values; it is no field or parameter type, so it stays unknown to ctype()
    if text[pos:].strip():
        raise HeaderError(f"declaration: {' '.join(text[pos:].split())[:200]}")
    return consts, structs, functions, status


with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, FUNCTIONS, _STATUS = parse_header(_f.read())
MAX_LEVELS, MLP_MAX_LAYERS, POSE_MAX_LAYERS, CROP_MAX_POINTS = (
    CONSTANTS[k] for k in ("MAX_LEVELS", "MLP_MAX_LAYERS", "POSE_MAX_LAYERS", "CROP_MAX_POINTS"))
_classes = {cls.__name__: cls for cls in STRUCTS.values()}                       # Pyramid, SdfWeights, EncoderLayerDesc, Mlp, ...
if len(_classes) != len(STRUCTS) or _classes.keys() & globals().keys():
    raise HeaderError(f"struct names that clash as classes: {sorted(_classes)}")
globals().update(_classes)

# views of FUNCTIONS.  SIGNATURES: the status entries (what `call` is for) -> argument ctypes; _RET: the argument-less strings;
# _OTHER: every other entry (size queries, switches) -> (argument ctypes, restype)
SIGNATURES: Dict[str, List] = {n: a for n, (a, _) in FUNCTIONS.items() if n in _STATUS}
_RET = {n: r for n, (a, r) in FUNCTIONS.items() if r is C.c_char_p and not a}
_OTHER = {n: ar for n, ar in FUNCTIONS.items() if n not in SIGNATURES and n not in _RET}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HoisdfLibraryError(
                f"{LIB_PATH} not found: the HIP extension is not built (make -C hoisdf_amd/csrc). "
                "There is no CPU fallback for the hot path.")
        L = C.CDLL(LIB_PATH)
        for name, (args, ret) in FUNCTIONS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = ret
        _lib = L
    return _lib


_timer = None


def set_timer(timer) -> None:
    """bench.py hook: ``timer.begin(name, args)`` / ``timer.end(name)`` bracket every C-ABI call whose
    name is in ``timer.names`` (HIP events on the launch stream).  None disables."""
    global _timer
    _timer = timer


def call(name: str, *args) -> None:
    t = _timer
    timed = t is not None and name in t.names
    if timed:
        t.begin(name, args)
    rc = getattr(lib(), name)(*args)
    if timed:
        t.end(name)
    if rc != 0:
        raise HoisdfError(rc, lib().hoisdf_last_error().decode())


def exported_symbols() -> List[str]:
    return list(FUNCTIONS)
