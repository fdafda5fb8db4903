"""ctypes binding of libcocos_hip.so, derived from include/cocos_hip.h: the header is the one place where the C ABI is written
down.  Importing this module parses it into `_SIGNATURES` (every `ret cocos_name(args);` prototype as ctypes) and `CONSTANTS`
(every integer `#define COCOS_*`); a new entry point needs a declaration there, a definition in csrc/ and a caller — no row here.

No fallback: if the library is missing or a call fails, this raises — the product path never
silently degrades to PyTorch or CPU code (the oracle lives under oracle/ and is test-only).
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COCOS_LIB_PATH") or os.path.join(_PKG_DIR, "lib", "libcocos_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "cocos_hip.h")


class CocosHipError(RuntimeError):
    """A libcocos_hip.so entry point returned a negative status (`code`: COCOS_ERR_* of include/cocos_hip.h)."""
    code = 0

    @property
    def unsupported(self) -> bool:
        """the kernel refused the shape (COCOS_ERR_UNSUPPORTED): callers with a framework route take it"""
        return self.code == CONSTANTS["COCOS_ERR_UNSUPPORTED"]


# C type -> ctypes; a parameter with a `*` is a pointer whatever it points to (device pointers travel as integers)
_C_TYPES = {
    "int": ctypes.c_int,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "long long": ctypes.c_longlong,
    "size_t": ctypes.c_size_t,
    "int64_t": ctypes.c_int64,
    "cocos_stream_t": ctypes.c_void_p,
    "const char*": ctypes.c_char_p,      # return type only: as a parameter it is a pointer like any other
}


def _ctype(decl: str, prototype: str):
    if decl not in _C_TYPES:
        raise CocosHipError(f"cocos_hip.h: no ctypes mapping for {decl!r} in `{prototype}`")
    return _C_TYPES[decl]


def _int_define(name: str, expr: str) -> int:
    m = re.fullmatch(r"\(\s*(.*?)\s*\)", expr)
    m = re.fullmatch(r"(-?\d+)(?:\s*<<\s*(\d+))?", m.group(1) if m else expr)
    if not m:
        raise CocosHipError(f"cocos_hip.h: #define {name} {expr}: not an integer, (integer) or (a << b)")
    return int(m.group(1)) << int(m.group(2) or 0)


def parse_header(text: str):
    """The text of cocos_hip.h -> (prototypes, signatures, constants), each in the header's order:
    prototypes  name -> (return type, [parameter declarations]) as C text, comments removed
    signatures  name -> (restype, [argtypes]) as ctypes classes
    constants   COCOS_* -> int for every `#define COCOS_NAME value` (a define without a value, the include guard, is none)
    Anything it does not understand raises: a wrong guess would hand a kernel wrong arguments."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants = {name: _int_define(name, expr)
                 for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(COCOS_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M)}
    code = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    prototypes, signatures = {}, {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(cocos_\w+)\s*\(([^()]*)\)\s*;", code):
        ret, params = " ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")]
        prototype = f"{ret} {name}({', '.join(params)})"
        if name in prototypes:
            raise CocosHipError(f"cocos_hip.h: `{prototype}` is declared twice")
        if params == ["void"]:
            params = []
        prototypes[name] = (ret, params)
        signatures[name] = (_ctype(ret, prototype),
                            [ctypes.c_void_p if "*" in p else _ctype(p.rpartition(" ")[0], prototype) for p in params])
    stray = set(re.findall(r"\b(cocos_\w+)\s*\(", code)) - set(prototypes)
    if stray:
        raise CocosHipError(f"cocos_hip.h: cannot read the declaration of {sorted(stray)}")
    return prototypes, signatures, constants


def _read_header() -> str:
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise CocosHipError(f"{HEADER_PATH}: the binding is derived from this header and cannot be read: {e}") from None


#: the ABI as include/cocos_hip.h declares it (read once, here): C prototypes, name -> (restype, argtypes), COCOS_* integers
PROTOTYPES, _SIGNATURES, CONSTANTS = parse_header(_read_header())

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lock = threading.Lock()
_lib = None


def load() -> ctypes.CDLL:
    """Load (once) and type the shared library. Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise CocosHipError(
                    f"{LIB_PATH} not found: build it with `python -m cocosnet_amd.build` "
                    "(there is no PyTorch/CPU fallback for the correspondence hot path)")
            # PyTorch-ROCm bundles its own libamdhip64; import it FIRST so that this library binds
            # to the same HIP runtime instance (two runtimes in one process = "no ROCm-capable
            # device" on the second one, and torch's streams/pointers would be foreign to it).
            import torch  # noqa: F401
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(lib, name)   # AttributeError -> header and library disagree
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def call(name: str, *args):
    """Invoke an int-returning entry point; raise CocosHipError with the library's message."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.cocos_last_error_string()
        err = CocosHipError(f"{name} failed with code {rc}: {msg.decode() if msg else ''}")
        err.code = rc                # COCOS_ERR_* of include/cocos_hip.h
        raise err
    return rc
