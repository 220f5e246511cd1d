"""ctypes binding of include/vvcgpu.h.  Fails loudly when the HIP library is missing or a call fails.

Every function gets its argtypes / restype from its prototype in the header, so a value of the wrong type is refused by
ctypes instead of reaching the library as garbage.  The struct mirrors are in `abi`."""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "lib", "libvvcgpu.so")
HEADER = os.path.join(ROOT, "include", "vvcgpu.h")

_lib = None

# C type of a parameter / a return value -> ctypes type; any pointer is c_void_p, except the error text
_PARAM = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}
_RESULT = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}


class VvcGpuError(RuntimeError):
    pass


def _ctype(decl, table, where):
    if decl in table:
        return table[decl]
    if decl.endswith("*"):
        return C.c_void_p
    raise VvcGpuError("%s: %s: type '%s' has no ctypes mapping" % (HEADER, where, decl))


def prototypes():
    """{name: (restype, argtypes)} of every function include/vvcgpu.h declares"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(vvcgpu_\w+)\s*\(([^()]*)\)\s*;", txt):
        args = []
        for i, prm in enumerate(params.split(",") if params.strip() != "void" else []):
            prm = " ".join(prm.split())
            m = re.fullmatch(r"(?:const )?(\w+) \w+", prm)
            args.append(C.c_void_p if "*" in prm else _ctype(m.group(1) if m else prm, _PARAM, "%s parameter %d" % (name, i + 1)))
        out[name] = (_ctype(" ".join(ret.split()).replace(" *", "*"), _RESULT, name + " result"), tuple(args))
    return out


def declared_symbols():
    """Every function name include/vvcgpu.h declares (used by the ABI test)."""
    return sorted(prototypes())


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VvcGpuError(
                "HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % LIB_PATH)
        dll = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = dll
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise VvcGpuError("%s failed (%d): %s" % (what, rc, lib().vvcgpu_last_error().decode()))


def call(name, *args):
    fn = getattr(lib(), name)
    if len(args) != len(fn.argtypes):                     # ctypes itself lets extra arguments through
        raise TypeError("%s takes %d arguments (%d given)" % (name, len(fn.argtypes), len(args)))
    check(fn(*args), name)


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())
