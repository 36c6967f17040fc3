"""ctypes binding of include/o3dsot.h (libo3dsot_hip.so), derived from the header itself.

The library is the product's only compute path: if it is missing or fails to load this
module raises -- there is NO CPU or PyTorch fallback.  `import torch` happens first on
purpose: torch brings its own ROCm runtime (libamdhip64.so.7) and the kernels must run on
the same runtime instance that owns torch's device pointers and streams.

The header is the one declaration of an entry point, a job struct or an `O3D_*` limit: it is parsed once at import
(no library needed) into SIGNATURES / RESTYPES / CONSTANTS and the layouts behind struct() / dtype().  The parser is
strict -- a declaration it does not fully understand fails the import; it never guesses.
"""
import ctypes
import functools
import os
import re

import numpy as np
import torch  # noqa: F401  (must be loaded before the HIP library, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "_lib", "libo3dsot_hip.so")
if os.environ.get("O3D_LIB_VARIANT"):      # A/B builds of tools/build_variant.sh (same ABI, different -D switches)
    SO_PATH = os.path.join(_HERE, "_lib", "libo3dsot_hip.%s.so" % os.environ["O3D_LIB_VARIANT"])
HEADER = os.path.join(_HERE, "..", "include", "o3dsot.h")


class O3DError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "unsigned": ctypes.c_uint, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
_RESTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_STARS = r"((?:\*\s*(?:const\s*)?)*)"                  # `*`, `**`, `* const*`
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*%s(\w+)?" % _STARS)
_DECLARATOR = re.compile(r"%s(\w+)\s*(?:\[\s*(\d+)\s*\])?" % _STARS)


def _ctype(base, stars, structs, what):
    """the ctypes type of `base` behind `stars`: any pointer is c_void_p (None and data_ptr() ints both convert)"""
    if stars:
        if base not in _SCALARS and base not in structs and base not in ("void", "char"):
            raise O3DError("o3dsot.h: pointer to unknown type in `%s`" % what)
        return ctypes.c_void_p
    if base not in _SCALARS:
        raise O3DError("o3dsot.h: unknown or by-value type in `%s`" % what)
    return _SCALARS[base]


def _parse_header(text):
    """(signatures, restypes, struct field lists, constants) of the header `text`; raises O3DError on anything that is not
    an include guard, an integer #define, a `typedef struct {scalars, pointers, 1-D arrays} name;` or a prototype over
    scalars and pointers."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)          # extern "C" { ... }
    constants, code = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*define\s+(O3D_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*", line)
        if m:
            constants[m.group(1)] = int(m.group(2))
        elif not re.fullmatch(r"\s*#\s*(include\s*<\w+\.h>|ifndef\s+\w+|define\s+\w+|endif)\s*", line):
            raise O3DError("o3dsot.h: directive not understood: `%s`" % line.strip())
    code = "\n".join(code)
    signatures, restypes, structs = {}, {}, {}
    for stmt in re.split(r";(?![^{}]*\})", code):                                 # the `;` outside braces
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"typedef struct \{([^{}]*)\} ?(\w+)", stmt)
        if m:
            fields = []
            for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
                base, rest = re.fullmatch(r"(?:const\s+)?(\w*)\s*(.*)", decl).groups()
                for d in rest.split(","):
                    dm = _DECLARATOR.fullmatch(d.strip())
                    if not dm:
                        raise O3DError("o3dsot.h: declarator not understood in `%s` of %s" % (decl, m.group(2)))
                    t = _ctype(base, dm.group(1), structs, decl)
                    fields.append((dm.group(2), t * int(dm.group(3)) if dm.group(3) else t))
            structs[m.group(2)] = fields
            continue
        m = re.fullmatch(r"(const char ?\*|int|long) ?(o3d_\w+) ?\(([^()]*)\)", stmt)
        if not m or m.group(2) in signatures:
            raise O3DError("o3dsot.h: statement not understood: `%s`" % stmt)
        argtypes = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                pm = _PARAM.fullmatch(p.strip())
                if not pm:
                    raise O3DError("o3dsot.h: parameter not understood: `%s` of %s" % (p.strip(), m.group(2)))
                argtypes.append(_ctype(pm.group(1), pm.group(2), structs, p.strip()))
        signatures[m.group(2)] = argtypes
        restypes[m.group(2)] = _RESTYPES[m.group(1).replace(" *", "*")]
    called = set(re.findall(r"\b(o3d_\w+)\s*\(", code))
    if called != set(signatures):
        raise O3DError("o3dsot.h: %d prototypes parsed, %d names declared: %s"
                       % (len(signatures), len(called), sorted(called ^ set(signatures))))
    return signatures, restypes, structs, constants


def _read_header():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise O3DError("open3dsot_amd: cannot read the C header %s: %s" % (os.path.abspath(HEADER), e))


# name -> argtypes / restype of every prototype, name -> [(field, ctype)] of every struct, the integer `#define O3D_*`
SIGNATURES, RESTYPES, _STRUCT_FIELDS, CONSTANTS = _parse_header(_read_header())


@functools.lru_cache(maxsize=None)
def struct(name):
    """the ctypes.Structure of a `typedef struct {...} name;` of the header: its fields, in its order, native alignment"""
    return type(name, (ctypes.Structure,), {"_fields_": _STRUCT_FIELDS[name]})


@functools.lru_cache(maxsize=None)
def dtype(name):
    """the same layout as a numpy record type (tables that are filled through numpy views of pinned buffers)"""
    return np.dtype(struct(name))


_lib = None


def load():
    """Load the HIP library (once).  Raises O3DError when it is absent -- by design."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise O3DError(
            "open3dsot_amd: %s is missing. Build it with `python -m open3dsot_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SO_PATH)
    try:
        lib = ctypes.CDLL(SO_PATH)
    except OSError as e:  # pragma: no cover
        raise O3DError("open3dsot_amd: cannot load %s: %s" % (SO_PATH, e))
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    _lib = lib
    return lib


_ERR = {-1: "invalid argument (shape / null pointer / unsupported size)",
        -2: "HIP launch failed"}


def check(rc, what):
    if rc != 0:
        raise O3DError("%s failed: %s (code %d)" % (what, _ERR.get(rc, "unknown"), rc))


def version():
    return load().o3d_version().decode()


def on_tensor_device(fn):
    """Run `fn` with the CUDA device of its first GPU-tensor argument current: the launch stream, the scratch
    allocations and the kernel launches of the fused operators then all belong to the device that owns the
    pointers, whichever device the caller left current (a model on cuda:1 while cuda:0 is current)."""
    @functools.wraps(fn)
    def wrapped(*args):
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index == torch.cuda.current_device():
                    break
                with torch.cuda.device(a.device):
                    return fn(*args)
        return fn(*args)
    return wrapped
