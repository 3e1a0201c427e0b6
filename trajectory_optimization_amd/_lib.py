"""ctypes loader of libtrajopt_hip.so (the C ABI declared in include/trajopt_hip.h).

The product path has no CPU fallback: if the HIP library is missing or does not load, importing
any op raises.  torch is imported first so that the library binds to the HIP runtime torch already
loaded (same SONAME, libamdhip64.so.7) instead of pulling a second runtime into the process.

Nothing of the ABI is restated here: SIGNATURES, the Structure classes and CONSTANTS are read from the header at import
(read_header), so a new entry point, field or #define is declared there and nowhere else.
"""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  (must precede the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOHIP_LIB") or os.path.join(_HERE, "libtrajopt_hip.so")   # (TOHIP_LIB: a diagnostic build, tools/)
SRC = os.path.join(_HERE, "csrc", "trajopt_hip.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared"]

HEADER = os.path.join(os.path.dirname(_HERE), "include", "trajopt_hip.h")

c_vp = ctypes.c_void_p

# (a uint32_t scalar — a reserved flags word — travels as the 32-bit integer it shares a register with: ctypes checks no range, and
# the scalar types a parameter can have stay these six)
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "int8_t", "uint8_t", "uint16_t", "uint32_t", "uint64_t"}   # what a pointer may point to
_DECLARATOR = re.compile(r"(?:const\s+)?(.+?)\s*(\**)\s*\b(\w+)\s*(?:\[(\d+)\])?")


def read_header(text):
    """The bindings of a C header written like include/trajopt_hip.h -> (constants, structs, signatures): {TOHIP_NAME: int} of the
    integer #defines, {tohip_name: ctypes.Structure subclass} of the `typedef struct tohip_name {...} tohip_name;` blocks and
    {tohip_name: (restype, [argtypes])} of the functions.

    _SCALARS maps the scalar types, a field's as a parameter's, and `const char *` is returned as c_char_p.  A field `[n]` is an
    array, a field of a struct's type nests it, a field that is a pointer is c_void_p.  A pointer parameter is POINTER(Struct)
    for `const tohip_<struct> *`; POINTER(its scalar) when its name ends in _host (POINTER(c_void_p) for a `**`): the header's
    convention for HOST memory; c_void_p otherwise, a device address.  Anything else raises ValueError with the declaration:
    no type is ever guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, structs, signatures = {}, {}, {}

    def declared(decl, ctx, base=None, param=False):
        """`[const] base [*[*]] name [[n]]` (base: the one a struct's `float *a, *b;` shares) -> (base, name, ctypes type)."""
        m = _DECLARATOR.fullmatch(decl.strip() if base is None else f"{base} {decl.strip()}")
        base, stars, name, count = m.groups() if m else (None, None, None, None)
        kind, host = _SCALARS.get(base) or structs.get(base), bool(param and name and name.endswith("_host"))
        if kind and not stars and (not param or (base in _SCALARS and not count)):
            t = kind * int(count) if count else kind
        elif param and base in structs and stars == "*":
            t = ctypes.POINTER(kind)
        elif host and ((base in _SCALARS and stars == "*") or (base in _POINTEES and stars == "**")):
            t = ctypes.POINTER(kind if stars == "*" else c_vp)
        elif not host and base in _POINTEES and stars == "*" and not count:
            t = c_vp
        else:
            raise ValueError(f"cannot map `{decl.strip()}` in `{ctx}`")
        return base, name, t

    for name, params, value in re.findall(r"^#define[ \t]+(\w+)(\(.*?\))?[ \t]*(.*?)[ \t]*$", text, flags=re.M):
        if not params and value:   # (not a macro with arguments, not the include guard)
            if not re.fullmatch(r"-?\d+|\(-?\d+\)", value):
                raise ValueError(f"`#define {name} {value}` is not an integer")
            constants[name] = int(value.strip("()"))
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", re.sub(r"^#.*$", "", text, flags=re.M), flags=re.S)

    def struct(m):
        fields = []
        for line in filter(None, map(str.strip, m.group(2).split(";"))):
            base = None
            for decl in line.split(","):
                base, name, t = declared(decl, f"{line}; of struct {m.group(1)}", base)
                fields.append((name, t))
        camel = "".join(w.capitalize() for w in m.group(1).split("_")[1:])   # tohip_traj_opt -> TrajOpt
        structs[m.group(1)] = type(camel, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"struct {m.group(1)} of the C ABI."})
        return ""

    text = re.sub(r"typedef\s+struct\s+(tohip_\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    for stmt in filter(None, map(str.strip, text.split(";"))):   # what is left: the functions
        ctx = " ".join(stmt.split()) + ";"
        m = re.fullmatch(r"(const char \*|\w+)\s*(tohip_\w+)\s*\((.*)\)", stmt, flags=re.S)
        res = m and {"const char *": ctypes.c_char_p, **_SCALARS}.get(m.group(1))
        if not res:
            raise ValueError(f"cannot read `{ctx}`")
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        signatures[m.group(2)] = (res, [declared(p, ctx, param=True)[2] for p in params])
    return constants, structs, signatures


try:
    with open(HEADER) as _f:
        # CONSTANTS: every integer #define; SIGNATURES: name -> (restype, argtypes), every symbol the header declares
        CONSTANTS, _structs, SIGNATURES = read_header(_f.read())
    Camera, Rig, TrajLoss, TrajOpt, PoseOpt, AdamGroup, OccGeom = (_structs["tohip_" + n] for n in (
        "camera", "rig", "traj_loss", "traj_opt", "pose_opt", "adam_group", "occ_geom"))
    ABI_VERSION, ADAM_MAX_GROUPS = CONSTANTS["TOHIP_ABI_VERSION"], CONSTANTS["TOHIP_ADAM_MAX_GROUPS"]
    ENOSPC, ENOTCONV, ENAN = CONSTANTS["TOHIP_ENOSPC"], CONSTANTS["TOHIP_ENOTCONV"], CONSTANTS["TOHIP_ENAN"]
except (OSError, ValueError, KeyError) as _e:
    raise ImportError(f"{HEADER}: {_e!r}: the bindings are read from this header and there is no other table") from _e

_lib = None


def build(force=False, verbose=False):
    """Compile csrc/trajopt_hip.hip for gfx950 into libtrajopt_hip.so (in-tree)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(HEADER)
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cmd = [HIPCC] + HIPCC_FLAGS + [SRC, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    # into a file of this process's own, then renamed: a second process building at the same time (the ranks of a launcher) or
    # loading the library never sees half of one
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    try:
        subprocess.check_call(cmd[:-1] + [tmp])
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


def lib():
    """The loaded library with argtypes set.  Raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.tohip_abi_version() != ABI_VERSION:
            raise ImportError("libtrajopt_hip.so ABI version mismatch")
        _lib = handle
    return _lib


class HipError(RuntimeError):
    code = None


def check(code, what):
    if code == ENAN:
        raise ValueError("Points cannot contain NaN")  # what scipy.spatial.ConvexHull raises in the reference (tools.py:63)
    if code != 0:
        err = HipError(f"{what} failed: {lib().tohip_error_string(code).decode()} (code {code})")
        err.code = code
        raise err


def make_camera(K, img_width, img_height, min_dist, max_dist, eps=1e-6):
    """K: 9 floats (row-major) on the host."""
    cam = Camera()
    for i, v in enumerate(K):
        cam.K[i] = float(v)
    cam.img_width, cam.img_height = float(img_width), float(img_height)
    cam.min_dist, cam.max_dist, cam.eps = float(min_dist), float(max_dist), float(eps)
    return cam


def stream_ptr():
    return c_vp(torch.cuda.current_stream().cuda_stream)


def device_index(device):
    """A HIP device's index ('cuda' alone: the current device's), resolved once where a plan is built."""
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def on_device(index, fn, *args):
    """fn(*args, stream) with `stream` the raw current stream of device `index`.  torch.cuda.device(index) is entered only when
    `index` is not the current device: the host-bound paths, whose device is current, pay no context manager."""
    if torch._C._cuda_getDevice() == index:
        return fn(*args, torch._C._cuda_getCurrentRawStream(index))
    with torch.cuda.device(index):
        return fn(*args, torch._C._cuda_getCurrentRawStream(index))


def ptr(t):
    return c_vp(t.data_ptr()) if t is not None else c_vp(0)
