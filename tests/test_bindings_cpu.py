"""CPU checks of the bindings _lib reads from include/trajopt_hip.h (no GPU): every struct as the C compiler lays it out, one
signature per mapping rule spelled out by hand, the rules over the whole table, and the reader refusing what it cannot map."""
import ctypes
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p as vp

import pytest

from abi_cases import c_layouts, header_text

STRUCTS = {"tohip_camera": "Camera", "tohip_rig": "Rig", "tohip_traj_loss": "TrajLoss", "tohip_traj_opt": "TrajOpt",
           "tohip_pose_opt": "PoseOpt", "tohip_adam_group": "AdamGroup", "tohip_occ_geom": "OccGeom"}
N_FIELDS = {"Camera": 6, "Rig": 3, "TrajLoss": 19, "TrajOpt": 44, "PoseOpt": 24, "AdamGroup": 10, "OccGeom": 3}


def test_every_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof and every offsetof, generated from each class's own field names, against ctypes."""
    from trajectory_optimization_amd import _lib
    classes = {c_name: getattr(_lib, py_name) for c_name, py_name in STRUCTS.items()}
    got = c_layouts({c_name: [f[0] for f in cls._fields_] for c_name, cls in classes.items()}, tmp_path)
    for c_name, cls in classes.items():
        assert cls.__name__ == STRUCTS[c_name] and len(cls._fields_) == N_FIELDS[cls.__name__], c_name
        assert got[c_name].pop("sizeof") == ctypes.sizeof(cls), c_name
        assert got[c_name] == {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}, c_name
    # what the field types are, where a wrong one would keep every offset: arrays, nested structs, pointers
    assert _lib.Camera._fields_[0] == ("K", c_float * 9) and dict(_lib.OccGeom._fields_)["dims"] is c_int32 * 3
    assert dict(_lib.TrajOpt._fields_)["cam"] is _lib.Camera and dict(_lib.TrajLoss._fields_)["rig"] is _lib.Rig
    assert _lib.Rig._fields_ == [("n_cams", c_int32), ("rig_quats", vp), ("rig_trans", vp)]
    assert _lib.AdamGroup._fields_ == [("param", vp), ("grad", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("n", c_int64), ("lr", c_float),
                                       ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("step", c_int32)]


def test_one_signature_per_rule_by_hand():
    from trajectory_optimization_amd import _lib
    S, Cam, Rig = _lib.SIGNATURES, POINTER(_lib.Camera), POINTER(_lib.Rig)
    assert S["tohip_error_string"] == (c_char_p, [c_int])                                    # the char * return
    assert S["tohip_padded_points"] == (c_int64, [c_int64])                                  # the int64_t return
    assert S["tohip_pack_cloud"] == (c_int, [vp, c_int64, c_int, vp, vp, c_size_t, vp])      # plain pointers and scalars
    assert S["tohip_traj_forward"] == (c_int, [vp, c_int64, vp, vp, c_int64, Cam, Rig, c_int, vp, vp, vp, vp, vp, c_size_t, vp])
    assert S["tohip_covmap_read_header"] == (c_int, [vp, POINTER(c_int64), POINTER(c_float), vp])   # _host pointers of two pointees
    assert S["tohip_traj_extrema_view"] == (c_int, [c_int64, c_int64, vp, c_size_t, POINTER(vp), POINTER(c_int64)])   # int32_t **
    assert S["tohip_views_select"] == (c_int, [vp, c_size_t, c_int64, c_int64, c_int64, vp, c_int64, c_double, vp, vp, vp, vp, vp])
    assert S["tohip_adam_step_multi"] == (c_int, [POINTER(_lib.AdamGroup), c_int32, vp])     # a struct pointer that is not the camera
    # the same objects, not equal ones: what the library handle gets is what a hand-written table would hold
    for name in S:
        assert all(t is u for t, u in zip(S[name][1], getattr(_lib.lib(), name).argtypes)), name
        assert getattr(_lib.lib(), name).restype is S[name][0], name


def test_the_rules_hold_over_the_whole_table():
    """Every parameter named *_host is a typed pointer, no other non-struct pointer is typed, and every argument count is the
    header's — by a parse of its own, from the declarations' text."""
    from trajectory_optimization_amd import _lib
    header = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    decls = re.findall(r"\b(tohip_\w+)\s*\(([^;{}]*)\)\s*;", header)
    assert len(decls) == len(_lib.SIGNATURES) == len({name for name, _ in decls}) and len(decls) >= 154
    struct_pointers = {POINTER(getattr(_lib, py_name)) for py_name in STRUCTS.values()}
    n_host = 0
    for name, params in decls:
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        argtypes = _lib.SIGNATURES[name][1]
        assert len(params) == len(argtypes), name
        for param, t in zip(params, argtypes):
            typed = isinstance(t, type) and issubclass(t, ctypes._Pointer)
            if "tohip_" in param:
                assert t in struct_pointers, (name, param)
            elif param.endswith("_host"):
                assert typed and "*" in param, (name, param)
                n_host += 1
            elif "*" in param:
                assert t is vp, (name, param)
            else:
                assert t in (c_int, c_int32, c_int64, c_size_t, c_float, c_double), (name, param)
    assert n_host >= 21


def test_constants_are_the_headers():
    from trajectory_optimization_amd import _lib
    C = _lib.CONSTANTS
    assert len(C) >= 28 and all(type(v) is int for v in C.values())
    assert (C["TOHIP_OK"], C["TOHIP_EINVAL"], C["TOHIP_ENOSPC"], C["TOHIP_ENOTCONV"], C["TOHIP_ENAN"]) == (0, -1, -2, -3, -4)
    assert (_lib.ENOSPC, _lib.ENOTCONV, _lib.ENAN, _lib.ADAM_MAX_GROUPS) == (-2, -3, -4, 8)
    assert C["TOHIP_POINT_TILE"] == 2048 and C["TOHIP_FLIP_WORKSPACE_BYTES"] == 8192 and C["TOHIP_TEAM_MAX_GAINS"] == 16
    assert "TOHIP_TRAJ_STRIDE" not in C and "TRAJOPT_HIP_H" not in C   # a macro with an argument, the include guard


GOOD = "typedef struct tohip_s { float a; } tohip_s;\nint tohip_f(const tohip_s *s_host, int64_t n, float *x, void *stream);\n"


@pytest.mark.parametrize("text, names", [
    ("int tohip_f(unsigned long x);", ("unsigned long", "tohip_f")),                                  # an unknown type
    ("int tohip_g(const tohip_nothing *p_host, void *stream);", ("tohip_nothing", "tohip_g")),       # an unknown struct pointer
    ("typedef struct tohip_t { float a; uint16_t bad, worse; } tohip_t;", ("uint16_t", "tohip_t")),   # a field it cannot map
    ("int tohip_h(float **rows);", ("float **", "tohip_h")),                                          # a ** that is not _host
    ("int tohip_i(void *blob_host);", ("void *", "tohip_i")),                                         # a _host pointer to nothing typed
    ("long tohip_j(int x);", ("long tohip_j",)),                                                      # an unknown return type
    ("#define TOHIP_X 1.5\n", ("TOHIP_X",)),                                                          # a constant that is no integer
    ("int tohip_k(int x)\nint y;", ("tohip_k",)),                                                     # not a declaration at all
])
def test_the_reader_refuses_and_names_the_declaration(text, names):
    from trajectory_optimization_amd import _lib
    constants, structs, signatures = _lib.read_header(GOOD)
    assert signatures == {"tohip_f": (c_int, [POINTER(structs["tohip_s"]), c_int64, vp, vp])} and not constants
    with pytest.raises(ValueError) as err:
        _lib.read_header(GOOD + text)
    for name in names:
        assert name in str(err.value), (name, str(err.value))


def test_import_fails_without_a_header_it_can_read(tmp_path):
    """_lib.py beside no include/trajopt_hip.h, then beside one it cannot map: an ImportError that names the file (and there is no
    table to fall back on: nothing of the module is left)."""
    import importlib.util
    import shutil
    from trajectory_optimization_amd import _lib
    (tmp_path / "pkg").mkdir()
    shutil.copy(_lib.__file__, tmp_path / "pkg" / "_lib.py")
    header = tmp_path / "include" / "trajopt_hip.h"
    for text, why in ((None, "FileNotFoundError"), ("int tohip_f(unsigned long x);\n", "unsigned long x")):
        if text is not None:
            header.parent.mkdir()
            header.write_text(text)
        spec = importlib.util.spec_from_file_location("_lib_without_header", tmp_path / "pkg" / "_lib.py")
        with pytest.raises(ImportError) as err:
            spec.loader.exec_module(importlib.util.module_from_spec(spec))
        assert str(header) in str(err.value) and why in str(err.value)
