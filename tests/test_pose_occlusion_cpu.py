"""CPU-side checks of the per-pose occlusion rows' C ABI (no GPU): tohip_pose_opt as the C compiler lays it out is what _lib.PoseOpt
declares, and the bit-row twins are exported.  (The argument errors are checked with real buffers in test_hip_pose_occlusion.py.)"""
import ctypes
import os
import shutil
import subprocess

from conftest import REPO


_FIELDS = ("packed", "n_points", "n_poses", "n_steps", "cam", "occlusion_mask", "trans", "quat", "lr_pose", "lr_quat", "beta1", "beta2",
           "adam_eps", "exp_avg_t", "exp_avg_sq_t", "exp_avg_q", "exp_avg_sq_q", "scalars", "trans_grad", "quat_grad", "loss_log",
           "workspace", "workspace_bytes", "occlusion_bits")


def test_pose_opt_layout_matches_the_c_compiler(tmp_path):
    from trajectory_optimization_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"   # (the library's toolchain)
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "trajopt_hip.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(tohip_pose_opt));']
    lines += [f'    printf("{f} %zu\\n", offsetof(tohip_pose_opt, {f}));' for f in _FIELDS]
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(_lib.PoseOpt)
    assert [name for name, _ in _lib.PoseOpt._fields_] == list(_FIELDS)
    for f in _FIELDS:
        assert int(got[f]) == getattr(_lib.PoseOpt, f).offset, f
    assert _lib.PoseOpt._fields_[-1][0] == "occlusion_bits"   # appended: every earlier offset is ABI 13's


def test_bit_row_twins_are_exported():
    from trajectory_optimization_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tohip_pose_forward_bits", "tohip_pose_backward_bits", "tohip_pose_forward_backward_bits", "tohip_pose_opt_step_bits",
                 "tohip_pose_forward_backward_multi_bits"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES, name
