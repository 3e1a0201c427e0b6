"""CPU-side checks of the per-pose occlusion rows' C ABI (no GPU): tohip_pose_opt as the C compiler lays it out is what _lib.PoseOpt
declares, and the bit-row twins are exported.  (The argument errors are checked with real buffers in test_hip_pose_occlusion.py.)"""
import ctypes

from abi_cases import c_layouts


_FIELDS = ("packed", "n_points", "n_poses", "n_steps", "cam", "occlusion_mask", "trans", "quat", "lr_pose", "lr_quat", "beta1", "beta2",
           "adam_eps", "exp_avg_t", "exp_avg_sq_t", "exp_avg_q", "exp_avg_sq_q", "scalars", "trans_grad", "quat_grad", "loss_log",
           "workspace", "workspace_bytes", "occlusion_bits")


def test_pose_opt_layout_matches_the_c_compiler(tmp_path):
    """(Every struct of the header, by the same compile: tests/test_bindings_cpu.py.)"""
    from trajectory_optimization_amd import _lib
    got = c_layouts({"tohip_pose_opt": _FIELDS}, tmp_path)["tohip_pose_opt"]
    assert got["sizeof"] == ctypes.sizeof(_lib.PoseOpt)
    assert [name for name, _ in _lib.PoseOpt._fields_] == list(_FIELDS)
    for f in _FIELDS:
        assert got[f] == getattr(_lib.PoseOpt, f).offset, f
    assert _lib.PoseOpt._fields_[-1][0] == "occlusion_bits"   # appended: every earlier offset is ABI 13's


def test_bit_row_twins_are_exported():
    from trajectory_optimization_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tohip_pose_forward_bits", "tohip_pose_backward_bits", "tohip_pose_forward_backward_bits", "tohip_pose_opt_step_bits",
                 "tohip_pose_forward_backward_multi_bits"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES, name
