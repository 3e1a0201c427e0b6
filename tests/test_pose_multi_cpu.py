"""CPU-side checks of the multi-pose C ABI (no GPU): the symbols are exported, the workspace grows with the number of poses, and
null or short arguments are refused before any launch."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from trajectory_optimization_amd import _lib
    return _lib.lib()


def test_multi_pose_symbols_are_exported():
    from trajectory_optimization_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tohip_pose_workspace_bytes_multi", "tohip_pose_forward_backward_multi", "tohip_pose_opt_step_multi"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES, name


def test_multi_pose_workspace_grows_with_poses(L):
    for n in (1, 40_452, 1_000_000, 16_000_000):
        sizes = [L.tohip_pose_workspace_bytes_multi(n, b) for b in (1, 2, 8, 64, 257)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (n, sizes)
        assert sizes[0] >= L.tohip_pose_workspace_bytes(n)
        # 16 doubles per (pose, block) partial row
        assert sizes[-1] - sizes[0] >= 256 * 16 * 8 * min(1024, (n + 2047) // 2048) - 256
    assert L.tohip_pose_workspace_bytes_multi(1000, 0) == 0


def test_multi_pose_argument_errors_without_gpu(L):
    from trajectory_optimization_amd import _lib
    cam = _lib.make_camera([1, 0, 0, 0, 1, 0, 0, 0, 1], 10, 10, 1, 5)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails before any launch
    need = L.tohip_pose_workspace_bytes_multi(1000, 4)
    fwd = L.tohip_pose_forward_backward_multi
    assert fwd(None, 1000, fake, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, fake, fake, need, None) == -1
    assert fwd(fake, 1000, None, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, fake, fake, need, None) == -1
    assert fwd(fake, 1000, fake, fake, 0, ctypes.byref(cam), None, None, fake, None, fake, fake, fake, need, None) == -1
    assert fwd(fake, 0, fake, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, fake, fake, need, None) == -1
    assert fwd(fake, 1000, fake, fake, 4, ctypes.byref(cam), None, None, None, None, fake, fake, fake, need, None) == -1   # scalars
    assert fwd(fake, 1000, fake, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, None, fake, need, None) == -1   # one grad
    assert fwd(fake, 1000, fake, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, fake, None, need, None) == -1
    assert fwd(fake, 1000, fake, fake, 4, ctypes.byref(cam), None, None, fake, None, fake, fake, fake, need - 1, None) == _lib.ENOSPC
    assert fwd(fake, 1000, fake, fake, 5, ctypes.byref(cam), None, None, fake, None, None, None, fake, need, None) == _lib.ENOSPC

    o = _lib.PoseOpt()
    o.packed, o.n_points, o.n_poses, o.n_steps, o.cam = 0x1000, 1000, 4, 10, cam
    o.trans = o.quat = o.exp_avg_t = o.exp_avg_sq_t = o.exp_avg_q = o.exp_avg_sq_q = o.scalars = o.loss_log = 0x1000
    o.workspace, o.workspace_bytes = 0x1000, need
    step = L.tohip_pose_opt_step_multi
    assert step(None, 1, None, None) == -1
    assert step(ctypes.byref(o), 0, None, None) == -1           # steps are 1-based
    assert step(ctypes.byref(o), 11, None, None) == -1          # beyond the loss log
    o.workspace_bytes = need - 1
    assert step(ctypes.byref(o), 1, None, None) == _lib.ENOSPC
    o.workspace_bytes, o.loss_log = need, None
    assert step(ctypes.byref(o), 1, None, None) == -1
    o.loss_log, o.packed = 0x1000, None
    assert step(ctypes.byref(o), 1, None, None) == -1
