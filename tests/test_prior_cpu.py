"""CPU checks of the log-odds prior's C ABI and argument checks (no GPU): the header declares the new entry points without a new ABI
version, the prior buffer's size follows its layout, every entry refuses null or bad arguments before any launch, and
ops.check_prior refuses what is not a finite, non-negative prior of one entry per point."""
import ctypes

import pytest
import torch

from abi_cases import check_abi_entries

EINVAL, ENOSPC = -1, -2
NEW = ("tohip_traj_prior_bytes", "tohip_traj_prior_build", "tohip_traj_reward_prior", "tohip_traj_reward_backward_prior",
       "tohip_traj_backward_prior", "tohip_traj_coverage")


def test_header_declares_the_prior_entries():
    from trajectory_optimization_amd import _lib
    header, _ = check_abi_entries(NEW)
    for sym in NEW:
        assert sym + "(" in header and sym in _lib.SIGNATURES
    # the _prior variants are the existing argument lists plus the prior buffer before the stream
    for old, new in (("tohip_traj_reward", "tohip_traj_reward_prior"), ("tohip_traj_reward_backward", "tohip_traj_reward_backward_prior"),
                     ("tohip_traj_backward", "tohip_traj_backward_prior")):
        a, b = _lib.SIGNATURES[old][1], _lib.SIGNATURES[new][1]
        assert b[:-2] == a[:-1] and b[-2:] == [ctypes.c_void_p, ctypes.c_void_p]


def test_prior_bytes_follow_the_layout():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    # 2 KB header (128 block bases + their total), then prior and sigmoid(prior), npad f32 each
    for n in (1, 2048, 2049, 1_000_000):
        assert L.tohip_traj_prior_bytes(n) == 2048 + 8 * L.tohip_padded_points(n)
    assert L.tohip_traj_prior_bytes(1) == 2048 + 8 * 2048
    assert L.tohip_traj_prior_bytes(0) == 0 and L.tohip_traj_prior_bytes(-5) == 0


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    cam = _lib.make_camera([1, 0, 0, 0, 1, 0, 0, 0, 1], 10, 10, 1, 5)
    c = ctypes.byref(cam)
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    nb = L.tohip_traj_prior_bytes(10)
    # build: null packed / prior / buffer / status, bad n, too small a buffer
    assert L.tohip_traj_prior_build(None, 10, p, p, nb, p, None) == EINVAL
    assert L.tohip_traj_prior_build(p, 10, None, p, nb, p, None) == EINVAL
    assert L.tohip_traj_prior_build(p, 10, p, None, nb, p, None) == EINVAL
    assert L.tohip_traj_prior_build(p, 10, p, p, nb, None, None) == EINVAL
    assert L.tohip_traj_prior_build(p, 0, p, p, nb, p, None) == EINVAL
    assert L.tohip_traj_prior_build(p, 10, p, p, nb - 1, p, None) == ENOSPC
    # reward: null arguments with a prior; a prior with prefilled (every reward is written); NULL prior = tohip_traj_reward's checks
    assert L.tohip_traj_reward_prior(None, p, 10, 1e-6, 0, p, p, p, 4096, p, None) == EINVAL
    assert L.tohip_traj_reward_prior(p, None, 10, 1e-6, 0, p, p, p, 4096, p, None) == EINVAL
    assert L.tohip_traj_reward_prior(p, p, 10, 1e-6, 0, None, p, p, 4096, p, None) == EINVAL
    assert L.tohip_traj_reward_prior(p, p, 0, 1e-6, 0, p, p, p, 4096, p, None) == EINVAL
    assert L.tohip_traj_reward_prior(p, p, 10, 1e-6, 1, p, p, p, 4096, p, None) == EINVAL
    assert L.tohip_traj_reward_prior(p, p, 10, 1e-6, 0, p, p, p, 16, p, None) == ENOSPC
    assert L.tohip_traj_reward_prior(None, p, 10, 1e-6, 0, p, p, p, 4096, None, None) == EINVAL
    # reward + backward
    ws = L.tohip_traj_workspace_bytes(10, 2)
    args = lambda **kw: [kw.get(k, v) for k, v in (("packed", p), ("n", 10), ("W", 2), ("cam", c), ("rig", None), ("flags", 0), ("occ", None),
                                                   ("lo", p), ("eps", 1e-6), ("pre", 0), ("rw", p), ("sc", p), ("gout", p), ("pg", p), ("qg", p),
                                                   ("ws", p), ("wsb", ws), ("prior", p), ("st", None))]
    assert L.tohip_traj_reward_backward_prior(*args(pre=1)) == EINVAL
    for k in ("packed", "lo", "rw", "sc", "gout", "pg", "qg", "ws", "cam"):
        assert L.tohip_traj_reward_backward_prior(*args(**{k: None})) == EINVAL, k
    assert L.tohip_traj_reward_backward_prior(*args(n=0)) == EINVAL
    assert L.tohip_traj_reward_backward_prior(*args(W=0)) == EINVAL
    assert L.tohip_traj_reward_backward_prior(*args(wsb=ws - 1)) == ENOSPC
    assert L.tohip_traj_reward_backward_prior(*args(prior=None, pre=1, rw=None)) == EINVAL
    # backward: the upstream is grad_rewards, or scalars and gout
    bargs = lambda **kw: [kw.get(k, v) for k, v in (("packed", p), ("n", 10), ("W", 2), ("cam", c), ("rig", None), ("flags", 0), ("occ", None),
                                                    ("lo", p), ("gr", None), ("sc", p), ("gout", p), ("pg", p), ("qg", p), ("ws", p),
                                                    ("wsb", ws), ("prior", p), ("st", None))]
    assert L.tohip_traj_backward_prior(*bargs(sc=None)) == EINVAL
    assert L.tohip_traj_backward_prior(*bargs(gout=None)) == EINVAL
    for k in ("packed", "lo", "pg", "qg", "ws", "cam"):
        assert L.tohip_traj_backward_prior(*bargs(**{k: None})) == EINVAL, k
    assert L.tohip_traj_backward_prior(*bargs(n=-1)) == EINVAL
    assert L.tohip_traj_backward_prior(*bargs(wsb=ws - 1)) == ENOSPC
    assert L.tohip_traj_backward_prior(*bargs(prior=None, lo=None)) == EINVAL
    # coverage: null pointers, bad n, a NaN or negative threshold
    inf = float("inf")
    assert L.tohip_traj_coverage(None, 10, p, p, inf, p, None) == EINVAL
    assert L.tohip_traj_coverage(p, 10, None, p, inf, p, None) == EINVAL
    assert L.tohip_traj_coverage(p, 10, p, p, inf, None, None) == EINVAL
    assert L.tohip_traj_coverage(p, 0, p, p, inf, p, None) == EINVAL
    assert L.tohip_traj_coverage(p, 10, p, p, float("nan"), p, None) == EINVAL
    assert L.tohip_traj_coverage(p, 10, p, None, -1.0, p, None) == EINVAL


def test_check_prior():
    from trajectory_optimization_amd import ops
    good = torch.tensor([0.0, 0.5, 3.0, -0.0])
    out = ops.check_prior(good, 4)
    assert out.dtype == torch.float32 and torch.equal(out, good)
    assert ops.check_prior(good.double(), 4).dtype == torch.float32
    bad = {
        "wrong length": torch.zeros(5),
        "two dimensions": torch.zeros(4, 1),
        "NaN": torch.tensor([0.0, float("nan"), 1.0, 1.0]),
        "inf": torch.tensor([0.0, float("inf"), 1.0, 1.0]),
        "-inf": torch.tensor([0.0, float("-inf"), 1.0, 1.0]),
        "negative": torch.tensor([0.0, -1e-3, 1.0, 1.0]),
        "integer": torch.zeros(4, dtype=torch.int32),
        "a list": [0.0, 0.0, 0.0, 0.0],
        "f64 beyond f32": torch.tensor([0.0, 1e300, 0.0, 0.0], dtype=torch.float64),
    }
    for what, p in bad.items():
        with pytest.raises(ValueError):
            ops.check_prior(p, 4)
    with pytest.raises(ValueError, match="lives on"):
        ops.check_prior(good, 4, device="cuda:0")
    ops.check_prior(good, 4, device="cpu")


def test_fuse_log_odds():
    from trajectory_optimization_amd import tools
    a, b = torch.tensor([0.0, 1.0, 2.0]), torch.tensor([0.5, 3.0, 0.0])
    assert torch.equal(tools.fuse_log_odds(a, b), torch.tensor([0.5, 4.0, 2.0]))
    assert torch.equal(tools.fuse_log_odds(a, b, clamp_max=3.5), torch.tensor([0.5, 3.5, 2.0]))
    assert torch.equal(a, torch.tensor([0.0, 1.0, 2.0]))   # the inputs are left as they are
    with pytest.raises(ValueError):
        tools.fuse_log_odds(a, torch.zeros(4))
    with pytest.raises(ValueError):
        tools.fuse_log_odds()
