"""CPU checks of team coverage (no GPU): the three entry points are declared in the header and in _lib's table with matching argument
counts and without a new ABI version; each entry refuses bad arguments before any launch; every team the host layer does not support
is refused with a ValueError that names why, before any GPU call; optimize_team with nothing to run returns an empty result."""
import ctypes
import types

import pytest
import torch

from abi_cases import ABI, check_abi_entries

EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_team_step_tail", "tohip_team_loss", "tohip_team_member_gains")
SIZES = ("tohip_team_state_bytes", "tohip_team_member_gains_bytes")


def test_header_and_table_declare_the_team_entries():
    header, before = check_abi_entries(ENTRIES + SIZES)
    # the history comment says why the number stays
    assert f"(still {ABI})" in header and "tohip_team_step_tail" in before


def test_sizes():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    # (n_steps + 1) rows of B members: 8 f32 of state and 4 f64 of terms each
    assert L.tohip_team_state_bytes(3, 10) == 11 * 3 * (32 + 32)
    assert L.tohip_team_state_bytes(0, 10) == 0 and L.tohip_team_state_bytes(3, 0) == 0
    assert L.tohip_team_member_gains_bytes(8) == 8 * (1 + 16) and L.tohip_team_member_gains_bytes(0) == 0


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    sb = L.tohip_team_state_bytes(2, 5)
    names = ("poses", "quats", "poses0", "W", "B", "pge", "qge", "n_eval", "step", "pg", "qg", "mp", "vp", "mq", "vq", "sw", "lw", "eps",
             "lrp", "lrq", "b1", "b2", "aeps", "rth", "sth", "scalars", "log", "log_stride", "state", "state_bytes", "n_steps", "i", "clr_w",
             "clr_grad", "clr_terms", "stream")
    base = dict(zip(names, (p, p, p, 8, 2, p, p, 4, 2, p, p, p, p, p, p, 14.0, 0.02, 1e-6, 0.1, 0.0, 0.9, 0.999, 1e-8, 1.2, 0.9, p, p, 40, p,
                            sb, 5, 0, 0.0, None, None, None)))
    tail = lambda **kw: L.tohip_team_step_tail(*[kw.get(k, base[k]) for k in names])
    for k in ("poses", "quats", "poses0", "pge", "qge", "pg", "qg", "mp", "vp", "mq", "vq", "scalars", "log", "state"):
        assert tail(**{k: None}) == EINVAL, k
    assert tail(W=2) == EINVAL and tail(B=0) == EINVAL and tail(B=257) == EINVAL and tail(n_eval=0) == EINVAL and tail(step=0) == EINVAL
    assert tail(n_eval=5) == EINVAL                  # the last evaluated row lies beyond the trajectory
    assert tail(i=5) == EINVAL and tail(i=-1) == EINVAL and tail(n_steps=0) == EINVAL
    assert tail(log_stride=39) == EINVAL             # two members' logs would overlap
    assert tail(clr_grad=p) == EINVAL and tail(clr_terms=p) == EINVAL   # the clearance rows and terms come together
    assert tail(clr_grad=p, clr_terms=p, clr_w=float("nan")) == EINVAL and tail(clr_grad=p, clr_terms=p, clr_w=-1.0) == EINVAL
    assert tail(state_bytes=sb - 1) == ENOSPC

    lnames = ("poses", "poses0", "W", "B", "sw", "lw", "eps", "scalars", "clr_w", "clr_terms", "terms", "terms64", "total", "grad", "grad_terms",
              "stream")
    lbase = dict(zip(lnames, (p, p, 8, 2, 14.0, 0.02, 1e-6, p, 0.0, None, p, None, p, None, None, None)))
    loss = lambda **kw: L.tohip_team_loss(*[kw.get(k, lbase[k]) for k in lnames])
    for k in ("poses", "poses0", "terms"):
        assert loss(**{k: None}) == EINVAL, k
    assert loss(W=2) == EINVAL and loss(B=0) == EINVAL and loss(B=257) == EINVAL
    assert loss(scalars=None) == EINVAL              # a total needs the team's vis
    assert loss(clr_terms=p, clr_w=float("inf")) == EINVAL

    gb = L.tohip_team_member_gains_bytes(3)
    assert L.tohip_team_member_gains(None, 10, p, 3, None, p, gb, None) == EINVAL
    assert L.tohip_team_member_gains(p, 10, None, 3, None, p, gb, None) == EINVAL
    assert L.tohip_team_member_gains(p, 10, p, 3, None, None, gb, None) == EINVAL
    assert L.tohip_team_member_gains(p, 0, p, 3, None, p, gb, None) == EINVAL
    assert L.tohip_team_member_gains(p, 10, p, 0, None, p, gb, None) == EINVAL
    assert L.tohip_team_member_gains(p, 10, p, 17, None, p, L.tohip_team_member_gains_bytes(17), None) == EINVAL
    assert L.tohip_team_member_gains(p, 10, p, 3, None, p, gb - 1, None) == ENOSPC


# ---- the host layer's refusals: stand-ins with the attributes the checks read (a real ModelTraj needs a device) ---------------------

class _Shard:
    def __init__(self, kind="waypoints", world_size=1):
        self.kind, self.world_size = kind, world_size


POINTS = torch.zeros(50, 3)


def _member(W=8, step=2, points=POINTS, occlusion=None, shard=None, prior=None):
    cam = types.SimpleNamespace(c=ctypes.c_int(7))
    m = types.SimpleNamespace(poses=torch.zeros(W, 3), quats=torch.zeros(W, 4), poses0=torch.zeros(W, 3), points=points,
                              _cloud=types.SimpleNamespace(n=points.shape[0]), _cam=cam, _rig=None, _flags=0, _shard=shard or _Shard(),
                              _occlusion=occlusion, _prior=prior, smoothness_weight=14.0, traj_length_weight=0.02, _clearance_on=False,
                              device=torch.device("cpu"), eps=1e-6)
    m._wps_step = lambda vis_wps_dist: step
    return m


def _prior(seed):
    return types.SimpleNamespace(values=torch.rand(50, generator=torch.Generator().manual_seed(seed)))


REFUSED = {
    "different W": (lambda: [_member(), _member(W=9)], "numbers of waypoints"),
    "different step": (lambda: [_member(), _member(step=3)], "waypoint step"),
    "occlusion": (lambda: [_member(), _member(occlusion="hpr")], "occlusion"),
    "a waypoint-sharded member": (lambda: [_member(), _member(shard=_Shard("waypoints", 2))], "sharded"),
    "a point-sharded member": (lambda: [_member(shard=_Shard("points", 1)), _member()], "sharded"),
    "two different priors": (lambda: [_member(prior=_prior(1)), _member(prior=_prior(2))], "prior"),
    "a prior the first model lacks": (lambda: [_member(), _member(prior=_prior(2))], "prior"),
    "different clouds": (lambda: [_member(), _member(points=torch.ones(50, 3))], "same points"),
    "different cloud sizes": (lambda: [_member(), _member(points=torch.zeros(40, 3))], "same points"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_teams(what):
    from trajectory_optimization_amd.model import TeamTraj
    from trajectory_optimization_amd.optimizer import optimize_team
    make, names = REFUSED[what]
    with pytest.raises(ValueError, match=names):
        optimize_team(make(), n_opt_steps=3)
    with pytest.raises(ValueError, match=names):
        TeamTraj(make())
    with pytest.raises(ValueError, match="no models"):
        optimize_team([])


def test_accepted_priors_and_nothing_to_run():
    from trajectory_optimization_amd.optimizer import TeamOptResult, check_team, optimize_team
    pr = _prior(1)
    same = types.SimpleNamespace(values=pr.values.clone())
    assert check_team([_member(prior=pr), _member()], 0.5, "t") is pr                 # the first model's, the others none
    assert check_team([_member(prior=pr), _member(prior=pr)], 0.5, "t") is pr         # ... or the same
    assert check_team([_member(prior=pr), _member(prior=same)], 0.5, "t") is pr       # ... or an equal tensor
    assert check_team([_member(), _member()], 0.5, "t") is None
    res = optimize_team([_member(), _member(), _member()], n_opt_steps=0)
    assert isinstance(res, TeamOptResult)
    assert (res.steps_taken, res.stopped, res.losses, res.visibility_gain, res.smoothness_gains, res.member_losses) == (0, False, [], 0.0,
                                                                                                                     [0.0] * 3, [])
