"""CPU checks of the unknown volume a view reveals and the greedy selection by it (no GPU): the new entry points are declared in the
header and in _lib's table at ABI 15; each refuses bad arguments before any launch; ops.check_view_volume refuses by name; and the
numpy restatements (synth.unknown_ref / view_volume_ref / volume_select_ref, what the kernels are compared against bit for bit) are
checked on hand cases and on the closed-room theorem."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_occ_unknown", "tohip_view_volume", "tohip_view_volume_pick")
SCENE = dict(origin=(-0.5, -0.5, -0.5), resolution=0.125, dims=(28, 24, 16))
SCANNER = np.float32([1.03, 0.97, 0.52])


def test_header_and_table_declare_the_new_entries_at_abi_15():
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_view_volume_pick" in before
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert src.index('#include "frontier_kernels.hip"') < src.index('#include "volume_kernels.hip"')   # the walk, the mask, the listing
    # the definition is stated where a C caller reads it
    for phrase in ("REVEALED", "start_skip 1, end_skip 0", "window != 0", "view_index"):
        assert phrase in header, phrase


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    # pointers no call may reach
    p, q, r, t, u, v, w = (ctypes.c_void_p(a) for a in (64, 4096, 8192, 16384, 32768, 65536, 131072))
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb = L.tohip_occ_bytes(64, 64, 32)
    cam = _lib.make_camera(synth.K_INTRINS.reshape(-1).tolist(), synth.IMG_WIDTH, synth.IMG_HEIGHT, 1.0, 5.0)
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    calls = {
        "unknown": (L.tohip_occ_unknown, ("occ", "free", "out", "bytes", "geom", "stream"), (p, q, r, nb, ok, None)),
        "volume": (L.tohip_view_volume, ("occ", "free", "claimed", "mark", "bytes", "geom", "poses", "quats", "n", "view_index", "cam", "dmin",
                                         "dmax", "window", "gains", "stop", "stats", "stream"),
                   (p, q, None, None, nb, ok, t, u, 3, None, ctypes.byref(cam), 0.5, 5.0, 1, v, None, None, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name, first in (("unknown", "out"), ("volume", "occ")):
        assert call(name, **{first: None}) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=nb - 1) == ENOSPC, name   # mismatched grid_bytes
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(occ=None), dict(free=None), dict(out=p), dict(out=q)):
        assert call("unknown", **kw) == EINVAL, kw
    for kw in (dict(free=None), dict(free=p), dict(poses=None), dict(quats=None), dict(cam=None), dict(gains=None), dict(n=0), dict(n=-1),
               dict(n=65536), dict(mark=p), dict(mark=q),
               dict(claimed=r, mark=r),              # mark == claimed with three views
               dict(claimed=r, mark=r, n=2)):
        assert call("volume", **kw) == EINVAL, kw
    # the pick: every pointer, the counts, min_gain >= 1, round >= 0
    pick = lambda **kw: L.tohip_view_volume_pick(*[kw.get(k, b) for k, b in zip(("gains", "taken", "n", "min_gain", "round", "order", "picked", "stop",
                                                                                   "stream"), (p, q, 12, 1, 0, r, t, u, None))])
    for kw in (dict(gains=None), dict(taken=None), dict(order=None), dict(picked=None), dict(stop=None), dict(n=0), dict(n=-1), dict(n=1 << 31),
               dict(min_gain=0), dict(min_gain=-3), dict(round=-1)):
        assert pick(**kw) == EINVAL, kw


def test_check_view_volume_names_what_is_wrong():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd import tools

    class G(ops.OccupancyGrid):   # a plane's geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    space = ops.SpaceMap(G(), G())
    P, Q = torch.zeros(3, 3), torch.tensor([[1.0, 0, 0, 0]] * 3)
    claimed = G()
    assert ops.check_view_volume(space, P, Q) == (3, None, 1)
    assert ops.check_view_volume(space, P, Q, 5, np.int64(7), claimed, G()) == (3, 3, 7)
    assert ops.check_view_volume(space, P, Q, 2, 1, claimed) == (3, 2, 1)
    assert ops.check_view_volume(space, P[:1], Q[:1], 1, 1, claimed, claimed) == (1, 1, 1)   # one view may claim what it counts
    with pytest.raises(ValueError, match="space must be an ops.SpaceMap"):
        ops.check_view_volume(G(), P, Q)
    for bad in (None, np.zeros((3, 3)), torch.zeros(3, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses must be a floating-point tensor"):
            ops.check_view_volume(space, bad, Q)
    for bad in (torch.zeros(3), torch.zeros(3, 4), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="poses must have shape \\(M,3\\) with M >= 1"):
            ops.check_view_volume(space, bad, Q)
    for bad in (torch.zeros(3, 3), torch.zeros(0, 4)):
        with pytest.raises(ValueError, match="quats must have shape \\(M,4\\) with M >= 1"):
            ops.check_view_volume(space, P, bad)
    with pytest.raises(ValueError, match="poses must be finite"):
        ops.check_view_volume(space, P * float("nan"), Q)
    with pytest.raises(ValueError, match="quats must be finite"):
        ops.check_view_volume(space, P, Q * float("inf"))
    with pytest.raises(ValueError, match="poses holds 3 views, quats 2"):
        ops.check_view_volume(space, P, Q[:2])
    for bad in (0, -1, 1.0, True, "2"):
        with pytest.raises(ValueError, match="k must be an integer >= 1"):
            ops.check_view_volume(space, P, Q, bad)
    many = torch.zeros(65536, 3), torch.ones(65536, 4)
    assert ops.check_view_volume(space, *many) == (65536, None, 1)   # (scoring chunks by 65 535; a selection scores all in one launch)
    with pytest.raises(ValueError, match="poses holds 65536 candidates, a selection \\(k given\\) takes at most 65535"):
        ops.check_view_volume(space, *many, 2)
    for bad in (0, -1, 0.5, 1.0, True, None):
        with pytest.raises(ValueError, match="min_gain must be an integer >= 1"):
            ops.check_view_volume(space, P, Q, 1, bad)
    for name in ("claimed", "mark"):
        with pytest.raises(ValueError, match=name + " must be an ops.OccupancyGrid or None"):
            ops.check_view_volume(space, P, Q, **{name: torch.zeros(3)})
        for plane in (space.occupied, space.free):
            with pytest.raises(ValueError, match=name + " must not be one of the map's own planes"):
                ops.check_view_volume(space, P, Q, **{name: plane})
        for g, what in ((G(origin=(0, 0, 0.5)), "origin"), (G(resolution=0.2), "resolution"), (G(dims=(8, 8, 5)), "dims"),
                        (G(device="cuda:1"), "device")):
            with pytest.raises(ValueError, match=f"{name}: its {what} differs from the map's"):
                ops.check_view_volume(space, P, Q, **{name: g})
    with pytest.raises(ValueError, match="mark may be the claimed plane itself only for one view, got 3 views"):
        ops.check_view_volume(space, P, Q, claimed=claimed, mark=claimed)
    # the tools layer: the map and the camera keywords
    with pytest.raises(ValueError, match="view_volume: the map must be an ops.SpaceMap or an ops.EvidenceMap"):
        tools.view_volume(G(), P, Q, intrins=synth.K_INTRINS, img_width=10, img_height=10)
    with pytest.raises(ValueError, match="select_views_volume: the camera is needed: \\['img_height'\\] missing"):
        tools.select_views_volume(space, P, Q, 2, intrins=synth.K_INTRINS, img_width=10)
    with pytest.raises(ValueError, match="select_views_volume: unknown keyword\\(s\\) \\['rig'\\]"):
        tools.select_views_volume(space, P, Q, 2, intrins=synth.K_INTRINS, img_width=10, img_height=10, rig=None)


# ------------------------------------------------------------------------------------------------------------ the restatements

def _corridor(middle):
    """Three voxels along x at r = 1: the camera's voxel 0 is free, voxel 2 is unknown, the middle one as asked."""
    occ, free = np.zeros((3, 1, 1), bool), np.zeros((3, 1, 1), bool)
    free[0] = True
    occ[1], free[1] = middle == "occupied", middle == "free"
    return occ, free


def test_unknown_ref_is_neither_plane():
    occ, free = np.zeros((2, 2, 1), bool), np.zeros((2, 2, 1), bool)
    occ[0, 0], free[0, 1], occ[1, 0], free[1, 0] = True, True, True, True   # (occupied wins where both are set)
    assert synth.unknown_ref(occ, free).tolist() == [[[False], [False]], [[False], [True]]]


@pytest.mark.parametrize("middle,want", [("occupied", []), ("free", [2]), ("unknown", [1, 2])])
def test_three_voxel_corridor(middle, want):
    occ, free = _corridor(middle)
    kept = np.ones((3, 1, 1), bool)
    gain, rev = synth.view_volume_ref(kept, [0.5, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)
    assert gain == len(want) and np.flatnonzero(rev[:, 0, 0]).tolist() == want
    # a voxel the cull does not keep is not revealed; a claimed one is not counted
    kept[2] = False
    assert synth.view_volume_ref(kept, [0.5, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)[0] == len([v for v in want if v != 2])
    claimed = np.zeros((3, 1, 1), bool)
    claimed[1] = True
    gain, rev = synth.view_volume_ref(np.ones((3, 1, 1), bool), [0.5, 0.5, 0.5], (0, 0, 0), 1.0, occ, free, claimed)
    assert np.flatnonzero(rev[:, 0, 0]).tolist() == [v for v in want if v != 1] and gain == int(rev.sum())
    # a camera out of range reveals nothing
    assert synth.view_volume_ref(np.ones((3, 1, 1), bool), [5000.0, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)[0] == 0
    assert synth.view_volume_ref(np.ones((3, 1, 1), bool), [np.nan, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)[0] == 0


def test_the_skip_rule_is_one_zero():
    """start_skip 1: the camera's own voxel is not tested, even when it is occupied; end_skip 0: every voxel up to the target is, so a
    target directly behind the camera's voxel is seen and one behind an occupied neighbour is not."""
    occ, free = np.zeros((3, 1, 1), bool), np.zeros((3, 1, 1), bool)
    occ[0] = True   # the camera stands inside an occupied voxel
    gain, rev = synth.view_volume_ref(np.ones((3, 1, 1), bool), [0.9, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)
    assert gain == 2 and rev[:, 0, 0].tolist() == [False, True, True]
    occ[1] = True   # the neighbour is tested (cheb 1 >= start_skip): voxel 2 is hidden
    assert synth.view_volume_ref(np.ones((3, 1, 1), bool), [0.9, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)[0] == 0
    # with the default skip (1, 1) of line_of_sight the neighbour of the target would not be tested: the rule here is stricter
    a, b = np.float32([[0.9, 0.5, 0.5]]), np.float32([[2.5, 0.5, 0.5]])
    assert synth.los_ref(a, b, (0, 0, 0), 1.0, occ, (1, 1)).tolist() == [1] and synth.los_ref(a, b, (0, 0, 0), 1.0, occ, (1, 0)).tolist() == [0]
    # the camera outside dims, in the apron: its walk enters the grid and is tested from the first voxel inside
    occ[:] = False
    occ[0] = True
    assert synth.view_volume_ref(np.ones((3, 1, 1), bool), [-1.5, 0.5, 0.5], (0, 0, 0), 1.0, occ, free)[0] == 0


def test_volume_select_ref_on_hand_sets():
    S = np.zeros((4, 6, 1, 1), bool)
    S[0, [0, 1, 2]] = True
    S[1, [2, 3, 4]] = True      # the same size as view 0: the tie goes to view 0
    S[2, [3, 4, 5]] = True
    S[3, [0]] = True
    order, gains, mask = synth.volume_select_ref(S, 4)
    assert order == [0, 2] and gains == [3, 3] and mask.all()          # after 0: view 1 adds 2, view 2 adds 3; then nothing is left
    order, gains, mask = synth.volume_select_ref(S, 1)
    assert order == [0] and gains == [3] and int(mask.sum()) == 3
    order, gains, mask = synth.volume_select_ref(S, 4, min_gain=3)
    assert order == [0, 2] and gains == [3, 3]
    order, gains, mask = synth.volume_select_ref(S, 4, min_gain=4)
    assert order == [] and gains == [] and not mask.any()
    claimed = np.zeros((6, 1, 1), bool)
    claimed[[0, 1]] = True
    order, gains, mask = synth.volume_select_ref(S, 4, claimed=claimed)
    assert order == [1, 2] and gains == [3, 1] and sum(gains) == int(mask.sum()) - int(claimed.sum()) and claimed.sum() == 2
    # a duplicated candidate adds nothing the second time
    order, gains, _ = synth.volume_select_ref(np.stack([S[1], S[1], S[3]]), 3)
    assert order == [0, 2] and gains == [3, 1]


def test_closed_room_reveals_nothing_from_free_space():
    """A scanned closed room has no frontier voxel; a walk takes face steps; so the first unknown voxel on any walk from a free voxel
    would be entered from a frontier voxel or from an occupied one — the first does not exist and the second blocks.  With kept = all
    ones (no frustum at all) every known-free position reveals nothing; with the doorway open the scanner position does."""
    rows = synth.box_room(doorway=False)
    free, _, _, _ = synth.carve_ref(SCANNER, rows, **SCENE)
    occ, _ = synth.occupancy_ref(rows, SCENE["origin"], SCENE["resolution"], SCENE["dims"])
    assert not synth.frontier_ref(occ, free).any() and synth.unknown_ref(occ, free).any()
    kept = np.ones(SCENE["dims"], bool)
    lattice = synth.roadmap_lattice([0.25, 0.25, 0.25], [1.75, 1.75, 0.75], 0.75)
    state = synth.state_ref(lattice, SCENE["origin"], SCENE["resolution"], occ, free)
    assert (state == 1).sum() >= 4
    for t in list(lattice[state == 1][:6]) + [SCANNER]:
        assert synth.view_volume_ref(kept, t, SCENE["origin"], SCENE["resolution"], occ, free)[0] == 0, t
    rows = synth.box_room(doorway=True)
    free, _, _, _ = synth.carve_ref(SCANNER, rows, **SCENE)
    occ, _ = synth.occupancy_ref(rows, SCENE["origin"], SCENE["resolution"], SCENE["dims"])
    gain, rev = synth.view_volume_ref(kept, SCANNER, SCENE["origin"], SCENE["resolution"], occ, free)
    assert gain > 0 and gain == int(rev.sum()) and not (rev & (occ | free)).any()
    x = synth.voxel_centres(SCENE["dims"], SCENE["origin"], SCENE["resolution"])[..., 0]
    assert (x[rev] > SCANNER[0]).all()   # everything it sees lies towards the doorway: a camera looking along -x has it behind
