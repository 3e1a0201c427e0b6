"""CPU checks of the ground layer (no GPU): the two entry points are declared in the header and in _lib's table at ABI 15 and refuse
bad arguments — a non-zero `flags` among them — before any launch; ops.check_ground refuses by name; and synth.ground_ref, what the
kernels are compared against bit for bit, is checked against a naive per-voxel loop written from the five numbered rules of DESIGN.md
10 "Ground layer", on the five hand scenes of that section and on its set relations."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

EINVAL, ENOSPC = -1, -2
ENTRIES = ["tohip_ground_build", "tohip_ground_snap"]
PLANES = ("support", "ground", "floor", "obstacles", "drive")


def test_header_and_table_declare_the_new_entries_at_abi_15():
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_ground_build / tohip_ground_snap" in before
    for sym in ENTRIES:   # `..., void *stream, uint32_t flags)`: the reserved word comes last
        assert " ".join(header.split("int " + sym + "(")[1].split(";")[0].split()).endswith("void *stream, uint32_t flags)")


def test_entries_refuse_bad_arguments_and_flags_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    occ, fre, a, b, c, d, e = (ctypes.c_void_p(v) for v in (4096, 8192, 16384, 32768, 65536, 131072, 262144))   # pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, dims=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*dims))
    ok, nb = geom(), L.tohip_occ_bytes(64, 64, 32)
    calls = {
        "build": (L.tohip_ground_build, ("occ", "free", "grid_bytes", "geom", "H", "s", "known", "support", "ground", "obstacles", "drive", "stream",
                                         "flags"), (occ, None, nb, ok, 4, 1, 0, a, b, c, d, None, 0)),
        "snap": (L.tohip_ground_snap, ("ground", "drive", "grid_bytes", "geom", "pos", "m", "max_drop", "standing", "drop", "stream", "flags"),
                 (a, b, nb, ok, c, 10, 3, d, e, None, 0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, v) for k, v in zip(names, base)])

    for name in calls:
        for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
            assert call(name, flags=flags) == EINVAL, (name, flags)
        assert call(name, geom=None) == EINVAL and call(name, grid_bytes=nb - 1) == ENOSPC, name
        for g in (geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(dims=(0, 64, 32)), geom(dims=(64, 2049, 32))):
            assert call(name, geom=g) == EINVAL, name
    for kw in (dict(occ=None), dict(H=0), dict(H=65), dict(s=-1), dict(s=5), dict(H=2, s=2), dict(H=1, s=1), dict(known=2), dict(known=-1),
               dict(known=1), dict(support=None), dict(ground=None), dict(obstacles=None), dict(drive=None), dict(support=occ), dict(drive=occ),
               dict(ground=a), dict(obstacles=b), dict(drive=c), dict(known=1, free=a), dict(known=1, free=d),
               dict(support=ctypes.c_void_p(16386))):
        assert call("build", **kw) == EINVAL, kw
    for kw in (dict(ground=None), dict(drive=None), dict(pos=None), dict(standing=None), dict(drop=None), dict(m=-1), dict(max_drop=-1),
               dict(max_drop=2049)):
        assert call("snap", **kw) == EINVAL, kw
    assert call("snap", m=0, pos=None, standing=None, drop=None) == 0   # (an empty query launches nothing)


def test_check_ground_names_every_refusal():
    from trajectory_optimization_amd import ops

    class G(ops.OccupancyGrid):   # a grid's geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    g = G()
    space = ops.SpaceMap(g, G())
    assert ops.check_ground(g, 0.4) == (g, None, 4, 1) and ops.check_ground(space, 0.4, 0) == (g, None, 4, 0)
    assert ops.check_ground(space, 0.4, 2, "obstacle") == (g, space.free, 4, 2)
    # H = ceil(f64(headroom) / f64(f32 resolution)): 0.1f is a little above 0.1, so 0.4 m is 4 voxels and 0.41 m is 5
    assert ops.check_ground(g, 0.41)[2] == 5 == synth.ground_headroom_voxels(0.41, 0.1) and ops.check_ground(G(resolution=0.125), 1.0)[2] == 8
    assert ops.check_ground(g, None, 0, H=np.int64(1))[2:] == (1, 0) and ops.check_ground(g, 6.4)[2] == 64
    for bad in (None, object(), torch.zeros(4, 3)):
        with pytest.raises(ValueError, match="the map must be an ops.OccupancyGrid, an ops.SpaceMap or an ops.EvidenceMap"):
            ops.check_ground(bad, 0.4)
    for bad in (None, "tall", 0.0, -1.0, float("nan"), float("inf"), 6.6, True):
        with pytest.raises(ValueError, match="headroom must be a finite number of metres > 0 and at most 64 voxels"):
            ops.check_ground(g, bad)
    for bad in (0, 65, 2.0, "4"):
        with pytest.raises(ValueError, match=r"H must be an integer number of voxels in \[1, 64\]"):
            ops.check_ground(g, None, 0, H=bad)
    for bad in (-1, 5, 1.0, None, "1"):
        with pytest.raises(ValueError, match=r"step must be an integer number of voxels in \[0, 4\]"):
            ops.check_ground(g, 1.0, bad)
    with pytest.raises(ValueError, match="step 2 needs a headroom of at least 3 voxels"):
        ops.check_ground(g, 0.2, 2)
    with pytest.raises(ValueError, match="unknown must be 'free' or 'obstacle'"):
        ops.check_ground(g, 0.4, 1, "maybe")
    with pytest.raises(ValueError, match="unknown='obstacle' needs an ops.SpaceMap or an ops.EvidenceMap"):
        ops.check_ground(g, 0.4, 1, "obstacle")
    for bad in (-1, 2049, 1.5, "3"):
        with pytest.raises(ValueError, match=r"max_drop must be an integer number of voxels in \[0, 2048\]"):
            ops.check_ground(g, 0.4, max_drop=bad)
    assert ops.check_ground(g, 0.4, max_drop=np.int32(2048))[2] == 4


# ---- the reference against a naive loop -------------------------------------------------------------------------------------------

def naive_ground(occ, free, H, s, unknown):
    """The five rules, voxel by voxel."""
    nx, ny, nz = occ.shape
    known = unknown == "obstacle"
    inside = lambda x, y, z: 0 <= x < nx and 0 <= y < ny and 0 <= z < nz   # noqa: E731

    def clear(x, y, z):
        if not inside(x, y, z):
            return not known
        return not occ[x, y, z] and (not known or bool(free[x, y, z]))

    out = {k: np.zeros(occ.shape, dtype=bool) for k in PLANES}
    sup, gr, fl, ob, dr = (out[k] for k in PLANES)
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):                                  # rule 1
        sup[x, y, z] = occ[x, y, z] and all(clear(x, y, z + k) for k in range(1, H + 1))
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):                                  # rule 2
        if not sup[x, y, z]:
            continue
        fine = 0
        for dx, dy in itertools.product((-1, 0, 1), repeat=2):
            cx, cy = x + dx, y + dy
            if (dx == 0 and dy == 0) or not (0 <= cx < nx and 0 <= cy < ny):
                continue
            a = any(inside(cx, cy, zz) and sup[cx, cy, zz] for zz in range(z - s, z + s + 1))
            b = any(inside(cx, cy, z + k) and occ[cx, cy, z + k] for k in range(1, H + 1))
            fine += a or b
        gr[x, y, z] = fine == 8
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):                                  # rules 3 and 4
        if occ[x, y, z]:
            top = z
            while top + 1 < nz and occ[x, y, top + 1]:
                top += 1
            fl[x, y, z] = gr[x, y, top]
        ob[x, y, z] = (occ[x, y, z] and not fl[x, y, z]) or (known and not occ[x, y, z] and not free[x, y, z])
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):                                  # rule 5
        dr[x, y, z] = not occ[x, y, z] and any(z - k >= 0 and gr[x, y, z - k] for k in range(1, s + 2))
    return out


def random_map(dims, fill, seed):
    """A random occupied plane and a free plane over four fifths of the rest; half the seeds get a solid bottom, so that ground exists."""
    rng = np.random.default_rng(seed)
    occ = rng.random(dims) < fill
    if seed % 2 == 0:
        occ[:, :, 0] = True
    free = (rng.random(dims) < 0.8) & ~occ
    return occ, free


@pytest.mark.parametrize("dims", [(5, 6, 3), (13, 11, 9)])
@pytest.mark.parametrize("fill", [0.05, 0.30, 0.70])
def test_ground_ref_equals_the_naive_loop(dims, fill):
    n = 0
    for seed, unknown, (H, s) in itertools.product((0, 1), synth.GROUND_UNKNOWN, [(H, s) for H in (1, 3, 64) for s in (0, 1, 2) if s + 1 <= H]):
        occ, free = random_map(dims, fill, 100 * seed + int(100 * fill) + dims[0])
        got, want = synth.ground_ref(occ, free, H, s, unknown), naive_ground(occ, free, H, s, unknown)
        for k in PLANES:
            assert np.array_equal(got[k], want[k]), (seed, unknown, H, s, k)
        n += got["ground"].sum()
    assert n > 0   # (some case has ground)


def test_ground_ref_refuses_bad_settings():
    occ = np.zeros((4, 4, 4), dtype=bool)
    for kw in (dict(headroom=0), dict(headroom=65), dict(step=-1), dict(step=5), dict(headroom=2, step=2), dict(unknown="maybe"),
               dict(unknown="obstacle")):
        with pytest.raises(ValueError):
            synth.ground_ref(occ, None, **kw)


# ---- the five hand scenes ---------------------------------------------------------------------------------------------------------

D_HAND, START = 6, (2, 4, 1)


def flat_floor(dims):
    occ = np.zeros(dims, dtype=bool)
    occ[:, :, 0] = True
    return occ


def travel_over(occ, H, s, need2=1):
    """(layer, T, cost): the layer of `occ`, the travel build's traversable set (field over the obstacles >= need2 and state 1 of
    SpaceMap(obstacles, drive)) and the travel field from START."""
    layer = synth.ground_ref(occ, None, H, s)
    field = synth.field_ref(layer["obstacles"], D=D_HAND)
    state = np.where(layer["obstacles"], 2, np.where(layer["drive"], 1, 0))
    T = synth.travel_traversable_ref(field, need2, state)
    return layer, T, synth.travel_ref(T, [START])


def test_wall_with_a_door():
    occ = flat_floor((24, 9, 12))
    occ[12, :, 1:10] = True
    occ[12, 3:6, 1:8] = False
    _, _, cost = travel_over(occ, 4, 1)
    assert cost[20, 4, 1] == 1152 and cost[12, 4, 1] == 640 and cost[12, 0, 1] == -1
    assert int((cost[:, :, 1] >= 0).sum()) == 88


def test_ramp_one_to_one():
    occ = np.zeros((24, 9, 20), dtype=bool)
    height = np.clip(np.arange(24) - 8, 0, 6)
    for x in range(24):
        occ[x, :, :height[x] + 1] = True
    layer, _, cost = travel_over(occ, 4, 1)
    for x in range(1, 23):   # every interior surface voxel is ground
        assert layer["ground"][x, 1:8, height[x]].all(), x
    assert cost[20, 4, 7] == 1499
    assert not layer["ground"][0].any() and not layer["ground"][:, 0].any()   # the outermost ring is never ground


def test_solid_ramp_is_floor_down_to_the_bottom_and_the_outer_ring_is_an_obstacle():
    occ = np.zeros((24, 9, 20), dtype=bool)
    height = np.clip(np.arange(24) - 8, 0, 6)
    for x in range(24):
        occ[x, :, :height[x] + 1] = True
    layer = synth.ground_ref(occ, None, 4, 1)
    ring = np.ones((24, 9), dtype=bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(layer["obstacles"], occ & ring[:, :, None])


def test_two_voxel_riser():
    occ = flat_floor((24, 9, 12))
    occ[12:, :, 1:3] = True
    layer, _, cost = travel_over(occ, 4, 1)
    assert cost[20, 4, 3] == -1 and not layer["ground"][12, 4, 2] and layer["ground"][14, 4, 2]
    layer, _, cost = travel_over(occ, 4, 2)
    assert cost[20, 4, 3] == 1206 and layer["ground"][12, 4, 2] and layer["ground"][14, 4, 2]


def test_thin_table():
    occ = flat_floor((24, 9, 12))
    occ[10:14, :, 5] = True
    _, _, cost = travel_over(occ, 4, 1)
    assert cost[20, 4, 1] == 1152   # it passes under
    layer, _, cost = travel_over(occ, 6, 1)
    assert cost[20, 4, 1] == -1 and not layer["support"][12, 4, 0]


def test_pit():
    occ = flat_floor((24, 9, 12))
    occ[10:13, 3:6, 0] = False
    _, T, _ = travel_over(occ, 4, 1, need2=4)
    assert "".join("#" if t else "." for t in T[:, 4, 1]) == "...####.........#####..."


# ---- properties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("unknown", synth.GROUND_UNKNOWN)
def test_set_relations(unknown):
    for seed, fill, (H, s) in itertools.product(range(4), (0.05, 0.3, 0.7), ((1, 0), (3, 1), (5, 4), (64, 2))):
        occ, free = random_map((13, 11, 9), fill, seed)
        p = synth.ground_ref(occ, free, H, s, unknown)
        assert not (p["drive"] & occ).any() and not (p["floor"] & ~occ).any() and not (p["ground"] & ~p["support"]).any()
        assert not (p["ground"] & ~p["floor"]).any() and not (p["drive"] & p["obstacles"]).any()
        assert np.array_equal(p["obstacles"] & occ, occ & ~p["floor"])
        if unknown == "obstacle":
            assert np.array_equal(p["obstacles"] & ~occ, ~occ & ~free)
        else:
            assert not (p["obstacles"] & ~occ).any()
        # a standing voxel lies right above every ground voxel that has a voxel above it
        assert np.array_equal(p["drive"][:, :, 1:] | ~p["ground"][:, :, :-1], np.ones_like(occ[:, :, 1:]))


def test_flat_floor_with_walls_gives_the_field_of_the_scene_without_its_floor():
    occ = flat_floor((20, 14, 10))
    occ[0, :, :] = occ[-1, :, :] = occ[:, 0, :] = occ[:, -1, :] = True   # walls to the top
    occ[8, 1:9, 1:7] = True                                                # a partition
    occ[13:16, 4:7, 1:3] = True                                            # a box
    layer = synth.ground_ref(occ, None, 4, 1)
    bare = occ.copy()
    bare[:, :, 0] = False
    # the floor under the walls, the partition and the box is not floor (their runs do not end in ground): at standing height the
    # field over the layer's obstacles is that of the scene with its floor deleted
    got, want = synth.field_ref(layer["obstacles"], D=D_HAND), synth.field_ref(bare, D=D_HAND)
    assert np.array_equal(got[:, :, 1], want[:, :, 1])
    assert synth.field_ref(occ, D=D_HAND)[:, :, 1].max() == 0   # ... where the plain field over the map refuses every voxel


def test_snap_ref_on_a_step():
    occ = flat_floor((12, 7, 10))
    occ[6:, :, 1:3] = True
    layer = synth.ground_ref(occ, None, 3, 2)
    o, r = (-0.3, 0.2, 1.0), 0.25
    centre = lambda v: (np.float32(o) + ((np.asarray(v, dtype=np.float32) + np.float32(0.5)) * np.float32(r)).astype(np.float32))   # noqa: E731
    pos = np.stack([centre((3, 3, 1)), centre((3, 3, 4)), centre((3, 3, 6)), centre((8, 3, 5)), centre((8, 3, 1)), centre((0, 3, 3)),
                    centre((3, 3, 12)), (np.nan, 0, 0), (1e6, 0, 0),
                    np.float32(o) + np.float32(r) * np.asarray((3, 3, 2), dtype=np.float32)]).astype(np.float32)
    standing, drop = synth.ground_snap_ref(pos, o, r, layer["ground"], layer["drive"], 4)
    # standing voxel, 3 below, out of reach (5 below), on the step (2 below), inside the step, over the outer ring, outside dims,
    # not finite, out of range, exactly on the face between levels 1 and 2 (the voxel above the face: 1 below)
    assert drop.tolist() == [0, 3, -1, 2, -1, -1, -2, -2, -2, 1]
    assert np.array_equal(standing[0], centre((3, 3, 1))) and np.array_equal(standing[1], centre((3, 3, 1)))
    assert np.array_equal(standing[3], centre((8, 3, 3))) and np.array_equal(standing[9], centre((3, 3, 1)))
    assert np.isnan(standing[[2, 4, 5, 6, 7, 8]]).all()


def test_pack_is_the_brick_layout():
    bits = np.zeros((5, 6, 3), dtype=bool)
    bits[1, 2, 1] = bits[4, 5, 2] = bits[0, 0, 0] = True
    words = synth.ground_pack(bits)
    assert words.shape == (2 * 2 * 2,) and words.dtype == np.uint32
    assert words[0] == (1 << 0) | (1 << (1 | 2 << 2 | 1 << 4)) and words[(1 * 2 + 1) * 2 + 1] == 1 << (0 | 1 << 2 | 0 << 4)
    assert int(sum(bin(int(w)).count("1") for w in words)) == 3
