"""CPU checks of the path refinement (no GPU): the two entry points are declared in the header and in _lib's table without a new ABI
version; tohip_path_bytes is the documented layout and 0 out of range; tohip_path_refine refuses every bad argument before any
launch; the host layer refuses by name before any GPU call; the numpy restatement (synth.path_refine_ref) gives what the definition
dictates on cases small enough to work out by hand; and the doorway scene of the GPU test is what that test assumes, by a brute-force
f64 segment-to-point distance with a 1 cm margin."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from abi_cases import ABI, check_abi_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_path_bytes", "tohip_path_refine")
f32 = np.float32
ONE = 1 << 20   # a metre in the integer lengths' unit


def test_header_and_table_declare_the_path_entries():
    from trajectory_optimization_amd import ops, synth
    header, before = check_abi_entries(ENTRIES)
    assert re.search(rf"\(still {ABI}\) \+ tohip_path_bytes", before)
    for name, v in (("NODES", 1024), ("ROWS", 4096)):
        assert f"#define TOHIP_PATH_MAX_{name} {v}\n" in header
        assert getattr(ops, f"PATH_MAX_{name}") == v == getattr(synth, f"PATH_MAX_{name}")
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert src.index('#include "tour_kernels.hip"') < src.index('#include "path_kernels.hip"')   # the one length function
    kern = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "path_kernels.hip")).read()
    assert "tour_len_fixed(tour_d2(" in kern and "llrint(sqrt" not in kern


def test_path_bytes_is_the_documented_layout():
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for n, R in ((2, 1), (3, 7), (65, 100), (1024, 4096)):
        lay = ops.path_layout(n, R)
        assert L.tohip_path_bytes(n, R) == 256 + up(8 * n) + 2 * up(4 * n) + up(12 * R) + up(16 * R) + up(4 * R) == lay["total"]
        assert lay["D"] == 256 and lay["pred"] == 256 + up(8 * n) and lay["corner"] == lay["pred"] + up(4 * n)
        assert lay["out_poses"] == lay["corner"] + up(4 * n) and lay["out_quats"] == lay["out_poses"] + up(12 * R)
        assert lay["row_node"] == lay["out_quats"] + up(16 * R)
        assert all(v % 256 == 0 for v in lay.values())
    for n, R in ((1, 10), (0, 10), (-3, 10), (1025, 10), (1 << 40, 10), (10, 0), (10, -1), (10, 4097), (10, 1 << 40)):
        assert L.tohip_path_bytes(n, R) == 0, (n, R)


def test_entry_refuses_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    n, R = 100, 500
    nb = L.tohip_path_bytes(n, R)
    names = ("nodes", "quats", "keep", "n_nodes", "window", "open_band", "spacing", "max_rows", "buf", "bytes", "stream")
    base = dict(zip(names, (p, p, p, n, n - 1, p, 0.25, R, p, nb, None)))
    call = lambda **kw: L.tohip_path_refine(*[kw.get(k, base[k]) for k in names])
    for k in ("nodes", "open_band", "buf"):
        assert call(**{k: None}) == EINVAL, k
    for v in (1, 0, -1, 1025, 1 << 40):
        assert call(n_nodes=v, window=1) == EINVAL, v
    for v in (0, -1, n, n + 5, 1 << 40):
        assert call(window=v) == EINVAL, v
    for v in (0, -1, 4097, 1 << 40):
        assert call(max_rows=v) == EINVAL, v
    for v in (-0.25, -float("inf"), float("inf"), float("nan")):
        assert call(spacing=v) == EINVAL, v
    assert call(bytes=nb - 1) == ENOSPC and call(bytes=0) == ENOSPC
    assert call(max_rows=2 * R) == ENOSPC and call(n_nodes=1024, window=5) == ENOSPC   # the buffer of (100, 500) is too short for either
    assert call(bytes=nb - 1, quats=None, keep=None, spacing=0.0) == ENOSPC   # both may be NULL and 0 is no spacing: past the checks


class _Shard:
    def __init__(self, kind="waypoints", world_size=1, collective=False):
        self.kind, self.world_size, self.collective = kind, world_size, collective


def test_host_refusals_come_before_any_gpu_call():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.tools import PlannedPath, Tour, refine_path
    P = torch.zeros(40, 3)
    assert ops.check_path(P) == (40, 39, None, 4096)
    assert ops.check_path(P, torch.ones(40, 4), torch.ones(40, dtype=torch.bool), 5, 0.25, 100) == (40, 5, 0.25, 100)
    assert ops.check_path(torch.zeros(2, 3, dtype=torch.float64), keep=torch.ones(2, dtype=torch.uint8), window=1) == (2, 1, None, 4096)
    bad = [
        (dict(path=[[0, 0, 0], [1, 1, 1]]), "path must be a floating-point tensor"),
        (dict(path=torch.zeros(40, 3, dtype=torch.int32)), "path must be a floating-point tensor"),
        (dict(path=torch.zeros(40, 2)), r"path must be a floating-point tensor of shape \(L,3\)"),
        (dict(path=torch.zeros(1, 3), window=None), "2 <= L <= 1024 nodes, got L = 1"),
        (dict(path=torch.zeros(1025, 3)), "2 <= L <= 1024 nodes, got L = 1025"),
        (dict(quats=torch.ones(40, 3)), r"quats must be None or a floating-point tensor of shape \(40,4\)"),
        (dict(quats=torch.ones(39, 4)), "quats must be None or"), (dict(quats=torch.ones(40, 4, dtype=torch.int64)), "quats must be"),
        (dict(keep=torch.ones(40)), r"keep must be None or a bool / uint8 tensor of shape \(40,\)"),
        (dict(keep=torch.ones(40, dtype=torch.int32)), "keep must be"), (dict(keep=torch.ones(39, dtype=torch.bool)), "keep must be"),
        (dict(keep=[True] * 40), "keep must be"),
        (dict(window=0), r"window must be None or an integer in 1\.\.39"), (dict(window=40), "window must be"),
        (dict(window=2.0), "window must be"), (dict(window=True), "window must be"),
        (dict(spacing=0.0), r"spacing must be None or a finite number > 0"), (dict(spacing=-1.0), "spacing must be"),
        (dict(spacing=float("nan")), "spacing must be"), (dict(spacing=float("inf")), "spacing must be"), (dict(spacing="wide"), "spacing must be"),
        (dict(spacing=1e-60), "spacing must be"), (dict(spacing=1e60), "spacing must be"),
        (dict(max_rows=0), r"max_rows must be None or an integer in 1\.\.4096"), (dict(max_rows=4097), "max_rows must be"),
        (dict(max_rows=10.0), "max_rows must be"), (dict(max_rows=True), "max_rows must be"),
    ]
    for kw, msg in bad:
        args = dict(path=P, quats=None, keep=None, window=5, spacing=0.25, max_rows=100)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.check_path(**args)
    pts = torch.zeros(50, 3)
    for kw, msg in ((dict(path=torch.zeros(1, 3)), "2 <= L"), (dict(path="walk.txt"), "path must be"), (dict(quats=torch.ones(3, 4)), "quats must be"),
                    (dict(keep=torch.ones(40)), "keep must be"), (dict(window=40), "window must be"), (dict(spacing=0), "spacing must be"),
                    (dict(max_rows=5000), "max_rows must be"), (dict(clearance_radius=None), "clearance_radius must be a finite number > 0"),
                    (dict(clearance_radius=0.0), "clearance_radius"), (dict(clearance_radius=float("nan")), "clearance_radius")):
        args = dict(path=P, quats=None, clearance_radius=0.3, spacing=0.25, keep=None, window=None, max_rows=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            refine_path(pts, **args)
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        model = types.SimpleNamespace(_cloud=types.SimpleNamespace(n=50), _shard=shard)
        with pytest.raises(ValueError, match="refine_path: a sharded model"):
            refine_path(model, P, clearance_radius=0.3)
    with pytest.raises(ValueError, match=r"refine_path: points must be an \(N,3\) tensor"):
        refine_path("cloud.pcd", P, clearance_radius=0.3)
    # a Tour and a PlannedPath are unpacked before the checks: what they carry is refused like an argument
    tour = Tour(poses=torch.zeros(1025, 3), quats=None, walk=[0, 1], walk_nodes=None, D=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="keep must be|2 <= L"):
        refine_path(pts, tour, clearance_radius=0.3)
    with pytest.raises(ValueError, match="2 <= L <= 1024 nodes, got L = 1"):
        refine_path(pts, PlannedPath(poses=torch.zeros(1, 3)), clearance_radius=0.3)
    # every argument is fine: the last check before the first GPU call
    with pytest.raises(ValueError, match="refine_path: points must live on a HIP device"):
        refine_path(pts, P, clearance_radius=0.3, spacing=0.25)
    walk = Tour(poses=P[:5], quats=torch.ones(5, 4), walk=[0, 2, 1], walk_nodes=[0, 7, 2, 9, 1], D=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="refine_path: points must live on a HIP device"):
        refine_path(pts, walk, clearance_radius=0.3)
    with pytest.raises(RuntimeError, match="P must live on a HIP device"):
        ops.path_refine(P, None, None, torch.ones(40, 39, dtype=torch.uint8))


def ref(P, keep=None, band=1, window=None, spacing=None, quats=None, max_rows=4096):
    from trajectory_optimization_amd import synth
    P = f32(P)
    W = len(P) - 1 if window is None else window
    ob = np.full((len(P), W), band, dtype=np.uint8) if np.isscalar(band) else np.asarray(band, dtype=np.uint8)
    return synth.path_refine_ref(P, None if keep is None else np.asarray(keep), ob, W, spacing, quats, max_rows)


def test_three_collinear_nodes():
    P = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]
    r = ref(P)   # the chord and the two legs tie at 2 m: the lowest predecessor wins, the middle node goes
    assert r["D"].tolist() == [0, ONE, 2 * ONE] and r["pred"].tolist() == [-1, 0, 0] and r["corners"].tolist() == [0, 2]
    assert (r["m"], r["R"], r["length_fixed"], r["input_length_fixed"], r["n_open"], r["status"]) == (1, 2, 2 * ONE, 2 * ONE, 1, 0)
    assert r["corner"].tolist() == [0, 2, -1] and r["row_node"].tolist() == [0, 2] and r["poses"].tolist() == [[0, 0, 0], [2, 0, 0]]
    k = ref(P, keep=[0, 1, 0])   # kept: the chord over it is not admissible
    assert k["pred"].tolist() == [-1, 0, 1] and k["corners"].tolist() == [0, 1, 2] and k["n_open"] == 0 and k["m"] == 2
    assert k["row_node"].tolist() == [0, 1, 2] and np.array_equal(k["poses"], f32(P))
    w1 = ref(P, window=1)   # a window of one: the input
    assert w1["corners"].tolist() == [0, 1, 2] and w1["n_open"] == 0
    assert ref(P, keep=[1, 1, 1])["corners"].tolist() == [0, 1, 2]
    assert ref(P, keep=[1, 0, 1])["corners"].tolist() == [0, 2]   # the ends are kept anyway


def test_right_angle_with_the_diagonal_open_and_closed():
    P = [[0, 0, 0], [1, 0, 0], [1, 1, 0]]
    diag = int(np.rint(np.sqrt(2.0) * ONE))
    o = ref(P)
    assert o["corners"].tolist() == [0, 2] and o["length_fixed"] == diag == 1482910 and o["input_length_fixed"] == 2 * ONE
    c = ref(P, band=[[1, 0], [1, 1], [1, 1]])   # band[0][1]: the chord (0, 2)
    assert c["corners"].tolist() == [0, 1, 2] and c["length_fixed"] == 2 * ONE and c["n_open"] == 0
    legs = ref(P, band=[[0, 1], [0, 0], [0, 0]])   # column 0, the input legs, is not read: they are always open
    assert legs["corners"].tolist() == [0, 2] and legs["n_open"] == 1
    far = ref([[0, 0, 0], [2e6, 0, 0], [2e6, 1, 0]])   # a chord above 2^40 units is closed, a leg that long is walked all the same
    assert far["corners"].tolist() == [0, 1, 2] and far["n_open"] == 0 and far["length_fixed"] == far["input_length_fixed"] > 1 << 40


def test_a_tie_between_two_routes_goes_to_the_lowest_predecessor():
    P = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]   # 0 -> 2 -> 3 and 0 -> 1 -> 3 are both 2 m; 0 -> 3 is closed
    band = [[1, 1, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0]]
    r = ref(P, band=band)
    assert r["D"].tolist() == [0, ONE, ONE, 2 * ONE] and r["pred"].tolist() == [-1, 0, 0, 1] and r["corners"].tolist() == [0, 1, 3]
    assert r["n_open"] == 2 and r["length_fixed"] == 2 * ONE < r["input_length_fixed"] == 2 * ONE + 1482910
    r2 = ref(P, band=[[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]])   # without (1, 3) the other route is alone
    assert r2["pred"].tolist() == [-1, 0, 0, 2] and r2["corners"].tolist() == [0, 2, 3]


def test_resampling_counts_and_rows():
    from trajectory_optimization_amd import synth
    P = [[0, 0, 0], [1, 0, 0]]
    assert synth.path_spacing_fixed(0.25) == 1 << 18 and synth.path_spacing_fixed(None) == 0 and synth.path_spacing_fixed(1e-9) == 1
    assert synth.path_spacing_fixed(3e38) == 1 << 42
    r = ref(P, spacing=0.25)   # an exact multiple of H: four pieces, not five
    assert r["R"] == 5 and r["row_node"].tolist() == [0, -1, -1, -1, 1] and r["poses"][:, 0].tolist() == [0, 0.25, 0.5, 0.75, 1.0]
    H = synth.path_spacing_fixed(0.3)
    assert H == int(np.rint(float(f32(0.3)) * ONE)) and ref(P, spacing=0.3)["R"] == 1 + -(-ONE // H) == 5
    just = ref([[0, 0, 0], [0.25 + 2.0 ** -20, 0, 0]], spacing=0.25)   # one unit over: a second piece
    assert just["R"] == 3 and just["poses"][1, 0] == f32((0.25 + 2.0 ** -20) / 2)
    big = ref([[0, 0, 0], [1, 0, 0], [1, 2, 0]], keep=[1, 1, 1], spacing=5.0)   # a spacing above every leg: the corners
    assert big["R"] == 3 and big["row_node"].tolist() == [0, 1, 2]
    none = ref([[0, 0, 0], [1, 0, 0], [1, 2, 0]], keep=[1, 1, 1])
    assert none["R"] == 3 and np.array_equal(none["poses"], big["poses"])
    twin = ref([[0, 0, 0], [0, 0, 0], [1, 0, 0]], keep=[1, 1, 1], spacing=0.5)   # a zero-length leg is one piece
    assert twin["R"] == 4 and twin["row_node"].tolist() == [0, 1, -1, 2] and twin["poses"][:, 0].tolist() == [0, 0, 0.5, 1.0]
    third = ref([[1, 2, 3], [2, 4, 7]], spacing=2.0)   # t / n is not exact: the row is the f64 expression, rounded once
    assert third["R"] == 4
    want = [f32(a + (b - a) * (1.0 / 3.0)) for a, b in zip((1.0, 2.0, 3.0), (2.0, 4.0, 7.0))]
    assert third["poses"][1].tolist() == want and third["poses"][0].tolist() == [1, 2, 3] and third["poses"][3].tolist() == [2, 4, 7]
    over = ref(P, spacing=0.25, max_rows=4)
    assert over["status"] == 2 and over["R"] == 5 and over["poses"] is None and over["row_node"] is None and over["corners"].tolist() == [0, 1]
    assert ref(P, spacing=0.25, max_rows=5)["status"] == 0


def test_status_bit_zero():
    assert ref([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0]]) == dict(status=1, m=0, R=0, length_fixed=0, input_length_fixed=0, n_open=0)
    assert ref([[0, 0, 0], [1, np.inf, 0]])["status"] == 1
    q = np.ones((3, 4), dtype=f32)
    P = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]
    q[1] = 0   # a row that is not kept is never read
    assert ref(P, quats=q)["status"] == 0 and ref(P, quats=q, keep=[0, 1, 0])["status"] == 1
    q[1] = [1, np.nan, 0, 0]
    assert ref(P, quats=q)["status"] == 0 and ref(P, quats=q, keep=[0, 1, 0])["status"] == 1
    q[1], q[2] = 1, 0
    assert ref(P, quats=q)["status"] == 1


def test_quaternions_turn_evenly_between_kept_rows():
    s = np.sqrt(0.5)
    P = [[0, 0, 0], [1, 0, 0]]
    q = f32([[2, 0, 0, 0], [0, -3, 0, 0]])   # not normalised, at right angles: no flip
    r = ref(P, spacing=0.5, quats=q)
    assert r["R"] == 3 and r["quats"].dtype == f32
    np.testing.assert_array_equal(r["quats"], f32([[1, 0, 0, 0], [s, -s, 0, 0], [0, -1, 0, 0]]))
    q = f32([[1, 0, 0, 0], [-1, -1, 0, 0]])   # the far hemisphere: the blend runs to -q_b, the kept row keeps its own sign
    r = ref(P, spacing=0.5, quats=q)
    mid = np.array([1 + s, s, 0, 0]) / np.linalg.norm([1 + s, s])
    np.testing.assert_allclose(r["quats"][1], mid, rtol=0, atol=2.0 ** -24)
    np.testing.assert_array_equal(r["quats"][[0, 2]], f32([[1, 0, 0, 0], [-s, -s, 0, 0]]))
    # a corner that is not kept lies between two kept rows by arc length: 1 m of 4 m, and the pieces of the second leg follow on
    P = [[0, 0, 0], [1, 0, 0], [1, 3, 0]]
    q = f32([[1, 0, 0, 0], [9, 9, 9, 9], [0, 0, 1, 0]])
    r = ref(P, band=0, spacing=1.5, quats=q)
    assert r["corners"].tolist() == [0, 1, 2] and r["row_node"].tolist() == [0, 1, -1, 2]
    for row, u in ((1, 0.25), (2, (1 + 1.5) / 4)):
        v = np.array([1 - u, 0, u, 0])
        np.testing.assert_allclose(r["quats"][row], v / np.linalg.norm(v), rtol=0, atol=2.0 ** -24)
    np.testing.assert_array_equal(r["quats"][[0, 3]], f32([[1, 0, 0, 0], [0, 0, 1, 0]]))
    # kept twins: S_ab = 0, u = 0
    r = ref([[0, 0, 0], [0, 0, 0], [0, 0, 0]], quats=q, band=0)
    np.testing.assert_array_equal(r["quats"], f32([[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]]))


def test_invariants_on_random_paths():
    from trajectory_optimization_amd import synth
    rng = np.random.default_rng(8)
    for trial in range(20):
        L = int(rng.integers(2, 40))
        W = int(rng.integers(1, L))
        P = (rng.integers(-8, 9, size=(L, 3)) * 0.25).astype(f32)   # a coarse grid: ties and twins
        keep = rng.random(L) < 0.2
        band = (rng.random((L, W)) < 0.6).astype(np.uint8)
        h = float(rng.choice([0.25, 0.4, 3.0]))
        r = synth.path_refine_ref(P, keep, band, W, h)
        cs = r["corners"].tolist()
        assert cs[0] == 0 and cs[-1] == L - 1 and cs == sorted(set(cs)) and set(np.flatnonzero(keep)) <= set(cs)
        assert r["length_fixed"] <= r["input_length_fixed"] and r["row_node"][r["row_node"] >= 0].tolist() == cs
        w = synth.path_chord_lengths(P)
        assert r["length_fixed"] == sum(int(w[a, b]) for a, b in zip(cs, cs[1:]))
        for a, b in zip(cs, cs[1:]):
            assert b - a <= W and (b == a + 1 or (band[a, b - a - 1] and not keep[a + 1:b].any()))
        step = np.linalg.norm(np.diff(r["poses"].astype(np.float64), axis=0), axis=1)
        assert (step <= h + 2.0 ** -20 + 1e-6).all()   # (1e-6: the rows' own f32 rounding at |x| <= 2)
        assert synth.path_refine_ref(P, keep, band[:, :1], 1, None)["corners"].tolist() == list(range(L))
        assert synth.path_refine_ref(P, np.ones(L), band, W, None)["corners"].tolist() == list(range(L))


def segment_point_distance(A, B, P):
    """The smallest distance from each segment A[e] -> B[e] to the points P, brute force in f64."""
    A, B, P = A.astype(np.float64), B.astype(np.float64), P.astype(np.float64)
    out = np.empty(len(A))
    for s in range(0, len(A), 128):
        a, e = A[s:s + 128, None, :], (B[s:s + 128] - A[s:s + 128])[:, None, :]
        ee = (e * e).sum(-1)
        u = P[None] - a
        t = np.clip((u * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        q = u - t[..., None] * e
        out[s:s + 128] = np.sqrt((q * q).sum(-1)).min(axis=1)
    return out


def doorway_walk():
    """The walk plan_path gives from node 0 to node 4 of the doorway scene, by the restatements and a brute-force edge stage."""
    from trajectory_optimization_amd import synth
    sc = synth.doorway_scene()
    pts, r = sc["points"], sc["radius"]
    Q = synth.roadmap_join(sc["nodes"][[0, 4]], sc["lattice"])
    nbr, length = synth.roadmap_knn_ref(Q, 12)
    ii, jj = np.repeat(np.arange(len(Q)), 12), nbr.reshape(-1)
    f = jj >= 0
    near = pts[(pts[:, 2] > 0.5 - r - 0.1) & (pts[:, 2] < 1.5 + r + 0.1)]
    de = segment_point_distance(Q[np.minimum(ii, jj)[f]], Q[np.maximum(ii, jj)[f]], near)
    assert (np.abs(de - r) > 0.01).all()
    opened = np.zeros(nbr.shape, dtype=bool)
    opened.reshape(-1)[f] = de > r
    D, pred = synth.roadmap_routes_ref(nbr, length, opened, [0])
    return sc, near, Q[synth.roadmap_walk(pred[0], 0, 1)]


def test_doorway_scene_is_what_the_gpu_test_assumes():
    from trajectory_optimization_amd import synth
    sc, near, walk = doorway_walk()
    r, margin, L = sc["radius"], 0.01, len(walk)
    assert L > 4 and ((np.abs(walk[:, 0]) <= 0.5) & (np.abs(walk[:, 1]) < 0.5)).any()
    i, j = np.triu_indices(L, 1)
    d = segment_point_distance(walk[i], walk[j], near)
    assert (np.abs(d - r) > margin).all()   # no chord of the walk is a close call: the device's band is this one
    band = np.zeros((L, L - 1), dtype=np.uint8)
    band[i, j - i - 1] = d > r
    assert band[np.arange(L - 1), 0].all()   # leg_blocked is all false
    assert band[i, j - i - 1][j >= i + 2].any() and not band[0, L - 2]   # a shortcut is open; the straight line through the wall is not
    got = synth.path_refine_ref(walk, None, band, L - 1, 0.25)
    assert got["m"] + 1 < L and got["length_fixed"] < got["input_length_fixed"]   # fewer corners, strictly shorter
    cs = got["corners"]
    assert (segment_point_distance(walk[cs[:-1]], walk[cs[1:]], near) > r + margin).all()   # the refined legs, hence their pieces
    rows = got["poses"]
    assert (segment_point_distance(rows[:-1], rows[1:], near) > r + margin).all()
    every = synth.path_refine_ref(walk, np.ones(L), band, L - 1, 0.25)
    assert every["corners"].tolist() == list(range(L))
