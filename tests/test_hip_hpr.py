"""Hidden-point removal on the GPU: bit-exact visible-point index sets vs the reference (golden) and vs
the oracle (scipy/Qhull, the hull the reference itself calls) at sizes beyond the fixtures."""
import numpy as np
import pytest
import torch

from conftest import load_golden, lowest_identical_rows, rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ["hpr_synth_outside", "hpr_synth_10k", "hpr_shell_origin_inside", "hpr_bundled_world",
                                  "hpr_synth_100k"])
def test_hpr_index_sets_bit_exact(dev, name):
    from trajectory_optimization_amd.tools import hidden_pts_removal, convexHull, sphericalFlip
    d = load_golden(name)
    pts = torch.from_numpy(d["points"]).to(dev)
    vis, mask = hidden_pts_removal(pts, dev)
    idx = np.flatnonzero(mask.cpu().numpy())
    assert np.array_equal(idx, d["visible_idx"])
    assert np.array_equal(vis.cpu().numpy(), d["points"][d["visible_idx"]])
    if "hull_vertices" in d:
        hull = convexHull(sphericalFlip(pts, dev, 2), dev)
        assert np.array_equal(hull.vertices.cpu().numpy(), d["hull_vertices"])
        assert bool(hull.vertices[-1].item() == len(d["points"])) == bool(d["origin_is_vertex"])


def test_hard_pipeline_bit_exact(dev):
    """pc_processor.run: transform -> hard cull -> HPR (22742 / 6699 / 4440 / 677)."""
    from trajectory_optimization_amd.tools import visible_points_from_camera
    d = load_golden("hard_pipeline_bundled")
    r = visible_points_from_camera(torch.from_numpy(d["points"]).to(dev), torch.from_numpy(d["trans"]).to(dev),
                                   torch.from_numpy(d["quat"]).to(dev), torch.from_numpy(K).to(dev), IH, IW,
                                   float(d["min_dist"]), float(d["max_dist"]))
    assert np.array_equal(r["kept_idx"].cpu().numpy(), d["kept_idx"]) and len(d["kept_idx"]) == 4440
    assert np.array_equal(r["kept_points"].cpu().numpy(), d["kept_pts"])
    assert np.array_equal(r["visible_idx"].cpu().numpy(), d["hpr_visible_idx"]) and len(d["hpr_visible_idx"]) == 677
    assert np.array_equal(r["visible_points"].cpu().numpy(), d["hpr_visible_pts"])


@pytest.mark.parametrize("name", ["pose_bundled_hpr", "pose_synth_10k_hpr"])
def test_model_pose_hpr(dev, name):
    from trajectory_optimization_amd.model import ModelPose
    d = load_golden(name)
    m = ModelPose(points=torch.from_numpy(d["points"]), trans0=torch.from_numpy(d["trans0"]), q0=torch.from_numpy(d["q0"]),
                  intrins=torch.from_numpy(K), img_width=IW, img_height=IH, device=dev)
    loss = m(hpr=True)
    loss.backward()
    assert abs(loss.item() - float(d["loss"])) <= 5e-6 * float(d["loss"])
    obs = m.observations.detach().cpu().numpy()
    # same occluded set: every point the reference zeroes is zero here (values below 1e-37 may underflow
    # differently, so the converse is checked on the mask itself)
    assert np.all(obs[d["observations"] == 0] < 1e-37)
    from oracle import oracle
    assert np.array_equal(np.flatnonzero(m._occlusion_mask.cpu().numpy()), oracle.hidden_pts_removal(d["points"])[0])
    np.testing.assert_allclose(obs, d["observations"], rtol=5e-5, atol=1e-9)
    assert rel_inf(m.trans.grad.cpu().numpy(), d["trans_grad"]) < 1e-5
    assert rel_inf(m.quat.grad.cpu().numpy(), d["quat_grad"]) < 1e-5


@pytest.mark.parametrize("n,seed,centre", [(1_000_000, 0, (0.0, 0.0, 0.0)), (300_000, 3, (25.0, -3.0, 1.0))])
def test_hpr_large_vs_qhull(dev, n, seed, centre):
    """BASELINE-size cloud: index set equal to scipy/Qhull on the same flipped points (oracle)."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(n, seed=seed) - np.asarray(centre, dtype=np.float32)
    vis_ref, _ = oracle.hidden_pts_removal(pts)
    idx, mask = ops.hidden_pts_removal(torch.from_numpy(pts).to(dev))
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), vis_ref)
    assert int(mask.sum().item()) == len(vis_ref)


def test_hpr_degenerate_inputs(dev):
    from trajectory_optimization_amd import ops, _lib
    flat = torch.zeros(100, 3, device=dev)
    flat[:, 0] = torch.arange(1, 101, device=dev)  # collinear with the origin: no 3-D hull (Qhull: QH6154)
    with pytest.raises(_lib.HipError):
        ops.hidden_pts_removal(flat)
    with pytest.raises(_lib.HipError):
        ops.hidden_pts_removal(torch.rand(3, 3, device=dev))  # fewer than 4 points
    # a zero-norm point flips to NaN (tools.py:49-52) and scipy refuses: "Points cannot contain NaN" 
    pts = torch.from_numpy(synth.make_cloud(2000, seed=4)).to(dev)
    pts[17] = 0.0
    with pytest.raises(ValueError, match="NaN"):
        ops.hidden_pts_removal(pts)
    good = torch.from_numpy(synth.make_cloud(3000, seed=5)).to(dev)
    idx, voff, mask, status = ops.hidden_pts_removal_batched(torch.cat([pts, good]), [0, 2000, 5000])
    assert status.tolist() == [3, 0] and voff.tolist()[:2] == [0, 0]
    one, _ = ops.hidden_pts_removal(good)
    assert torch.equal(idx - 2000, one)


def test_hpr_batched_matches_qhull_per_segment(dev):
    """Many viewpoints in one pass: every segment's visible set equals scipy/Qhull's on that segment alone, with its
    own flip radius and its own dropped last vertex; short, empty and flat segments report a status and nothing else."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(11)
    segs = []
    for k, n in enumerate([5000, 0, 37, 3, 12000, 800, 4, 25000, 1]):
        c = rng.uniform(-15, 15, 3).astype(np.float32) * (k % 3 != 0)  # some viewpoints inside their cloud, some outside
        segs.append(synth.make_cloud(n, seed=20 + k) * np.float32(0.5 + 0.2 * k) - c if n else np.zeros((0, 3), np.float32))
    flat = np.zeros((50, 3), np.float32)
    flat[:, 0] = np.arange(1, 51)
    flat[:, 1] = rng.uniform(-1, 1, 50)  # coplanar with the appended origin (z = 0)
    segs.insert(4, flat)
    # origin strictly inside a closed shell: the origin is no hull vertex and the highest real vertex is dropped
    u = rng.normal(size=(3000, 3))
    segs.append((u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(4, 6, (3000, 1))).astype(np.float32))
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    allp = np.concatenate(segs).astype(np.float32)
    idx, voff, mask, status = ops.hidden_pts_removal_batched(torch.from_numpy(allp).to(dev), offs)
    idx, mask, status = idx.cpu().numpy().astype(np.int64), mask.cpu().numpy(), status.cpu().numpy()
    assert voff[0] == 0 and voff[-1] == len(idx)
    for s, pts in enumerate(segs):
        got = idx[voff[s]:voff[s + 1]] - offs[s]
        if len(pts) < 4:
            assert status[s] == 1 and len(got) == 0
        elif s == 4:
            assert status[s] == 2 and len(got) == 0
        else:
            ref, ref_mask = oracle.hidden_pts_removal(pts)
            assert status[s] == 0
            assert np.array_equal(got, ref), f"segment {s}"
            assert np.array_equal(mask[offs[s]:offs[s + 1]], ref_mask)
            one, _ = ops.hidden_pts_removal(torch.from_numpy(pts).to(dev))
            assert np.array_equal(one.cpu().numpy(), got)


def test_hpr_batched_single_segment_and_errors(dev):
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(synth.make_cloud(20000, seed=2)).to(dev)
    idx, voff, mask, status = ops.hidden_pts_removal_batched(pts, [0, 20000])
    one, one_mask = ops.hidden_pts_removal(pts)
    assert torch.equal(idx, one) and torch.equal(mask, one_mask) and status.tolist() == [0] and voff.tolist() == [0, one.numel()]
    with pytest.raises(ValueError):
        ops.hidden_pts_removal_batched(pts, [0, 100])
    with pytest.raises(Exception):
        ops.hidden_pts_removal_batched(pts, [0, 15000, 10000, 20000])  # offsets must not decrease


def test_hard_pipeline_many_cameras(dev):
    """The per-camera pipeline over a rig in one batched hull pass == camera by camera (and camera 0 == the golden run)."""
    from trajectory_optimization_amd.tools import visible_points_from_camera, visible_points_from_cameras
    d = load_golden("hard_pipeline_bundled")
    pts = torch.from_numpy(d["points"]).to(dev)
    rq, _ = synth.camera_rig(5)
    quats = np.stack([synth.quat_mul(d["quat"].reshape(4), q) for q in rq]).astype(np.float32)
    trans = np.repeat(d["trans"].reshape(1, 3), 5, axis=0) + np.arange(5, dtype=np.float32)[:, None] * np.float32(0.5)
    args = (torch.from_numpy(K).to(dev), IH, IW, float(d["min_dist"]), float(d["max_dist"]))
    many = visible_points_from_cameras(pts, torch.from_numpy(trans).to(dev), torch.from_numpy(quats).to(dev), *args)
    assert len(many) == 5
    for c in range(5):
        one = visible_points_from_camera(pts, torch.from_numpy(trans[c]).to(dev), torch.from_numpy(quats[c]).to(dev), *args)
        for k in ("kept_idx", "kept_points", "visible_idx", "visible_points"):
            assert torch.equal(many[c][k], one[k]), (c, k)
    assert np.array_equal(many[0]["visible_idx"].cpu().numpy(), d["hpr_visible_idx"])


def test_hpr_batched_many_small_segments(dev):
    """A thousand tiny viewpoints (sizes 0..60, many below the 4 points a hull needs) and an all-empty batch."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 61, 1000)
    segs = [(rng.normal(size=(n, 3)) * 3 + rng.uniform(-8, 8, 3)).astype(np.float32) for n in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    idx, voff, mask, status = ops.hidden_pts_removal_batched(torch.from_numpy(np.concatenate(segs)).to(dev), offs)
    idx, status = idx.cpu().numpy().astype(np.int64), status.cpu().numpy()
    checked = 0
    for s in range(0, 1000, 7):
        got = idx[voff[s]:voff[s + 1]] - offs[s]
        if sizes[s] < 4:
            assert status[s] == 1 and len(got) == 0
            continue
        assert status[s] == 0
        assert np.array_equal(got, oracle.hidden_pts_removal(segs[s])[0]), s
        checked += 1
    assert checked > 100
    assert np.array_equal(status[sizes < 4], np.ones((sizes < 4).sum(), np.int32))
    idx, voff, mask, status = ops.hidden_pts_removal_batched(torch.empty((0, 3), device=dev), [0, 0, 0])
    assert idx.numel() == 0 and voff.tolist() == [0, 0, 0] and status.tolist() == [1, 1] and mask.numel() == 0


def test_hpr_batched_ten_thousand_segments_walked_eight_to_a_wave(dev):
    """10 000 viewpoints of 24 points on a sphere of radius 3: round 0 has about four candidates per segment, more than the
    32 768 from which the host launches k_owner_claim_sub (eight walks to a wave), and the segments are far too small for the
    sample phase.  Every 97th segment against Qhull on that segment alone; two calls agree bit for bit."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(17)
    nseg, per = 10_000, 24
    v = rng.normal(size=(nseg, per, 3))
    v *= 3.0 / np.linalg.norm(v, axis=2, keepdims=True)
    pts = (v + rng.uniform(-8, 8, (nseg, 1, 3))).astype(np.float32)
    offs = np.arange(nseg + 1) * per
    cloud = torch.from_numpy(pts.reshape(-1, 3)).to(dev)
    idx, voff, mask, status = ops.hidden_pts_removal_batched(cloud, offs)
    idx2, voff2, mask2, status2 = ops.hidden_pts_removal_batched(cloud, offs)
    assert torch.equal(idx, idx2) and torch.equal(voff, voff2) and torch.equal(mask, mask2) and torch.equal(status, status2)
    assert voff[0] == 0 and voff[-1] == len(idx)
    idx, voff, status = idx.cpu().numpy().astype(np.int64), voff.numpy(), status.cpu().numpy()
    for s in range(0, nseg, 97):
        assert status[s] == 0, s
        assert np.array_equal(idx[voff[s]:voff[s + 1]] - offs[s], oracle.hidden_pts_removal(pts[s])[0]), s


def test_hull_all_points_on_a_sphere_retries_with_a_larger_face_pool(dev):
    """Every point a hull vertex: the default face pool / face lists run out (TOHIP_ENOSPC) and ops retries with 4x the bytes."""
    from scipy.spatial import ConvexHull
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(11)
    v = rng.normal(size=(300_000, 3))
    pts = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    got = ops.hull_vertices_with_origin(torch.from_numpy(pts).to(dev), False).cpu().numpy()
    ref = np.sort(ConvexHull(pts.astype(np.float64)).vertices)
    assert np.array_equal(got.astype(np.int64), ref)


def test_hull_careful_path_in_a_child_process():
    """The slow path of the hull build (ownership propagated to convergence with the host checking, taken after a round that
    accepts nobody) is switched on for a whole process by TOHIP_HULL_CAREFUL: same index sets."""
    import os, subprocess, sys
    from conftest import REPO
    code = ("import sys, numpy as np, torch; sys.path.insert(0, 'tests'); from conftest import load_golden\n"
            "from trajectory_optimization_amd import ops\n"
            "for name in ('hpr_synth_10k', 'hpr_synth_outside'):\n"
            "    d = load_golden(name)\n"
            "    idx, _ = ops.hidden_pts_removal(torch.from_numpy(d['points']).cuda())\n"
            "    assert np.array_equal(idx.cpu().numpy(), d['visible_idx']), name\n"
            "print('careful ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=dict(os.environ, TOHIP_HULL_CAREFUL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "careful ok" in r.stdout, r.stdout + r.stderr


def _shape_cloud(kind, n, rng):
    """tools/stress_hpr_large.py's shapes: what the sample phase's polytope looks like differs with each."""
    if kind == "ball":
        x = rng.normal(size=(n, 3)) * 7.0
    elif kind == "slab":
        x = rng.uniform(-1, 1, (n, 3)) * np.array([20, 20, 0.5]) + np.array([0, 0, 2.5])
    elif kind == "cluster":
        c = rng.uniform(-10, 10, (6, 3)); x = c[rng.integers(0, 6, n)] + rng.normal(size=(n, 3)) * 0.5
    elif kind == "ring":
        t = rng.uniform(0, 2 * np.pi, n); x = np.stack([np.cos(t) * 8, np.sin(t) * 8, rng.normal(size=n) * 0.2], 1) + rng.normal(size=(n, 3)) * 0.05
    elif kind == "far":
        x = rng.normal(size=(n, 3)) * 2 + np.array([300.0, -150.0, 40.0])
    elif kind == "grid":   # a lattice: thousands of exactly coplanar and collinear points on the hull of the flipped cloud's neighbours
        g = int(round(n ** (1 / 3)))
        x = np.stack(np.meshgrid(*(np.arange(g, dtype=np.float64),) * 3, indexing="ij"), -1).reshape(-1, 3) * 0.5 + np.array([1.0, -3.0, 2.0])
    else:   # terrain
        xy = rng.uniform(-20, 20, (n, 2)); x = np.concatenate([xy, (np.sin(xy[:, :1] * 0.4) * np.cos(xy[:, 1:] * 0.3) * 1.5 - 2.0) + 0.02 * rng.normal(size=(n, 1))], 1)
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", ["ball", "slab", "cluster", "ring", "far", "grid", "terrain"])
def test_sample_hull_by_sequential_insertion_on_many_shapes(dev, kind):
    """r06: for segments of >= 32 k points the sample's hull is built by k_sample_hull (a block per segment, sequential insertion out of
    LDS) instead of the first rounds.  Seven shapes of 40 k - 64 k points, each alone and all in one batch: the visible index sets
    equal Qhull's (the reference's call), whatever the schedule."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(2026)
    pts = _shape_cloud(kind, 64_000 if kind != "grid" else 40 ** 3, rng)
    ref = oracle.hidden_pts_removal(pts)[0]
    P = torch.from_numpy(pts).to(dev)
    for _ in range(2):
        got = ops.hidden_pts_removal(P)[0].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref), kind
    # the same cloud twice in a batch, next to a small segment that takes no part in the sample phase
    small = _shape_cloud("ball", 3_000, rng)
    allp = torch.from_numpy(np.concatenate([pts, small, pts])).to(dev)
    offs = np.cumsum([0, len(pts), len(small), len(pts)])
    idx, voff, _, status = ops.hidden_pts_removal_batched(allp, offs)
    idx = idx.cpu().numpy().astype(np.int64)
    assert status.cpu().tolist() == [0, 0, 0]
    assert np.array_equal(idx[voff[0]:voff[1]], ref) and np.array_equal(idx[voff[2]:voff[3]] - offs[2], ref)
    assert np.array_equal(idx[voff[1]:voff[2]] - offs[1], oracle.hidden_pts_removal(small)[0])


def test_a_build_that_runs_out_of_faces_is_retried_cleanly(dev):
    """A cloud most of whose points are visible needs more faces than the recommended workspace holds: the build returns TOHIP_ENOSPC
    and ops retries with 4x the bytes.  The host only learns of the overflow from its next readback — up to two batches of rounds are
    enqueued behind the failing one; they must not walk the half-built round (r06: a memory fault found by repeated builds,
    on exactly this path, when the workspace held another build's bytes).  Three builds into poisoned memory: no fault, Qhull's set."""
    from oracle import oracle
    from trajectory_optimization_amd import _lib, ops
    from trajectory_optimization_amd._lib import ptr, stream_ptr
    rng = np.random.default_rng(17)
    u = rng.normal(size=(120_000, 3))   # a noisy shell around the viewpoint: more than half of its points are visible
    pts = (u / np.linalg.norm(u, axis=1, keepdims=True) * 12.0 * (1 + 0.01 * rng.normal(size=(120_000, 1)))).astype(np.float32)
    ref = oracle.hidden_pts_removal(pts)[0]
    assert len(ref) > 50_000   # ~6 faces are created per vertex: more than the 262 144 the recommended workspace of a small cloud holds
    P = torch.from_numpy(pts).to(dev)
    L = _lib.lib()
    n = len(pts)
    wsb = L.tohip_hpr_workspace_bytes(n)
    idx, cnt, mask = torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
    for fill in (0xFF, 0x01, 0x7F):
        ws = torch.full((wsb,), fill, dtype=torch.uint8, device=dev)
        rc = L.tohip_hidden_pts_removal(ptr(P), n, 2.0, ptr(idx), ptr(cnt), ptr(mask), ptr(ws), wsb, stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.ENOSPC, rc          # the recommended size is too small for this cloud ...
        del ws
        poison = torch.full((4 * wsb,), fill, dtype=torch.uint8, device=dev)   # ... and the retry's 4x block comes back full of this
        del poison
        got = ops.hidden_pts_removal(P)[0].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref)


def test_sample_rounds_and_sequential_insertion_agree_in_a_child_process():
    """TOHIP_HULL_SERIAL=0 (the sample's rounds of r05) gives the same index sets as the default: the sample phase is a schedule, not a result."""
    import os, subprocess, sys
    from conftest import REPO
    code = ("import sys, numpy as np, torch; sys.path.insert(0, 'tests'); from conftest import load_golden\n"
            "from trajectory_optimization_amd import ops, synth\n"
            "pts = synth.make_cloud(200_000, seed=7)\n"
            "idx, _ = ops.hidden_pts_removal(torch.from_numpy(pts).cuda())\n"
            "np.save(sys.argv[1], idx.cpu().numpy())\n")
    import tempfile
    outs = []
    with tempfile.TemporaryDirectory() as d:
        for serial in ("0", "1"):
            f = os.path.join(d, f"idx{serial}.npy")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=REPO, env=dict(os.environ, TOHIP_HULL_SERIAL=serial), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            outs.append(np.load(f))
    assert np.array_equal(outs[0], outs[1]) and len(outs[0]) > 1000


def test_regions_that_share_edges_give_the_same_hull_in_fewer_rounds():
    """convex_across (r06): two regions that share a horizon edge are inserted in the same round when the new faces on it meet convexly.
    TOHIP_HULL_SHARE_EDGES=0 is the rule of r05 (adjacent regions exclude each other): the same vertex set — with and without the
    origin, on a cloud, a thin shell (every point a vertex) and a grid (coplanar faces everywhere) — in clearly more rounds."""
    import os, subprocess, sys, tempfile
    from conftest import REPO
    code = ("import sys, numpy as np, torch\n"
            "from trajectory_optimization_amd import ops, synth\n"
            "rng = np.random.default_rng(3)\n"
            "u = rng.normal(size=(60_000, 3)); shell = (u / np.linalg.norm(u, axis=1, keepdims=True) * 7.0).astype(np.float32)\n"
            "g = np.stack(np.meshgrid(*[np.arange(40, dtype=np.float32)] * 3, indexing='ij'), -1).reshape(-1, 3) - np.float32(19.5)\n"
            "out = {}\n"
            "for name, pts in (('cloud', synth.make_cloud(300_000, seed=9)), ('shell', shell), ('grid', g)):\n"
            "    P = torch.from_numpy(pts).cuda()\n"
            "    v, rounds = ops.hull_vertices_with_origin(P, with_origin=True, return_rounds=True)\n"
            "    out[name] = v.cpu().numpy(); out[name + '_rounds'] = np.int64(rounds)\n"
            "    out[name + '_hpr'] = ops.hidden_pts_removal(P)[0].cpu().numpy()\n"
            "np.savez(sys.argv[1], **out)\n")
    res = []
    with tempfile.TemporaryDirectory() as d:
        for share in ("1", "0"):
            f = os.path.join(d, f"hull{share}.npz")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=REPO, env=dict(os.environ, TOHIP_HULL_SHARE_EDGES=share), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            res.append(dict(np.load(f)))
    new, old = res
    for name in ("cloud", "shell", "grid"):
        assert np.array_equal(new[name], old[name]) and np.array_equal(new[name + "_hpr"], old[name + "_hpr"]), name
    assert len(new["shell"]) == 60_001 or len(new["shell"]) == 60_000   # every point of the shell is a vertex (the origin is inside)
    assert int(new["cloud_rounds"]) * 4 <= int(old["cloud_rounds"]) * 3, (int(new["cloud_rounds"]), int(old["cloud_rounds"]))


def test_hpr_batched_large_and_degenerate_segments_sample_phase(dev):
    """Segments large enough for the build's sample phase (first rounds on every k-th point, then all points join the sample's
    hull) next to tiny, flat and empty ones whose share of the sample may be a single point or none."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(5)
    flat = np.zeros((60, 3), np.float32)
    flat[:, 0] = np.arange(1, 61)
    flat[:, 1] = rng.uniform(-1, 1, 60)
    segs = [synth.make_cloud(220_000, seed=41) - np.float32([3.0, 1.0, 0.5]), np.zeros((0, 3), np.float32), synth.make_cloud(5, seed=42), flat,
            synth.make_cloud(150_000, seed=43) * np.float32(1.7), synth.make_cloud(3, seed=44), synth.make_cloud(900, seed=45)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    assert offs[-1] // len(segs) >= 32768   # the average segment size switches the sample phase on
    idx, voff, mask, status = ops.hidden_pts_removal_batched(torch.from_numpy(np.concatenate(segs)).to(dev), offs)
    idx, status = idx.cpu().numpy().astype(np.int64), status.cpu().numpy()
    assert status.tolist() == [0, 1, 0, 2, 0, 1, 0]
    for s, pts in enumerate(segs):
        got = idx[voff[s]:voff[s + 1]] - offs[s]
        if status[s] != 0:
            assert len(got) == 0
        else:
            ref, _ = oracle.hidden_pts_removal(pts)
            assert np.array_equal(got, ref), f"segment {s}"


def test_hull_with_exact_copies_of_points(dev):
    """Duplicated rows (a copy of a hull vertex lies ON the hull whatever the rounding of its plane distance says): as many
    vertices as Qhull finds, at the same coordinates, each reported at the LOWEST row that has its coordinates — with and without
    the sample phase of the build (the larger cloud goes through it)."""
    from scipy.spatial import ConvexHull
    from trajectory_optimization_amd import ops
    for n, seed in ((20_000, 61), (120_000, 62)):
        base = synth.make_cloud(n, seed=seed)
        ref0 = np.sort(ConvexHull(base.astype(np.float64)).vertices)
        rng = np.random.default_rng(seed)
        dup = np.concatenate([ref0[rng.integers(0, len(ref0), 300)], rng.integers(0, n, 300)])   # copies of vertices and of others
        pts = np.concatenate([base, base[dup], base[dup[:100]]]).astype(np.float32)
        got = ops.hull_vertices_with_origin(torch.from_numpy(pts).to(dev), False).cpu().numpy().astype(np.int64)
        ref = ConvexHull(pts.astype(np.float64)).vertices
        assert len(got) == len(ref) == len(ref0)
        assert np.array_equal(np.unique(pts[got], axis=0), np.unique(pts[ref], axis=0))
        assert np.array_equal(got, ref0)   # every vertex is reported at its first row (the copies were appended)
        assert np.array_equal(got, lowest_identical_rows(pts, ref))


@pytest.mark.parametrize("name", ["hpr_synth_dups_20k", "hpr_synth_dups_120k"])
def test_hpr_with_duplicate_rows_vs_reference(dev, name):
    """The reference's hidden_pts_removal (/root/reference/src/tools.py:67-85) on clouds with exact duplicate rows, copies before
    and after their originals (fixtures from the reference itself, 20 k and 120 k rows: without and with the sample phase of the
    GPU build).  Which of several identical rows Qhull reports follows its insertion history (the first copy in ~70 % of the
    cases, the last in the others) and no parallel build can reproduce it; what is pinned: the SAME visible points — count and
    coordinates — each reported at the lowest row with its coordinates, i.e. Qhull's set mapped through that rule, exactly."""
    from trajectory_optimization_amd.tools import hidden_pts_removal, convexHull, sphericalFlip
    d = load_golden(name)
    assert bool(d["origin_is_vertex"])   # (else the reference's drop-last quirk would pick between copies)
    pts = torch.from_numpy(d["points"]).to(dev)
    for _ in range(3):   # claims land in a different order from build to build; the result must not move
        vis, mask = hidden_pts_removal(pts, dev)
        got = np.flatnonzero(mask.cpu().numpy())
        ref = d["visible_idx"]
        assert len(got) == len(ref)
        assert np.array_equal(np.unique(d["points"][got], axis=0), np.unique(d["points"][ref], axis=0))
        assert np.array_equal(got, lowest_identical_rows(d["points"], ref))
        hull = convexHull(sphericalFlip(pts, dev, 2), dev).vertices.cpu().numpy()
        assert np.array_equal(hull[:-1], got) and hull[-1] == len(d["points"])
    assert int((got != ref).sum()) > 0   # the fixture does exercise the difference between the two rules
    # the guard for callers that need Qhull's own row indices: it fires on this cloud and stays silent on one without duplicates
    with pytest.raises(ValueError, match="duplicate rows"):
        hidden_pts_removal(pts, dev, duplicate_rows="error")
    clean = torch.from_numpy(load_golden("hpr_synth_100k")["points"]).to(dev)
    vis_c, mask_c = hidden_pts_removal(clean, dev, duplicate_rows="error")
    assert np.array_equal(np.flatnonzero(mask_c.cpu().numpy()), load_golden("hpr_synth_100k")["visible_idx"])
    with pytest.raises(ValueError):
        hidden_pts_removal(clean, dev, duplicate_rows="first")


def test_hull_builds_repeat(dev):
    """The order in which concurrent claims land differs from build to build (and with it face ids and the number of rounds); the
    vertex set must not: twelve builds of two fixtures, every one equal to Qhull's."""
    from trajectory_optimization_amd.tools import convexHull, sphericalFlip
    for name in ("hpr_synth_outside", "hpr_synth_100k"):
        d = load_golden(name)
        pts = torch.from_numpy(d["points"]).to(dev)
        for _ in range(12):
            if "hull_vertices" in d:
                assert np.array_equal(convexHull(sphericalFlip(pts, dev, 2), dev).vertices.cpu().numpy(), d["hull_vertices"])
            else:
                from trajectory_optimization_amd.tools import hidden_pts_removal
                _, mask = hidden_pts_removal(pts, dev)
                assert np.array_equal(np.flatnonzero(mask.cpu().numpy()), d["visible_idx"])
