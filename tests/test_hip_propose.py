"""View proposals on the GPU (tools.propose_views, propose_kernels.hip): the bearing histograms against the numpy restatement of the
pair test (synth.propose_hist_ref) with torch.equal — at one point, one tile plus one point and a position count that fills no block,
for 8, 32 and 128 sectors, with and without weights; points exactly on sector boundaries and on, one ulp inside and one ulp outside
each gate; excluded rows; independence of the packed order, of the prune and of the run; exact translation invariance; the headings
against synth.propose_headings_ref; the public call on a scene whose answer is known; and the example."""
import os

import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
TAN_V = float((IH / 2) / K[1, 1])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev, dt=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def hist_both(dev, pts, pos, open_=None, weights=None, S=32, mn=1.0, mx=10.0, tv=TAN_V, sort=True, cloud=None):
    """The device's histogram against the restatement, bit for bit -> (device hist on the host, the packed cloud)."""
    from trajectory_optimization_amd import ops
    cloud = ops.PackedCloud(_t(pts, dev, f32), sort=sort) if cloud is None else cloud
    got = ops.view_histogram(cloud, _t(pos, dev, f32), _t(open_, dev, np.uint8), _t(weights, dev, np.int32), S, mn, mx, tv).cpu()
    want = synth.propose_hist_ref(pts, pos, np.ones(len(pos)) if open_ is None else open_, weights, S, mn, mx, tv)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(pos), S)
    assert torch.equal(got, torch.from_numpy(want)), f"{int((got != torch.from_numpy(want)).sum())} of {got.numel()} bins differ"
    return got, cloud


_CLOUDS = {}


def sized_case(N, M):
    """A make_cloud of N points and M positions inside its slab (for the clouds too thin to be seen from anywhere: around the first
    point), random weights in [0, 32768] that include both ends; made once."""
    if (N, M) not in _CLOUDS:
        rng = np.random.default_rng(1000 * M + N % 997)
        pts = synth.make_cloud(N, seed=N % 89)
        if N < 1000:
            pos = pts[0].astype(np.float64) + np.concatenate([rng.uniform(-5, 5, (M, 2)), rng.uniform(-1, 1, (M, 1))], axis=1)
            pos[0] = pts[0].astype(np.float64) + [3.0, 1.0, 0.25]   # the first point is inside this one's shell and field of view
        else:
            pos = rng.uniform([-20, -20, -2], [20, 20, 2], (M, 3))
        w = rng.integers(0, 32769, N)
        w[rng.random(N) < 0.1] = 0
        w[rng.random(N) < 0.1] = 32768
        w[0] = 32768
        _CLOUDS[(N, M)] = (pts, pos.astype(f32), w.astype(np.int32), {})
    return _CLOUDS[(N, M)]


@pytest.mark.parametrize("S", [8, 32, 128])
@pytest.mark.parametrize("N,M", [(1, 1), (1, 37), (257, 1), (257, 37), (20_000, 1), (20_000, 37), (100_000, 300)])
def test_histogram_sizes(dev, N, M, S):
    pts, pos, w, keep = sized_case(N, M)
    got, keep["cloud"] = hist_both(dev, pts, pos, S=S, cloud=keep.get("cloud"))
    assert int(got.sum()) > 0 and int(got[0].sum()) > 0
    gw, _ = hist_both(dev, pts, pos, weights=w, S=S, cloud=keep["cloud"])
    assert int(gw.sum()) > int(got.sum())   # (the mean weight is far above 1; the thin clouds' point 0 weighs 32 768)


def test_boundaries_and_gates_by_hand(dev):
    """min = 2, max = 5, tan_v = 1/2 from the origin with S = 8: every expectation below follows from the definition."""
    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(0))
    rows = [((2, 0, 0), 0), ((2, 2, 0), 1), ((0, 2, 0), 2), ((-2, 2, 0), 3), ((-2, 0, 0), 4), ((-2, -2, 0), 5), ((0, -2, 0), 6),
            ((2, -2, 0), 7),                                   # on the 0, 45, ... 315 degree boundaries: the upper sector
            ((0, 0, 3), None),                                 # the dx = dy = 0 column
            ((dn(2), 0, 0), None), ((up(2), 0, 0), 0),         # one ulp inside / outside min_dist (exactly on it: the first row)
            ((5, 0, 0), 0), ((3, 4, 0), 1), ((up(5), 0, 0), None), ((dn(5), 0, 0), 0),   # exactly max_dist, and one ulp either side
            ((2, 0, 1), 0), ((2, 0, -1), 0), ((2, 0, up(1)), None), ((0, -4, dn(2)), 6), ((0, -4, up(2)), None)]   # the elevation gate
    pts = np.array([r[0] for r in rows], dtype=f32)
    want = np.bincount([r[1] for r in rows if r[1] is not None], minlength=8)
    got, _ = hist_both(dev, pts, np.zeros((1, 3), f32), S=8, mn=2.0, mx=5.0, tv=0.5)
    assert got[0].tolist() == want.tolist() == [6, 2, 1, 1, 1, 1, 2, 1]


def test_boundaries_on_a_lattice(dev):
    g = np.arange(-6, 7)
    lat = np.stack(np.meshgrid(g, g, np.arange(-2, 3), indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    pos = np.array([[0, 0, 0], [1, 2, 0], [-6, 6, 1], [0.5, 0.5, 0.0]], dtype=f32)   # three lattice points and a cell centre
    for S in (8, 32):
        got, _ = hist_both(dev, lat, pos, S=S, mn=2.0, mx=5.0, tv=0.5)
        assert int(got[0].sum()) > 100
    # from a lattice point the lattice is symmetric under a quarter turn, and a boundary point belongs to the upper sector in every
    # quadrant alike: the histogram of 8 sectors repeats with period 2
    got, _ = hist_both(dev, lat, pos[:1], S=8, mn=2.0, mx=5.0, tv=0.5)
    assert got[0].view(4, 2).eq(got[0, :2]).all()


def test_excluded_rows_and_positions(dev):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(5000, seed=4)
    pts[7] = [np.nan, 0, 0]
    pts[300] = [0, np.inf, 0]
    pts[4999] = [1, 1, -np.inf]
    pos = np.array([[0, 0, 0], [np.nan, 0, 0], [1, np.inf, 0], [2, 2, 0], [0, 0, 0]], dtype=f32)
    open_ = np.array([1, 1, 1, 0, 1], dtype=np.uint8)
    got, cloud = hist_both(dev, pts, pos, open_)
    assert int(got[0].sum()) > 0 and torch.equal(got[0], got[4]) and not got[1:4].any()
    clean = np.delete(pts, [7, 300, 4999], axis=0)
    assert torch.equal(hist_both(dev, clean, pos, open_)[0], got)   # the rows that are not finite never count
    heading, score = ops.view_headings(got.to(dev), 3, 2)
    assert heading[1:4].eq(-1).all() and score[1:4].eq(0).all() and heading[0, 0] >= 0


def test_prune_and_order_independence(dev):
    from trajectory_optimization_amd import ops
    pts, pos, w, _ = sized_case(20_000, 37)
    a, cloud = hist_both(dev, pts, pos, weights=w, sort=True)
    b, flat = hist_both(dev, pts, pos, weights=w, sort=False)
    assert torch.equal(a, b)
    args = (_t(pos, dev), None, _t(w, dev), 32, 1.0, 10.0, TAN_V)
    assert torch.equal(ops.view_histogram(cloud, *args).cpu(), a)                   # the same call twice: the same bits
    assert torch.equal(ops.view_histogram(cloud, *args, prune=False).cpu(), a)      # the prune changes no bit
    assert torch.equal(ops.view_histogram(flat, *args, prune=False).cpu(), a)


def test_translation_invariance(dev):
    """A cloud and positions on a 2^-8 m grid moved by (8192, -8192, 4096): every x - t keeps its bits, so must the histogram."""
    snap = lambda a: (np.round(np.asarray(a, dtype=np.float64) * 256) / 256)
    pts, pos, w, _ = sized_case(20_000, 37)
    pts, pos = snap(pts), snap(pos)
    T = np.array([8192.0, -8192.0, 4096.0])
    assert ((pts + T).astype(f32).astype(np.float64) == pts + T).all() and ((pos + T).astype(f32).astype(np.float64) == pos + T).all()
    here, _ = hist_both(dev, pts.astype(f32), pos.astype(f32), weights=w)
    there, _ = hist_both(dev, (pts + T).astype(f32), (pos + T).astype(f32), weights=w)
    assert torch.equal(here, there) and int(here.sum()) > 0


def headings_both(dev, hist, hw, n_per, sep=None, min_score=0):
    from trajectory_optimization_amd import ops
    hist = np.asarray(hist, dtype=np.int64)
    wh, ws = synth.propose_headings_ref(hist, hw, n_per, sep, min_score)
    gh, gs = ops.view_headings(_t(hist, dev), hw, n_per, sep, min_score)
    assert gh.dtype == torch.int32 and gs.dtype == torch.int64
    assert torch.equal(gh.cpu(), torch.from_numpy(wh)) and torch.equal(gs.cpu(), torch.from_numpy(ws))
    return wh, ws


def test_headings_against_the_restatement(dev):
    rng = np.random.default_rng(5)
    for S in (8, 16, 32, 64, 128):
        for M in (1, 5, 130):
            hist = rng.integers(0, 1 << 40, (M, S))   # window sums far above 2^32
            hist[rng.random((M, S)) < 0.3] = 0
            for hw in sorted({0, 1, S // 8, (S - 1) // 2}):
                for n_per in (1, 3, 8):
                    headings_both(dev, hist, hw, n_per)
            headings_both(dev, hist, 1, 4, sep=0)
            headings_both(dev, hist, 1, 4, sep=S)
            headings_both(dev, rng.integers(0, 4, (M, S)), 1, 8)   # many ties
    # an all-equal row: ties go to the lowest heading, and the next ones follow at the separation
    h, s = headings_both(dev, np.full((1, 32), 5), 3, 8)
    assert h[0].tolist() == [0, 7, 14, 21, -1, -1, -1, -1] and s[0].tolist() == [35] * 4 + [0] * 4   # 28 is within 6 of 0 round the circle
    # a peak at sector 0 and at S - 1: the window wraps
    for S in (8, 128):
        for at in (0, S - 1):
            row = np.zeros((1, S), dtype=np.int64)
            row[0, at] = 9
            h, s = headings_both(dev, row, 1, 2)
            assert h[0].tolist() == [min((at - 1) % S, at, (at + 1) % S), -1] and s[0].tolist() == [9, 0]
    # hw = 0 and the window that is the whole circle
    row = np.array([[3, 1, 4, 1, 5, 9, 2, 6]])
    h, s = headings_both(dev, row, 0, 3)
    assert h[0].tolist() == [5, 7, 4] and s[0].tolist() == [9, 6, 5]
    row16 = np.arange(16)[None]
    h, s = headings_both(dev, np.concatenate([row16, row16[:, ::-1]]), 7, 2)   # 2 hw + 1 = 15 of 16: the window leaves one sector out
    assert s[:, 0].tolist() == [120, 120] and h[:, 0].tolist() == [8, 7] and h[:, 1].tolist() == [-1, -1]
    # n_per beyond what the suppression leaves; min_score between two scores; sums above 2^32
    h, s = headings_both(dev, np.array([[7, 0, 0, 0, 3, 0, 0, 0]]), 0, 8, sep=1)
    assert h[0].tolist() == [0, 4] + [-1] * 6
    h, s = headings_both(dev, np.array([[7, 0, 0, 0, 3, 0, 0, 0]]), 0, 3, sep=1, min_score=5)
    assert h[0].tolist() == [0, -1, -1] and s[0].tolist() == [7, 0, 0]
    big = np.zeros((1, 32), dtype=np.int64)
    big[0, 10:13] = (1 << 45) + 1
    h, s = headings_both(dev, big, 1, 1)
    assert h[0, 0] == 11 and s[0, 0] == 3 * ((1 << 45) + 1)
    assert headings_both(dev, np.zeros((3, 32)), 3, 2)[0].tolist() == [[-1, -1]] * 3   # nothing to see: no proposal (score >= 1)


# ---- the public call -----------------------------------------------------------------------------------------------------------------
S_PUB, BIG_AT, SMALL_AT = 32, 3, 19


def arc(sector, half_deg, n_bearings, r=3.0):
    """A wall patch: points at range r on the bearings centre(sector) +- half_deg, five heights."""
    mid = (sector + 0.5) * 360.0 / S_PUB
    b = np.deg2rad(np.linspace(mid - half_deg, mid + half_deg, n_bearings))
    z = np.array([-0.5, -0.25, 0.0, 0.25, 0.5])
    return np.stack([np.repeat(r * np.cos(b), 5), np.repeat(r * np.sin(b), 5), np.tile(z, n_bearings)], axis=1)


def scene():
    big, small = arc(BIG_AT, 37.0, 60), arc(SMALL_AT, 37.0, 20)   # each spans its heading's seven sectors and no other's fully
    pts = np.concatenate([big, small]).astype(f32)
    pos = np.array([[0, 0, 0], [0.5, -0.25, 0.1], pts[17] + f32([0.05, 0.0, 0.02]), [-1, 0.5, 0]], dtype=f32)   # row 2 hugs a point
    return pts, pos, len(big)


def test_propose_views_on_a_known_scene(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj
    from trajectory_optimization_amd.tools import propose_views, select_views, trajectory_clearance
    pts, pos, n_big = scene()
    P, Q = torch.from_numpy(pts).to(dev), torch.from_numpy(pos).to(dev)
    cam = dict(K=torch.from_numpy(K), img_width=IW, img_height=IH)
    qtable = torch.from_numpy(synth.propose_tables(S_PUB)[1])
    prop = propose_views(P, Q[:1], sectors=S_PUB, **cam)
    assert prop.hw == 3 and prop.weights is None and prop.open.tolist() == [True]
    assert prop.heading.tolist() == [BIG_AT, SMALL_AT] and prop.score.tolist() == [n_big, len(pts) - n_big]
    assert prop.position_index.tolist() == [0, 0] and torch.equal(prop.quats.cpu(), qtable[[BIG_AT, SMALL_AT]])
    assert torch.equal(prop.poses.cpu(), torch.from_numpy(pos[[0, 0]]))
    want = synth.propose_hist_ref(pts, pos[:1], [1], None, S_PUB, 1.0, 5.0, prop.tan_v)
    assert torch.equal(prop.hist.cpu(), torch.from_numpy(want)) and prop.tan_v == float(f32(TAN_V))
    # the large patch is covered already: the top heading moves to the small one
    prior = torch.zeros(len(pts), device=dev)
    prior[:n_big] = 20.0
    seen = propose_views(P, Q[:1], sectors=S_PUB, prior_log_odds=prior, **cam)
    assert seen.weights.dtype == torch.int32 and seen.weights[:n_big].eq(0).all() and seen.weights[n_big:].eq(16384).all()
    assert seen.heading.tolist() == [SMALL_AT] and seen.score.tolist() == [16384 * (len(pts) - n_big)]
    want = synth.propose_hist_ref(pts, pos[:1], [1], seen.weights.cpu().numpy(), S_PUB, 1.0, 5.0, seen.tan_v)
    assert torch.equal(seen.hist.cpu(), torch.from_numpy(want))
    # a position within the radius of a point is closed: trajectory_clearance's verdict
    r = 0.3
    near = propose_views(P, Q, sectors=S_PUB, clearance_radius=r, **cam)
    d, _ = trajectory_clearance(P, Q, r)
    assert torch.equal(near.open, d >= r) and near.open.tolist() == [True, True, False, True]
    assert not near.hist[2].any() and 2 not in near.position_index.tolist()
    assert propose_views(P, Q, sectors=S_PUB, **cam).open.all()
    # the ranking is the stated key, and max_views cuts it
    heading, score = ops.view_headings(near.hist, near.hw, 2)
    rows = sorted((-int(score[p, j]), p, int(heading[p, j])) for p in range(len(pos)) for j in range(2) if int(heading[p, j]) >= 0)
    assert [(-int(s), int(p), int(h)) for s, p, h in zip(near.score, near.position_index, near.heading)] == rows and len(rows) == 6
    cut = propose_views(P, Q, sectors=S_PUB, clearance_radius=r, max_views=4, **cam)
    assert cut.n_views == 4
    for name in ("poses", "quats", "score", "position_index", "heading"):
        assert torch.equal(getattr(cut, name), getattr(near, name)[:4]), name
    assert torch.equal(near.poses, Q[near.position_index]) and torch.equal(near.quats.cpu(), qtable[near.heading.long().cpu()])
    # the proposals feed select_views as they are
    sel = select_views(P, near.poses, near.quats, 1, intrins=torch.from_numpy(K), img_width=IW, img_height=IH)
    assert sel.n_selected == 1 and float(sel.gains[0]) > 0.0
    # a model brings its own cloud, camera, distances and prior
    poses, quats = synth.make_path(4)
    model = ModelTraj(P, torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, min_dist=1.5, max_dist=4.0,
                      device=dev, prior_log_odds=prior)
    a = propose_views(model, Q, n_per_position=3, sectors=16, clearance_radius=r, min_score=2)
    b = propose_views(P, Q, n_per_position=3, sectors=16, clearance_radius=r, min_score=2, prior_log_odds=prior, min_dist=1.5, max_dist=4.0,
                      **cam)
    assert a.n_views > 0 and (a.min_dist, a.max_dist, a.hw) == (1.5, 4.0, b.hw)
    for name in ("poses", "quats", "score", "position_index", "heading", "hist", "open", "weights"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_example_runs(dev):
    import importlib.util
    spec = importlib.util.spec_from_file_location("view_proposal_sample", os.path.join(REPO, "examples", "view_proposal_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main([])
    assert np.isfinite(out["proposals"]) and np.isfinite(out["grid"]) and out["n_proposals"] > 0
