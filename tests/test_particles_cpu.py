"""The particle filter's numpy restatement (synth.mcl_*_ref, philox4x32_ref) against known answers, its own invariants and the
tracking scene of tests/particle_cases.py; ops.check_particles' refusals.  No GPU."""
import numpy as np
import pytest

import particle_cases as pc
from trajectory_optimization_amd import synth


@pytest.mark.parametrize("counter, key, words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    assert " ".join(f"{int(v):08x}" for v in synth.philox4x32_ref(counter, key)) == words


def test_philox_broadcasts_over_the_particle_index():
    many = synth.philox4x32_ref((np.arange(5), 0, 7, 1), (3, 4))
    assert many.shape == (5, 4) and many.dtype == np.uint32
    for i in range(5):
        assert np.array_equal(many[i], synth.philox4x32_ref((i, 0, 7, 1), (3, 4)))


def test_tables_end_points_and_symmetry():
    trig, gauss, exp2 = synth.mcl_tables_ref()
    assert trig.shape == (16384, 2) and trig.dtype == np.int32
    assert trig[0].tolist() == [32768, 0] and trig[4096].tolist() == [0, 32768] and trig[8192].tolist() == [-32768, 0] and trig[12288].tolist() == [0, -32768]
    assert np.array_equal(trig[:, 0], trig[(-np.arange(16384)) % 16384, 0]) and np.array_equal(trig[:, 1], -trig[(-np.arange(16384)) % 16384, 1])
    assert np.array_equal(trig[:, 1], trig[(np.arange(16384) - 4096) % 16384, 0])          # sin(a) = cos(a - 90 degrees)
    assert np.abs(trig.astype(np.int64)[:, 0] ** 2 + trig.astype(np.int64)[:, 1] ** 2 - 32768 ** 2).max() <= 2 * 32768   # |c, s| within a unit
    assert gauss.shape == (1025,) and gauss[512] == 0 and np.array_equal(gauss, -gauss[::-1]) and (np.diff(gauss) > 0).all()
    assert gauss[1024] == 13506 and gauss[0] == -13506                                      # 4096 x 3.2974: the tails end near 3.3 sigma
    assert exp2.shape == (256,) and exp2[0] == 1 << 20 and exp2[128] == round(2 ** 19.5) and exp2[255] == round(2 ** (20 - 255 / 256)) and (np.diff(exp2) < 0).all()
    words = synth.mcl_table_words_ref()
    assert words.shape == (synth.MCL_TABLE_WORDS,) and np.array_equal(words[:32768].reshape(16384, 2), trig)
    assert np.array_equal(words[32768:32768 + 1025], gauss) and np.array_equal(words[33796:], exp2) and not words[32768 + 1025:33796].any()


def test_the_host_layers_tables_are_the_restatements():
    from trajectory_optimization_amd import ops
    assert np.array_equal(ops.particle_tables(), synth.mcl_table_words_ref())


def test_noise_is_a_cut_standard_normal():
    u = synth.philox4x32_ref((np.arange(1 << 16), 0, 0, 0), (11, 0)).astype(np.int64).reshape(-1)
    g = synth.mcl_gauss_ref(u) / 4096.0
    assert abs(g.mean()) < 0.01 and 0.985 < g.std() < 1.0 and 3.2 < g.max() < 3.3 and -3.3 < g.min() < -3.2
    assert np.array_equal(synth.mcl_noise_ref(u, 0), np.zeros_like(u))
    assert np.array_equal(synth.mcl_noise_ref(u, 256 * 4096), synth.mcl_gauss_ref(u))      # sigma = 4096 state units: the table itself
    assert synth.mcl_noise_ref(np.array([0, 0xFFFFFFFF]), 1 << 24).tolist() == [-13506 * 16, (13505 * 1 + 13506 * 65535) // 65536 * 16]


@pytest.mark.parametrize("n", [1, 7, 1024])
def test_equal_weights_keep_every_particle(n):
    w = np.full(n, 1 << 20, dtype=np.int64)
    for r in (0, 1, (n << 20) // 2, (n << 20) - 1):
        assert np.array_equal(synth.mcl_ancestors_ref(w, r), np.arange(n)), r


@pytest.mark.parametrize("pattern", ["random", "zeros_first", "peaked"])
@pytest.mark.parametrize("n", [5, 257, 4096])
def test_ancestors_never_decrease_and_offspring_are_proportional(n, pattern):
    lw = pc.synthetic_log_weights(n, pattern)
    w = synth.mcl_weight_ref(np.maximum(lw - lw.max(), synth.MCL_FLOOR))
    s1 = int(w.sum())
    for r in (0, s1 // 3, s1 - 1):
        a = synth.mcl_ancestors_ref(w, r)
        assert (np.diff(a) >= 0).all() and a.min() >= 0 and a.max() < n
        assert (w[a] > 0).all()
        assert (np.abs(np.bincount(a, minlength=n) - n * w / s1) < 1.0).all()


def test_one_survivor_fathers_everyone():
    n = 300
    lw, w, rec = synth.mcl_weights_ref(np.zeros((n, 4), dtype=np.int32), pc.synthetic_log_weights(n, "one"), None, threshold=0.5 * n)
    assert (w > 0).sum() == 1 and w[200] == 1 << 20 and rec[7] == 200 and rec[0] == 1 << 20 and rec[11] == 1 and lw[200] == 0 and rec[13] == 77
    for r in (0, (1 << 20) - 1):
        assert (synth.mcl_ancestors_ref(w, r) == 200).all()
    state, lw2, a, verdict = synth.mcl_resample_ref(np.arange(4 * n).reshape(n, 4), lw, w, 0.5 * n)
    assert verdict == 1 and (a == 200).all() and (state == np.arange(800, 804)).all() and not lw2.any()


def test_weights_floor_sums_and_verdict():
    n = 64
    state = pc.random_state(n, (8, 8, 4), 0)
    lw0 = pc.synthetic_log_weights(n, "zeros_first")
    lw, w, rec = synth.mcl_weights_ref(state, lw0, None, threshold=0.5 * n)
    assert lw.max() == 0 and lw.min() == synth.MCL_FLOOR and w.max() == 1 << 20 and w[0] == 0
    trig = synth.mcl_tables_ref()[0].astype(object)[state[:, 3]]
    wo, so = w.astype(object), state.astype(object)
    assert rec[:7].tolist() == [wo.sum(), (wo * wo).sum(), (wo * so[:, 0]).sum(), (wo * so[:, 1]).sum(), (wo * so[:, 2]).sum(),
                                (wo * trig[:, 0]).sum(), (wo * trig[:, 1]).sum()]
    n_eff = float(rec[0]) ** 2 / float(rec[1])
    assert np.float64(n_eff).view(np.int64) == rec[12] and rec[14] == n
    for threshold, verdict in ((n_eff, 0), (np.nextafter(n_eff, np.inf), 1), (0.0, 0)):
        assert synth.mcl_weights_ref(state, lw0, None, threshold=threshold)[2][11] == verdict
        assert synth.mcl_resample_ref(state, lw, w, threshold)[3] == verdict
    same = synth.mcl_resample_ref(state, lw, w, 0.0)
    assert np.array_equal(same[0], state) and np.array_equal(same[1], lw) and np.array_equal(same[2], np.arange(n))
    # a weight halves per 65536 units and is 0 beyond 20 halvings
    assert synth.mcl_weight_ref([0, -65536, -65536 * 20, -65536 * 21, -256, -255]).tolist() == [1 << 20, 1 << 19, 1, 0, synth.mcl_tables_ref()[2][1], 1 << 20]


def test_predict_and_seed_restatements_wrap_and_clamp():
    n = 33
    state = pc.random_state(n, (8, 8, 4), 1)
    out = synth.mcl_predict_ref(state, [300, -200, 50, 16000], [100 * 256, 100 * 256, 0, 256 * 256], seed=5, step=2)
    assert out.dtype == np.int32 and (np.abs(out[:, :3]) <= synth.MCL_CLAMP).all() and (out[:, 3] >= 0).all() and (out[:, 3] < 16384).all()
    assert out[1, 0] == synth.MCL_CLAMP or out[1, 1] == -synth.MCL_CLAMP       # the row at the clamp stays inside it
    assert np.array_equal(out[:, 2] - state[:, 2], np.where(np.abs(state[:, 2] + 50) > synth.MCL_CLAMP, out[:, 2] - state[:, 2], 50))
    still = synth.mcl_predict_ref(state, [0, 0, 0, 0], [0, 0, 0, 0], seed=5, step=2)
    assert np.array_equal(still, state)
    ahead = synth.mcl_predict_ref(np.array([[0, 0, 0, 4096]], dtype=np.int32), [256, 0, 0, 0], [0, 0, 0, 0])   # heading +y: forward is +y
    assert ahead.tolist() == [[0, 256, 0, 4096]]
    left = synth.mcl_predict_ref(np.array([[0, 0, 0, 0]], dtype=np.int32), [0, 256, 0, -1], [0, 0, 0, 0])      # left of +x is +y; -1 wraps
    assert left.tolist() == [[0, 256, 0, 16383]]
    a, b = synth.mcl_seed_gaussian_ref(n, [1, 2, 3, 16380], [512, 512, 256, 2560], seed=9), synth.mcl_seed_gaussian_ref(n, [1, 2, 3, 16380], [512, 512, 256, 2560], seed=10)
    assert not np.array_equal(a, b) and (a[:, 3] < 16384).all() and (a[:, 3] >= 0).all() and ((a[:, 3] < 100) | (a[:, 3] > 16000)).all()
    g = synth.mcl_seed_positions_ref(200, [[0.05, 0.05, 0.05], [0.35, 0.15, 0.25]], (0, 0, 0), 0.1, True, seed=2)
    v = g[:, :3] >> 8
    assert set(map(tuple, v.tolist())) == {(0, 0, 0), (3, 1, 2)} and len(np.unique(g[:, 3])) > 100
    c = synth.mcl_seed_positions_ref(200, [[0.35, 0.15, 0.25]], (0, 0, 0), 0.1, False, seed=2)
    assert (c[:, :3] == [3 * 256 + 128, 256 + 128, 2 * 256 + 128]).all()


def test_poses_restatement_is_scan_matchings_pose():
    state = np.array([[256 * 3 + 128, 256 * 2, -256, 0], [0, 0, 0, 4096]], dtype=np.int32)
    T = synth.mcl_poses_ref(state, (1.0, 2.0, 3.0), 0.5)
    assert T.dtype == np.float32 and T.shape == (2, 12)
    assert T[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0 + 0.5 * 3.5, 3.0, 2.5]
    assert T[1].tolist() == [0, -1, 0, 1, 0, 0, 0, 0, 1, 1.0, 2.0, 3.0]
    # the weigh restatement against scan matching's own, particle by particle, with an attitude
    import scan_match_cases as sc
    dims = (9, 7, 5)
    L, pts, A = sc.random_log_odds(dims, 3), sc.random_scan(dims, 90, 3), pc.attitude()
    st = pc.random_state(12, dims, 2)
    score, used, known = synth.mcl_weigh_ref(L, sc.ORIGIN, sc.RES, pts, st, A, floor=-20, unknown_value=-3, chunk=5)
    P = synth.mcl_poses_ref(st, sc.ORIGIN, sc.RES, A)
    for i in range(12):
        want = synth.scan_score_ref(L, sc.ORIGIN, sc.RES, pts, P[i, :9].reshape(3, 3), P[i, 9:], (0, 0, 0), -20, -3)
        assert (score[i], used[i], known[i]) == (want[0], want[1], want[3]), i
    assert len(np.unique(score)) > 6 and used.max() > 0


def test_check_particles_names_every_refusal():
    import torch

    from trajectory_optimization_amd import ops

    class M(ops.EvidenceMap):   # a map's geometry without a device
        def __init__(self):
            self.origin, self.resolution, self.dims, _ = ops.check_los((0, 0, 0), 0.1, (8, 8, 4))
            self.device = torch.device("cuda:0")

    class Matcher(ops.ScanMatcher):
        def __init__(self, m):
            self.map, self.floor, self.unknown_value = m, -20, -3

    m = M()
    c = ops.check_particles(m, 1024, 5, 300, -10, -3, sigma=(0.1, 0.1, 0.05, np.pi / 180), delta=(0.25, 0.0, 0.0, -np.pi / 2), ratio=0.5,
                            attitude=np.eye(3))
    assert (c["map"], c["floor"], c["unknown_value"], c["n"], c["seed"], c["beta_q"], c["ratio"]) == (m, -10, -3, 1024, 5, 300, 0.5)
    assert c["sigma_q8"] == [65536, 65536, 32768, round(256 * 16384 / 360)] and c["delta"] == [640, 0, 0, -4096]
    assert c["attitude"].dtype == np.float32 and c["attitude"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert ops.check_particles(m, sigma=(1, 2, 3, 4), delta=(5, 6, 7, 8.4), units="state")["delta"] == [5, 6, 7, 8]
    got = ops.check_particles(Matcher(m), np.int64(1 << 20), (1 << 64) - 1, 65536)
    assert (got["map"], got["floor"], got["unknown_value"], got["n"]) == (m, -20, -3, 1 << 20)
    for bad in (None, "map", torch.zeros(3)):
        with pytest.raises(ValueError, match="the map must be an ops.EvidenceMap or an ops.ScanMatcher"):
            ops.check_particles(bad)
    for kw in (dict(floor=-1), dict(unknown_value=-1)):
        with pytest.raises(ValueError, match="belong to the ScanMatcher"):
            ops.check_particles(Matcher(m), **kw)
    with pytest.raises(ValueError, match="floor must be"):
        ops.check_particles(m, floor=1)
    with pytest.raises(ValueError, match="unknown_value must be"):
        ops.check_particles(m, unknown_value=-128)
    for bad in (0, (1 << 20) + 1, 1.5, True, None):
        with pytest.raises(ValueError, match="n must be an integer in"):
            ops.check_particles(m, bad)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed must be an integer in"):
            ops.check_particles(m, 1, bad)
    for bad in (0, 65537, 1.0):
        with pytest.raises(ValueError, match="beta_q must be an integer in"):
            ops.check_particles(m, 1, 0, bad)
    with pytest.raises(ValueError, match="units must be"):
        ops.check_particles(m, units="feet")
    for bad in ((1, 1, 1), "abc", (1, 1, 1, np.nan)):
        with pytest.raises(ValueError, match="sigma must be"):
            ops.check_particles(m, sigma=bad)
    for bad in ((-0.1, 0, 0, 0), (30.0, 0, 0, 0)):   # 30 m at 0.1 m voxels: 76 800 state units
        with pytest.raises(ValueError, match="sigma must be four numbers >= 0"):
            ops.check_particles(m, sigma=bad)
    with pytest.raises(ValueError, match="delta must be"):
        ops.check_particles(m, delta=(1, 2))
    with pytest.raises(ValueError, match="delta must be four numbers"):
        ops.check_particles(m, delta=(1 << 24, 0, 0, 0), units="state")
    for bad in (-0.1, 1.1, "x", np.nan):
        with pytest.raises(ValueError, match="ratio must be a number in"):
            ops.check_particles(m, ratio=bad)
    for bad in (np.eye(4), [1, 2, 3], np.full((3, 3), np.inf), "A"):
        with pytest.raises(ValueError, match="attitude must be nine finite numbers"):
            ops.check_particles(m, attitude=bad)


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_tracking_on_the_scan_matching_scene(seed):
    """From the third update on, the restatement's weighted mean lies within 0.5 voxel per axis and 1.5 degrees of the truth.
    Measured with this restatement, seeds 1, 2, 3, updates 3 .. 5: at worst 0.154 voxel and 0.58 degrees."""
    out = pc.tracking_ref(seed)
    assert len(out) == pc.UPDATES and all(len(s) == 768 for s in pc.scene()["scans"])
    for k, o in enumerate(out, 1):
        dv, dy = pc.errors(o["record"], k)
        print(f"seed {seed} update {k}: error {dv.round(3).tolist()} voxel, {dy:.3f} degrees, n_eff {synth.mcl_n_eff(o['record'][0], o['record'][1]):.1f}, "
              f"verdict {o['record'][11]}, best score {o['record'][8]}")
        if k >= pc.BAR_FROM:
            assert (dv <= pc.BAR_VOXEL).all() and dy <= pc.BAR_DEG, (seed, k, dv, dy)
    assert any(o["record"][11] == 1 for o in out)          # the filter did resample
    assert out[-1]["record"][8] == 70 * 768                   # the best particle puts every return on an occupied voxel


def test_the_path_stays_in_the_rooms_air():
    import scan_match_cases as sc
    occ, L = sc.room_occupancy(), pc.scene()["L"]
    for v in pc.path()[0]:
        x, y, z = (int(c) for c in np.floor(v))
        assert not occ[x, y, z] and L[x, y, z] == -40
