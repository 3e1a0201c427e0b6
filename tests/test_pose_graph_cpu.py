"""Pose-graph optimisation on the CPU (no GPU): everything about ACCURACY is shown here on the numpy restatement of synth.py, which the
kernels equal bit for bit (tests/test_hip_pose_graph.py): the Jacobians are the residual's derivative, the residual ignores a
quaternion's sign and length, the block-sparse gather is the dense assembly, the optimiser ends where a dense Levenberg-Marquardt
with np.linalg.solve ends, a loop's drift is corrected, Geman-McClure finds the wrong closures; and the host layer refuses what it
must, by name."""
import ctypes
import re

import numpy as np
import pytest

import pose_graph_cases as pc
from trajectory_optimization_amd import synth

TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def _edges(c):
    return c["ab"], c["zt"], c["zq"]


@pytest.mark.parametrize("name", ["pair", "ring_5", "duplicate_edges", "ring_5_signs_and_norms", "two_components"])
def test_jacobians_are_the_central_differences_of_the_residual(name):
    """h = 1e-6: the truncation error is about h^2 = 1e-12 and the rounding error about 1e-16 / h = 1e-10 on entries that are O(1)
    (positions within 3 m, so a lever arm of at most 10): 1e-7 leaves three orders of magnitude."""
    c = pc.case(name)
    t, q = c["t"], c["q"]
    Ja, Jb = synth.pose_graph_jacobians_ref(t, q, *_edges(c))
    h, n = 1e-6, len(t)
    worst = 0.0
    for node in range(n):
        for col in range(6):
            x = np.zeros((n, 6))
            x[node, col] = h
            ep = synth.pose_graph_residual_ref(*synth.pose_graph_perturb_ref(t, q, x), *_edges(c))
            em = synth.pose_graph_residual_ref(*synth.pose_graph_perturb_ref(t, q, -x), *_edges(c))
            d = (ep - em) / (2.0 * h)
            for k, (a, b) in enumerate(c["ab"]):
                want = Ja[k][:, col] if a == node else Jb[k][:, col] if b == node else np.zeros(6)
                worst = max(worst, float(np.abs(d[k] - want).max()))
    print(f"{name}: the largest difference between a Jacobian entry and its central difference: {worst:.3e}")
    assert worst <= 1e-7


def test_residual_ignores_the_sign_and_the_length_of_every_quaternion():
    c = pc.case("ring_5")
    e = synth.pose_graph_residual_ref(c["t"], c["q"], *_edges(c))
    rng = np.random.default_rng(0)
    assert np.abs(e).max() > 0.05
    for trial in range(4):
        fq = rng.choice([-1.0, 1.0], (5, 1)) * rng.uniform(0.2, 5.0, (5, 1))
        fz = rng.choice([-1.0, 1.0], (5, 1)) * rng.uniform(0.2, 5.0, (5, 1))
        e2 = synth.pose_graph_residual_ref(c["t"], c["q"] * fq, c["ab"], c["zt"], c["zq"] * fz)
        assert np.abs(e2 - e).max() <= 1e-13      # (a few roundings of numbers below 1)
    assert np.array_equal(synth.pose_graph_residual_ref(c["t"], -c["q"], c["ab"], c["zt"], -c["zq"]), e)   # a sign alone changes no bit


def test_a_registration_becomes_an_absolute_edge_with_no_change_of_frame():
    from trajectory_optimization_amd import ops, tools
    rng = np.random.default_rng(3)
    M = rng.standard_normal((6, 6))
    A = M @ M.T
    A[[2, 3, 4]] = 0.0
    A[:, [2, 3, 4]] = 0.0                                         # a planar registration: dof 'xyw'
    q = np.asarray([0.9, 0.1, -0.2, 0.3])
    reg = tools.ScanRegistration(pose=np.asarray([1.0, -2.0, 0.5]), quat=q / np.sqrt((q * q).sum()), cost=12.5, rms=0.1, used=103, inside=100,
                                 iterations=5, accepted=4, status="CONVERGED", lam=1e-6, information=A, covariance=np.zeros((6, 6)))
    g = ops.PoseGraph(np.zeros((2, 3)), np.tile([1.0, 0, 0, 0], (2, 1)), fixed=[0]).add_registration(1, reg)
    sigma2 = 12.5 / (103 - 3)
    assert g.ab.tolist() == [[-1, 1]] and np.array_equal(g.omega[0], np.asarray([A[i, j] / sigma2 for i, j in TRIU]))
    assert np.array_equal(g.meas[0], np.concatenate([reg.pose, reg.quat]))
    e = synth.pose_graph_residual_ref(np.stack([np.zeros(3), reg.pose]), np.stack([[1.0, 0, 0, 0], 2.5 * reg.quat]), g.ab, g.meas[:, :3], g.meas[:, 3:])
    assert np.abs(e).max() <= 1e-15                               # zero at the registered pose, whatever the quaternion's length
    for status in ("DEGENERATE", "EMPTY"):
        reg.status = status
        with pytest.raises(ValueError, match=status):
            g.add_registration(1, reg)


@pytest.mark.parametrize("name", ["star_70", "two_components", "planar_xyw", "duplicate_edges"])
def test_the_gather_is_the_dense_assembly(name):
    """H and g from the same J and Omega by numpy's matrix products: the only difference is the order of sums of at most 70 terms,
    so 1e-12 of the largest entry."""
    c = pc.case(name)
    n, mask = len(c["t"]), pc.free_mask(c)
    rec = synth.pose_graph_linearize_ref(c["t"], c["q"], *_edges(c), c["omega"], mask)
    D, g, cost = synth.pose_graph_gather_ref(rec, c["ab"], n, mask)
    Ja, Jb = synth.pose_graph_jacobians_ref(c["t"], c["q"], *_edges(c))
    O = synth.pose_graph_omega_full(c["omega"])
    e = synth.pose_graph_residual_ref(c["t"], c["q"], *_edges(c))
    free = np.asarray([[(int(m) >> i) & 1 for i in range(6)] for m in mask], dtype=np.float64)
    H, gd = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for k, (a, b) in enumerate(c["ab"]):
        blocks = [(b, Jb[k] * free[b])] + ([(a, Ja[k] * free[a])] if a >= 0 else [])
        for i, Ji in blocks:
            gd[6 * i:6 * i + 6] += Ji.T @ O[k] @ e[k]
            for j, Jj in blocks:
                H[6 * i:6 * i + 6, 6 * j:6 * j + 6] += Ji.T @ O[k] @ Jj
    locked = free.reshape(-1) == 0
    H[locked, locked] = 1.0
    Dfull = np.zeros((n, 6, 6))
    for m, (i, j) in enumerate(TRIU):
        Dfull[:, i, j] = Dfull[:, j, i] = D[:, m]
    scale = np.abs(H).max()
    for i in range(n):
        assert np.abs(Dfull[i] - H[6 * i:6 * i + 6, 6 * i:6 * i + 6]).max() <= 1e-12 * scale
    assert np.abs(g.reshape(-1) - gd).max() <= 1e-12 * np.abs(gd).max()
    assert abs(cost - np.einsum("ki,kij,kj->", e, O, e)) <= 1e-12 * cost
    # and the off-diagonal blocks, through the product the solver uses (lambda = 0)
    p = np.random.default_rng(1).standard_normal((n, 6)) * free
    Ap = synth.pose_graph_matvec_ref(D, rec, c["ab"], 0.0, mask, p)
    assert np.abs(Ap.reshape(-1) - H @ p.reshape(-1)).max() <= 1e-12 * scale * np.abs(p).max() * 6 * n


# measured here: |cost - dense cost| / dense cost, and the bar at ten times that
DENSE = {"ring_5": (9.66e-16, 9.7e-15), "loop_300_12_closures": (1.45e-16, 1.5e-15)}


@pytest.mark.parametrize("name", sorted(DENSE))
def test_the_optimiser_ends_where_a_dense_levenberg_marquardt_ends(name):
    """pose_graph_optimize_ref (block-sparse, conjugate gradients, fixed order) against pose_graph_dense_ref (dense H, np.linalg.solve):
    both CONVERGED, after as many iterations, and the final costs agree.  Measured: ring_5 9.66e-16 relative (1.8390273112865527 against
    ...51), loop_300_12_closures 1.45e-16 (196.03655613661962 against ...965) — a unit or two in the last place, since the cost is
    stationary in the poses and the solves agree to cg_tol = 1e-8.  The bars are ten times the measured values."""
    c, s = pc.case(name), pc.reference(name)[30]
    d = synth.pose_graph_dense_ref(c["t"], c["q"], *_edges(c), c["omega"], fixed=c["fixed"])
    assert synth.POSEGRAPH_STATUS[s["status"]] == synth.POSEGRAPH_STATUS[d["status"]] == "CONVERGED"
    assert s["iterations"] == d["iterations"] and s["accepted"] == d["accepted"]
    rel = abs(s["cost"] - d["cost"]) / d["cost"]
    print(f"{name}: cost {s['cost']!r} against the dense {d['cost']!r}: {rel:.3e} relative; poses differ by {np.abs(s['t'] - d['t']).max():.3e} m")
    assert rel <= DENSE[name][1]
    assert np.abs(s["t"] - d["t"]).max() <= 1e-6


def test_a_loops_drift_is_corrected():
    """The 300-node double loop of synth.pose_graph_loop (biased odometry, 12 closures): the mean position error against the truth is
    4.261 m for the dead-reckoned start and 0.363 m after the optimisation, a factor 11.7 (measured).  The bar is a factor 5: a margin
    of more than two, against another seed's or another platform's rounding, not against a wrong answer: what remains is the noise of
    the closures and the drift between them."""
    c, s = pc.case("loop_300_12_closures"), pc.reference("loop_300_12_closures")[30]
    before, after = pc.mean_error(c["t"], c["truth_t"]), pc.mean_error(s["t"], c["truth_t"])
    print(f"mean position error {before:.3f} m -> {after:.3f} m: a factor {before / after:.1f}")
    assert after * 5.0 <= before and s["cost"] < 1e-4 * s["initial_cost"]


def test_geman_mcclure_finds_the_wrong_closures():
    c, s = pc.case("robust_two_wrong_closures"), pc.reference("robust_two_wrong_closures")[30]
    w = s["rec"][:, synth.PG_W]
    assert sorted(np.argsort(w, kind="stable")[:2].tolist()) == sorted(c["wrong"])
    assert w[list(c["wrong"])].max() < 1e-6 and np.delete(w, c["wrong"]).min() > 0.9
    assert (s["rec"][list(c["wrong"]), synth.PG_S] > 1e5).all()          # their chi^2 is how a caller finds them
    plain = synth.pose_graph_optimize_ref(c["t"], c["q"], *_edges(c), c["omega"], fixed=c["fixed"], iterations=10)
    robust_err, plain_err = pc.mean_error(s["t"], c["truth_t"]), pc.mean_error(plain["t"], c["truth_t"])
    print(f"mean position error: start {pc.mean_error(c['t'], c['truth_t']):.3f} m, plain {plain_err:.3f} m, robust {robust_err:.3f} m")
    assert synth.POSEGRAPH_STATUS[s["status"]] == "CONVERGED" and robust_err < plain_err


def test_the_cases_are_what_their_notes_say():
    row_ptr, inc = synth.pose_graph_incidence(pc.case("star_70")["ab"], 71)
    hub = inc[row_ptr[0]:row_ptr[1]]
    assert len(hub) == 70 and set((hub & 1).tolist()) == {0, 1} and np.array_equal(hub >> 1, np.arange(70))
    assert len(pc.case("loop_300_12_closures")["t"]) == 300 and len(pc.case("loop_300_12_closures")["ab"]) == 299 + 12
    assert (pc.case("ring_5_one_zero_omega")["omega"][5] == 0.0).all()
    q = pc.case("ring_5_signs_and_norms")["q"]
    assert (q[:, 0] < 0).any() and (q[:, 0] > 0).any() and np.abs(np.sqrt((q * q).sum(axis=1)) - 1.0).min() > 0.01
    for name in pc.NAMES:       # every case runs to an end that is not an error, and moves
        s = pc.reference(name)[30]
        assert synth.POSEGRAPH_STATUS[s["status"]] in ("CONVERGED", "RUNNING") and s["accepted"] >= 1 and s["cost"] < s["initial_cost"], name


def test_statuses_of_the_state_machine():
    c = pc.case("ring_5")
    args = (c["ab"], c["zt"], c["zq"], c["omega"])
    # an edge between nodes exactly half a turn apart: w(eps) = 0
    half = synth.pose_graph_optimize_ref(np.zeros((2, 3)), [[1.0, 0, 0, 0], [0.0, 0, 0, 1.0]], [[0, 1]], np.zeros((1, 3)), [[1.0, 0, 0, 0]],
                                         c["omega"][:1], fixed=[0], iterations=3)
    assert synth.POSEGRAPH_STATUS[half["status"]] == "NONFINITE" and half["iterations"] == 1
    # a node whose only edge has no information: a block pivot of 0
    om = c["omega"].copy()
    om[:] = 0.0
    deg = synth.pose_graph_optimize_ref(c["t"], c["q"], *args[:3], om, fixed=[0], iterations=3)
    assert synth.POSEGRAPH_STATUS[deg["status"]] == "DEGENERATE" and not deg["x"].any()
    # out of iterations: RUNNING
    run = synth.pose_graph_optimize_ref(c["t"], c["q"], *args, fixed=[0], iterations=2)
    assert synth.POSEGRAPH_STATUS[run["status"]] == "RUNNING" and run["iterations"] == 2
    # at the optimum already, no step lowers the cost: lambda climbs to its ceiling
    s = pc.reference("ring_5")[30]
    stall = synth.pose_graph_optimize_ref(s["t"], s["q"], *args, fixed=[0], iterations=40, tol_t=0.0, tol_r=0.0)
    assert synth.POSEGRAPH_STATUS[stall["status"]] in ("STALLED", "CONVERGED")


def test_the_host_layer_refuses_by_name():
    import torch
    from trajectory_optimization_amd import ops
    c = pc.case("two_components")
    n = len(c["t"])
    ops.check_pose_graph(n, c["ab"], c["fixed"])
    with pytest.raises(ValueError, match=r"node 4 belongs to a floating component \(5 nodes\)"):
        ops.check_pose_graph(n, c["ab"][:-1], c["fixed"])          # without its absolute edge the second component floats
    with pytest.raises(ValueError, match=r"node 0 belongs to a floating component"):
        ops.check_pose_graph(n, c["ab"], ())
    g = ops.PoseGraph(c["t"], c["q"], fixed=c["fixed"])
    eye = np.eye(6)
    with pytest.raises(ValueError, match=r"edge 0 = \(3, 3\): a and b must differ"):
        g.add_edges([3], [3], np.zeros((1, 3)), [[1.0, 0, 0, 0]], eye)
    with pytest.raises(ValueError, match=r"edge 0 = \(3, 9\): an index out of range for 9 nodes"):
        g.add_edges([3], [9], np.zeros((1, 3)), [[1.0, 0, 0, 0]], eye)
    with pytest.raises(ValueError, match=r"edge 0 = \(-2, 1\)"):
        g.add_edges([-2], [1], np.zeros((1, 3)), [[1.0, 0, 0, 0]], eye)
    bad = np.tile(eye, (2, 1, 1))
    bad[1, 4, 4] = -1.0
    with pytest.raises(ValueError, match=r"edge 1 has a non-finite entry or a negative diagonal entry"):
        g.add_edges([0, 1], [1, 2], np.zeros((2, 3)), np.tile([1.0, 0, 0, 0], (2, 1)), bad)
    with pytest.raises(ValueError, match=r"edge 0 is not symmetric"):
        g.add_edges([0], [1], np.zeros((1, 3)), [[1.0, 0, 0, 0]], eye + np.eye(6, k=1))
    assert g.n_edges == 0                                            # a refused call appended nothing
    with pytest.raises(ValueError, match="fixed: node 9 out of range"):
        ops.PoseGraph(c["t"], c["q"], fixed=[9])
    with pytest.raises(ValueError, match="robust must be None or a finite number > 0"):
        ops.check_pose_graph_options(robust=0.0)
    with pytest.raises(ValueError, match="cg_iterations"):
        ops.check_pose_graph_options(cg_iterations=0)
    assert ops.check_pose_graph_options(30, None, n_nodes=300)[:2] == (30, 1000) and ops.check_pose_graph_options(n_nodes=5)[1] == 30
    # an output that is an input, by name
    a, b = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    ops.check_pose_graph_buffers({"out": a}, {"meas": b})
    with pytest.raises(ValueError, match="the output `out` aliases `meas`"):
        ops.check_pose_graph_buffers({"out": b}, {"nodes": a, "meas": b})
    big = torch.zeros(16, dtype=torch.float64)
    with pytest.raises(ValueError, match="the output `out` aliases `meas`"):            # an overlap at an offset, not at the base
        ops.check_pose_graph_buffers({"out": big[7:15]}, {"meas": big[:8]})
    ops.check_pose_graph_buffers({"out": big[8:]}, {"meas": big[:8]})                     # back to back is no overlap


def test_the_c_entries_refuse_before_anything_is_enqueued():
    """Bad arguments come back as TOHIP_EINVAL / TOHIP_ENOSPC from the checks alone: the addresses are never touched (this machine
    needs no GPU for it)."""
    from trajectory_optimization_amd import _lib
    L, vp = _lib.lib(), ctypes.c_void_p
    n, e = 5, 5
    need = L.tohip_posegraph_workspace_bytes(n, e, 0)
    off = (ctypes.c_int64 * _lib.CONSTANTS["TOHIP_POSEGRAPH_REGIONS"])()
    assert L.tohip_posegraph_layout(n, e, off, 0) == 0 and need == 8 * off[len(off) - 1] and list(off) == sorted(off)
    assert L.tohip_posegraph_workspace_bytes(n, e, 1) == 0 and L.tohip_posegraph_workspace_bytes(0, e, 0) == 0
    assert L.tohip_posegraph_workspace_bytes((1 << 22) + 1, e, 0) == 0 and L.tohip_posegraph_layout(n, e, off, 1) == -1
    buf = [vp(0x100000 * (k + 1)) for k in range(8)]         # distinct, aligned, far apart, never dereferenced
    graph = buf[:6] + [n, e, 2 * e]
    einval, enospc = _lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]
    assert L.tohip_posegraph_gather(*graph, buf[6], need, None, 1) == einval                                  # flags
    assert L.tohip_posegraph_gather(*graph, buf[6], need - 8, None, 0) == enospc                              # a short workspace
    assert L.tohip_posegraph_gather(*graph, buf[1], need, None, 0) == einval                                  # the workspace is `meas`
    assert L.tohip_posegraph_gather(*(buf[:5] + [vp(0)]), n, e, 2 * e, buf[6], need, None, 0) == einval        # a null
    assert L.tohip_posegraph_gather(*(buf[:5] + [vp(0x600002)]), n, e, 2 * e, buf[6], need, None, 0) == einval # misaligned
    # an input that begins INSIDE the workspace, or ends inside it: ranges are compared, not base addresses
    assert L.tohip_posegraph_gather(*graph, vp(0x200000 - need + 8), need, None, 0) == einval                  # its last word is meas's first
    assert L.tohip_posegraph_gather(*graph, vp(0x200000 + 8 * 7 * e - 8), need, None, 0) == einval              # it begins at meas's last word
    assert L.tohip_posegraph_gather(*buf[:6], n, e, 2 * e + 1, buf[6], need, None, 0) == einval               # more incidences than 2 E
    assert L.tohip_posegraph_linearize(*graph, -1.0, buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_linearize(*graph, float("nan"), buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_step(*graph, 0, 1e-8, 1e-5, 1e-6, buf[6], need, None, 0) == einval               # no CG iteration
    assert L.tohip_posegraph_step(*graph, 4097, 1e-8, 1e-5, 1e-6, buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_step(*graph, 10, 1e-8, -1.0, 1e-6, buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_optimize(*graph, 0, 10, 1e-8, 0.0, 1e-5, 1e-6, buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_optimize(*graph, 257, 10, 1e-8, 0.0, 1e-5, 1e-6, buf[6], need, None, 0) == einval
    assert L.tohip_posegraph_optimize(*graph, 3, 10, 1e-8, 0.0, 1e-5, 1e-6, buf[6], need, None, 2) == einval
    assert L.tohip_posegraph_start(buf[6], n, e, buf[6], need, None, 0) == einval                             # nodes is the workspace
    assert L.tohip_posegraph_start(buf[0], n, e, buf[6], need, None, 4) == einval
    assert L.tohip_posegraph_result(n, e, buf[6], need, buf[6], None, 0) == einval                            # out is the workspace
    assert L.tohip_posegraph_result(n, e, buf[6], need - 1, buf[7], None, 0) == enospc
    assert L.tohip_posegraph_result(n, e, buf[6], need, vp(0x700000 + need - 8), None, 0) == einval            # out begins at the workspace's last word
    assert L.tohip_posegraph_start(vp(0x700000 - 8 * 7 * n + 8), n, e, buf[6], need, None, 0) == einval          # nodes ends inside the workspace


def test_the_header_and_the_bindings_name_the_same_entries():
    from trajectory_optimization_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    decls = dict(re.findall(r"\b(tohip_posegraph_\w+)\s*\(([^;{}]*)\)\s*;", text))
    assert set(decls) == {n for n in _lib.SIGNATURES if n.startswith("tohip_posegraph_")}
    assert set(decls) == {"tohip_posegraph_" + n for n in ("workspace_bytes", "layout", "start", "linearize", "gather", "step", "optimize", "result")}
    for name, params in decls.items():
        params = [" ".join(p.split()) for p in params.split(",")]
        assert params[-1] == "uint32_t flags", name                                       # the reserved word, last
        if any("stream" in p for p in params):
            assert params[-2] == "void *stream", name                                     # ... right behind the stream
    assert sum(any("stream" in p for p in v.split(",")) for v in decls.values()) == 6
