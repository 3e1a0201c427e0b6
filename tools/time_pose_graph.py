"""What pose-graph optimisation costs ("Pose graph"), in one process, on two graphs:

  loop   synth.pose_graph_loop(500, 2 laps, 201 closures): 1 000 nodes, 1 200 edges, a biased odometry chain closed every few nodes
  grid   50 000 nodes on a 250 x 200 lattice visited row by row, 250 000 edges: the odometry chain and the lattice's other neighbours
         (up, the two diagonals, two ahead, two up), cut at the count; truth plus noise, started from a perturbed truth

Medians of --reps windows.

  linearize, gather   one launch each (event-timed, 20 calls per window)
  step                the accept / reject / factor launch and ONE conjugate-gradient iteration (two launches), from a fresh start
                      each call so that the iteration runs (event-timed with its start, linearize and gather; their time subtracted)
  cg_iteration        the difference of a step with 101 and with 1 iterations, over 100 (both event-timed)
  optimize            PoseGraphProblem.start + optimize + result, launches only, and what it did: outer iterations, accepted steps,
                      CG iterations in total, status, cost (event-timed, 1 call per window)
  end_to_end          PoseGraph.optimize: the check, the incidence list, the upload, the launches, the read-back (wall-clock)
  spsolve             the same Levenberg-Marquardt on the host: synth's linearisation, the normal matrix assembled as a scipy.sparse
                      CSR matrix, scipy.sparse.linalg.spsolve per step (wall-clock, ONE run: it is a baseline for scale), on the loop
                      and on the same lattice at 2 000 and 10 000 nodes, which are measured on the device as well; of the 50 000-node
                      lattice ONE solve of the first damped system, in a fresh process ended after --big-solve-limit seconds: what is
                      recorded is its time, or that it did not finish within the limit

Nothing here is a bar: the numbers are recorded in profiles/time_pose_graph.json.

    python tools/time_pose_graph.py [--reps 5] [--big-solve-limit 240] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trajectory_optimization_amd import ops, synth  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402

TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def grid_graph(nx=250, ny=200, n_edges=250_000, seed=0, sigma_t=0.02, sigma_r=0.01):
    """-> dict like synth.pose_graph_loop's: the lattice graph of the module's docstring."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    ix = np.where(iy % 2 == 0, ix, nx - 1 - ix)                                  # row by row, there and back
    cell = np.stack([ix.reshape(-1), iy.reshape(-1)], axis=1)                    # lattice cell of node k, in visit order
    index = np.full((ny, nx), -1, dtype=np.int64)                                # and the node of a cell
    index[cell[:, 1], cell[:, 0]] = np.arange(n)
    truth_t = np.concatenate([0.5 * cell, 0.1 * np.sin(0.05 * cell[:, :1])], axis=1).astype(np.float64)
    yaw = 0.3 * np.sin(0.01 * np.arange(n))
    truth_q = np.stack([np.cos(yaw / 2), 0.02 * np.sin(0.03 * np.arange(n)), 0.02 * np.cos(0.03 * np.arange(n)), np.sin(yaw / 2)], axis=1)
    pairs = [np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)]
    for dx, dy in ((0, 1), (1, 1), (-1, 1), (2, 0), (0, 2)):
        x0, y0 = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
        x1, y1 = x0 + dx, y0 + dy
        ok = (x1 >= 0) & (x1 < nx) & (y1 < ny)
        a, b = index[y0[ok], x0[ok]], index[y1[ok], x1[ok]]
        keep = np.abs(a - b) != 1                                                 # (the chain has those)
        pairs.append(np.stack([a[keep], b[keep]], axis=1))
    ab = np.concatenate(pairs)
    assert len(ab) >= n_edges
    ab = ab[:n_edges]
    zt, zq = synth.pose_graph_relative_ref(truth_t[ab[:, 0]], truth_q[ab[:, 0]], truth_t[ab[:, 1]], truth_q[ab[:, 1]])
    m = len(ab)
    zt = zt + sigma_t * rng.standard_normal((m, 3))
    zq = synth._quat_mul_np(np.concatenate([np.ones((m, 1)), 0.5 * sigma_r * rng.standard_normal((m, 3))], axis=1), zq)
    omega = np.zeros((m, 21))
    for k, (i, j) in enumerate(TRIU):
        if i == j:
            omega[:, k] = 1.0 / sigma_t ** 2 if i < 3 else 1.0 / sigma_r ** 2
    t = truth_t + 0.1 * rng.standard_normal((n, 3))
    q = synth._quat_mul_np(np.concatenate([np.ones((n, 1)), 0.5 * 0.03 * rng.standard_normal((n, 3))], axis=1), truth_q)
    t[0], q[0] = truth_t[0], truth_q[0]
    return dict(truth_t=truth_t, truth_q=truth_q, t=t, q=q, ab=ab.astype(np.int32), zt=zt, zq=zq, omega=omega)


def full_blocks(tri):
    """(E,21) upper triangles -> (E,6,6) symmetric blocks."""
    M = np.zeros((len(tri), 6, 6))
    for k, (i, j) in enumerate(TRIU):
        M[:, i, j] = M[:, j, i] = tri[:, k]
    return M


def assemble(rec, ab, n):
    """The edge records -> (H as a scipy.sparse CSR matrix (6 n, 6 n), the gradient (6 n,))."""
    import scipy.sparse as sp
    r6, c6 = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    rows, cols, vals = [], [], []
    for blocks, ri, ci in ((full_blocks(rec[:, synth.PG_HAA:synth.PG_HAA + 21]), ab[:, 0], ab[:, 0]),
                           (full_blocks(rec[:, synth.PG_HBB:synth.PG_HBB + 21]), ab[:, 1], ab[:, 1]),
                           (rec[:, synth.PG_HAB:synth.PG_HAB + 36].reshape(-1, 6, 6), ab[:, 0], ab[:, 1]),
                           (rec[:, synth.PG_HAB:synth.PG_HAB + 36].reshape(-1, 6, 6).transpose(0, 2, 1), ab[:, 1], ab[:, 0])):
        rows.append((6 * ri[:, None, None] + r6).reshape(-1))
        cols.append((6 * ci[:, None, None] + c6).reshape(-1))
        vals.append(blocks.reshape(-1))
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n)).tocsr()
    grad = np.zeros(6 * n)
    np.add.at(grad, (6 * ab[:, 0:1] + np.arange(6)).reshape(-1), rec[:, synth.PG_GA:synth.PG_GA + 6].reshape(-1))
    np.add.at(grad, (6 * ab[:, 1:2] + np.arange(6)).reshape(-1), rec[:, synth.PG_GB:synth.PG_GB + 6].reshape(-1))
    return H, grad


def one_solve(nx, ny):
    """The first damped system of the nx x ny lattice, assembled, and ONE scipy.sparse.linalg.spsolve of it timed: host only."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    g = grid_graph(nx, ny, 5 * nx * ny)
    n, ab = nx * ny, g["ab"].astype(np.int64)
    mask = synth.pose_graph_free_masks(n, [0], 63)
    free = np.repeat(mask != 0, 6)
    H, grad = assemble(synth.pose_graph_linearize_ref(g["t"], g["q"], ab, g["zt"], g["zq"], g["omega"], mask), ab, n)
    A = (H + synth.POSEGRAPH_LAMBDA0 * sp.diags(H.diagonal()))[free][:, free].tocsc()
    t0 = time.perf_counter()
    x = spsolve(A, -grad[free])
    return dict(nodes=n, edges=len(ab), unknowns=int(A.shape[0]), nnz=int(A.nnz), seconds=time.perf_counter() - t0, finite=bool(np.isfinite(x).all()))


def spsolve_lm(g, iterations):
    """Levenberg-Marquardt with scipy.sparse.linalg.spsolve on the host, the optimiser's state machine -> dict(seconds, iterations,
    accepted, status, cost, seconds per solve)."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    n, ab = len(g["t"]), g["ab"].astype(np.int64)
    mask = synth.pose_graph_free_masks(n, [0], 63)
    free = np.repeat(mask != 0, 6)
    t, q, x = g["t"].copy(), g["q"].copy(), np.zeros((n, 6))
    lam, cost, status, accepted, done, solves = synth.POSEGRAPH_LAMBDA0, 0.0, 0, 0, 0, []
    H = grad = None
    t0 = time.perf_counter()
    for it in range(iterations):
        done += 1
        tt, tq = synth.pose_graph_perturb_ref(t, q, x)
        rec = synth.pose_graph_linearize_ref(tt, tq, ab, g["zt"], g["zq"], g["omega"], mask)
        c = float(rec[:, synth.PG_RHO].sum())
        if it == 0 or c < cost:
            t, q, cost = tt, tq, c
            H, grad = assemble(rec, ab, n)
            if it > 0:
                accepted += 1
                lam = max(lam / 8.0, 2.0 ** -30)
                if (np.abs(x[:, :3]) <= 1e-5).all() and (np.abs(x[:, 3:]) <= 1e-6).all():
                    status = 1
                    break
        else:
            lam *= 8.0
            if lam > 2.0 ** 30:
                status = 2
                break
        A = (H + lam * sp.diags(H.diagonal()))[free][:, free].tocsc()
        s0 = time.perf_counter()
        sol = spsolve(A, -grad[free])
        solves.append(time.perf_counter() - s0)
        x = np.zeros(6 * n)
        x[free] = sol
        x = x.reshape(n, 6)
    return dict(seconds=time.perf_counter() - t0, iterations=done, accepted=accepted, status=synth.POSEGRAPH_STATUS[status], cost=cost,
                seconds_per_solve=float(np.median(solves)) if solves else None)


def measure(name, g, reps, dev):
    graph = ops.PoseGraph(g["t"], g["q"], fixed=[0], device=dev).add_edges(g["ab"][:, 0], g["ab"][:, 1], g["zt"], g["zq"], g["omega"])
    n, e = graph.n_nodes, graph.n_edges
    cg = ops.check_pose_graph_options(n_nodes=n)[1]
    res = {"nodes": n, "edges": e, "cg_iterations_per_solve": cg, "workspace_MB": ops.pose_graph_layout(n, e)["total"] * 8 / 2 ** 20}
    p = graph.upload()
    res["start_ms"] = event_ms(lambda: p.start(), reps, 20)
    res["linearize_ms"] = event_ms(lambda: p.start().linearize(), reps, 20) - res["start_ms"]
    res["gather_ms"] = event_ms(lambda: p.start().linearize().gather(), reps, 20) - res["linearize_ms"] - res["start_ms"]
    before = res["start_ms"] + res["linearize_ms"] + res["gather_ms"]
    one = event_ms(lambda: p.start().linearize().gather().step(1), reps, 20) - before
    many = event_ms(lambda: p.start().linearize().gather().step(101, cg_tol=0.0), reps, 5) - before
    res["step_with_one_cg_iteration_ms"] = one
    res["cg_iteration_ms"] = (many - one) / 100.0
    res["optimize_ms"] = event_ms(lambda: p.start().optimize(30, cg).result(), reps, 1)
    r = ops.pose_graph_result(p.start().optimize(30, cg).result().cpu().numpy(), n, e)
    res.update(outer_iterations=r.iterations, accepted=r.accepted, cg_iterations_total=r.cg_iterations, status=r.status, cost=r.cost,
               initial_cost=r.initial_cost, launches=30 * (3 + 2 * cg) + 2)
    err = lambda t: float(np.sqrt(((t - g["truth_t"]) ** 2).sum(axis=1)).mean())   # noqa: E731
    res["mean_error_before_m"], res["mean_error_after_m"] = err(g["t"]), err(r.poses)
    res["end_to_end_ms"] = wall_ms(lambda: graph.optimize(), reps)
    print(json.dumps({name: res}), flush=True)
    return res


def baseline(res, g, iterations):
    res["spsolve"] = dict(spsolve_lm(g, iterations), iterations_allowed=iterations, runs=1)
    print(json.dumps({"spsolve": res["spsolve"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big-solve-limit", type=float, default=240.0, help="seconds the 50 000-node lattice's one host solve may take")
    ap.add_argument("--one-solve", type=int, nargs=2, metavar=("NX", "NY"), default=None, help="host only: time one spsolve of a lattice")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.one_solve:
        print(json.dumps(one_solve(*a.one_solve)), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def save():
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(res, fh, indent=1)
    loop = synth.pose_graph_loop(500, 2, 0.02, 0.01, 201, seed=0)
    res["loop_1000_1200"] = measure("loop_1000_1200", loop, a.reps, dev)
    baseline(res["loop_1000_1200"], loop, 30)
    for nx, ny, allowed in ((50, 40, 10), (125, 80, 2)):          # the same lattice smaller: where the host's direct solve still runs
        g = grid_graph(nx, ny, 5 * nx * ny)
        name = f"grid_{nx * ny}_{5 * nx * ny}"
        res[name] = measure(name, g, a.reps, dev)
        baseline(res[name], g, allowed)
        save()
    res["grid_50000_250000"] = measure("grid_50000_250000", grid_graph(), a.reps, dev)
    save()
    # the large lattice on the host: ONE solve, in a fresh process that never opens the device, ended at the limit
    cmd = [sys.executable, os.path.abspath(__file__), "--one-solve", "250", "200"]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.big_solve_limit, check=True).stdout
        res["grid_50000_250000"]["spsolve_one_solve"] = json.loads(out.strip().split("\n")[-1])
    except subprocess.TimeoutExpired:
        res["grid_50000_250000"]["spsolve_one_solve"] = {"did_not_finish_within_s": a.big_solve_limit}
    save()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
