"""Three contracts of every op that the bit-for-bit comparisons cannot see, over the one table of tests/contract_cases.py:

a. Plain run, twice on the default stream with no guard: every output equal bit for bit (a NaN equals the same NaN).
b. Guarded runs (tests/guarded_alloc.py) after ops.release_scratch(): every tensor a factory call makes sits between canary bands
   and `empty` ones are poisoned, with 0xFF and again with 0x00.  Both runs must equal the plain run bit for bit and no canary byte
   may have changed: a write past the end of an exact-size buffer, a size query a little too small, a read of memory the call never
   wrote and a header nobody cleared all show here.
c. Side-stream run: the inputs' device buffers hold the DECOYS (another seed's valid values); on a torch.cuda.Stream that is proven
   to run beside the default stream (the `side_stream` fixture: one stream in four of the pool shares the default stream's hardware
   queue and would hide a misplaced launch) a calibrated torch.cuda._sleep runs first, then the real inputs are copied in and the case runs.  Anything enqueued on the null
   stream executes during the sleep and sees decoys; a host read-back that does not wait for the given stream sees stale bytes.
   The outputs, read on that stream, must equal the plain run's.
d. Detection proofs, all inside memory the test owns: one element written past a guarded output through as_strided is reported
   for exactly that arena; a multiply launched explicitly on the default stream inside the side-stream harness returns the decoy's.
e. Coverage is counted: the cases run once over a recording proxy of the library, and the stream-taking entry points of
   _lib.SIGNATURES nobody called must equal contract_cases.NOT_DRIVEN.

Where ops.py deliberately allocates more than a size query reports, the guard sees less.  Those call sites are the users of
ops._scratch (+10 % and 256 bytes, cached per stream): _occlusion_rows_chunk's `zbuf`, `zvis`, `hvis`, `hcat`; _hpr_batched_mask's
`hidx`; cull_waypoints(scratch=True)'s `kept`, `kpts`, `cullws`; _with_hull_workspace(scratch=True)'s `hull`; and
allreduce_log_odds' `_compact` buffer (twice the count, at least 64 Ki floats).  The same workspaces are exact-size where the cases
call cull_waypoints, hidden_pts_removal and hidden_pts_removal_batched directly.

The side-stream delay.  torch.cuda._sleep's cycles are calibrated once per module with events (the difference of two sleeps, so that
the launch cancels); a case's delay is four times the host wall time of its second plain run — an upper bound on what the host
needs to enqueue it — and never less than 2 ms.  Measured on an MI355X: 8.37 ms for 2e7 cycles and 41.77 ms for 1e8, 2.40e6 cycles
per ms; the cases take 0.1 ms (hull_flip) to 6.5 ms (model_traj_forward_backward) on the host, median 1.3 ms, so the delays run from
the 2 ms floor to 25.9 ms.  The ordering guarantee holds up to a case's first host synchronisation (a count read back, an .item(),
a finiteness check): from there the sleep has drained and the check is best-effort, which is why objects with read-backs in the
middle of their build head cases of their own and evidence_fold_first folds before anything synchronises.
"""
import time

import numpy as np
import pytest
import torch

import contract_cases as cc
from guarded_alloc import GuardedAlloc

pytestmark = pytest.mark.gpu
MIN_DELAY_MS = 2.0
MAX_UNDEFINED = 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cycles_per_ms(dev):
    """torch.cuda._sleep's rate, measured with events: two sleeps of different lengths, so that the launch overhead cancels."""
    torch.cuda._sleep(1_000_000)   # (warm-up)
    torch.cuda.synchronize()
    ms = []
    for cycles in (20_000_000, 100_000_000):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    rate = 80_000_000 / (ms[1] - ms[0])
    assert ms[1] > ms[0] > 0 and rate > 0, ms
    print(f"torch.cuda._sleep: {ms[0]:.2f} ms for 2e7 cycles, {ms[1]:.2f} ms for 1e8: {rate:.0f} cycles per ms")
    return rate


def _misplaced_launch_probe(dev, side, cycles):
    """In the side-stream harness on `side`: a multiply of the input buffer launched explicitly on the default stream, and one on
    `side` -> (the misplaced result, the placed one, the real input).  The buffer holds the decoy -5 until the copy behind the
    sleep."""
    real = torch.arange(1, 260, dtype=torch.float32, device=dev)
    buf = torch.full((259,), -5.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        buf.copy_(real)
        with torch.cuda.stream(torch.cuda.default_stream(dev)):
            misplaced = buf * 2.0          # a launch that names the wrong stream: it runs during the sleep
        placed = buf * 2.0
        side.synchronize()
    torch.cuda.synchronize()
    return misplaced, placed, real


@pytest.fixture(scope="module")
def side_stream(dev, cycles_per_ms):
    """A torch.cuda.Stream that is proven to run beside the default stream.  The runtime multiplexes its streams onto a few hardware
    queues (GPU_MAX_HW_QUEUES, 4 by default): measured on an MI355X, every fourth stream of torch's pool shares the default stream's
    queue, and work misplaced onto the default stream is then serialised BEHIND that stream's sleep — it would read the real inputs
    and the harness would see nothing.  So streams are taken from the pool until the misplaced multiply of the probe returns the
    decoy's; the cases' side-stream runs use that one."""
    for attempt in range(8):
        side = torch.cuda.Stream(device=dev)
        misplaced, placed, real = _misplaced_launch_probe(dev, side, int(20.0 * cycles_per_ms))
        assert torch.equal(placed, real * 2.0)
        if torch.equal(misplaced, torch.full((259,), -10.0, device=dev)):
            print(f"side stream: the pool's stream number {attempt} runs beside the default stream")
            return side
    pytest.fail("no stream of the pool runs beside the default stream: the side-stream check would see nothing")


def _host(v):
    """An output on the host in a form that compares bit for bit: (shape, dtype, bytes)."""
    if torch.is_tensor(v):
        a = v.detach().contiguous().cpu()
        a = a.view(torch.uint8).numpy() if a.dtype == torch.bool else a.numpy()
    else:
        a = np.asarray(v)
    return a


def _to_host(out):
    return {k: _host(v) for k, v in out.items()}


def _differ(x, y):
    if x.shape != y.shape or x.dtype != y.dtype:
        return f"{x.shape} {x.dtype} against {y.shape} {y.dtype}"
    if x.tobytes() == y.tobytes():
        return None
    xb, yb = x.reshape(-1).view(np.uint8).reshape(x.size, -1), y.reshape(-1).view(np.uint8).reshape(y.size, -1)
    bad = np.flatnonzero((xb != yb).any(axis=1))
    i = int(bad[0])
    return f"{len(bad)} of {x.size} entries differ, the first at {i}: {x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r}"


def _masked(case, name, a):
    """`a` with the case's undefined region of output `name` zeroed (a copy), and the bytes that covers."""
    if name not in case.undefined:
        return a, 0
    index, reason = case.undefined[name]
    assert reason, f"{case.name}: undefined region of {name} without the line that declares it"
    a = a.copy()
    region = a[index]
    nbytes = region.size * a.dtype.itemsize
    assert 0 < nbytes < a.size * a.dtype.itemsize, f"{case.name}: the undefined region of {name} must be a proper part of it"
    a[index] = 0
    return a, nbytes


def assert_same(case, got, want, what):
    """Two runs' outputs on the host, bit for bit outside the case's `undefined` regions (and under the named bar for `loose`)."""
    assert got.keys() == want.keys(), (what, sorted(set(got) ^ set(want)))
    total = sum(v.size * v.dtype.itemsize for v in want.values())
    hidden = 0
    for k in want:
        x, nx = _masked(case, k, got[k])
        y, _ = _masked(case, k, want[k])
        hidden += nx
        if k in case.loose:
            rtol, atol, why = case.loose[k]
            assert why
            np.testing.assert_allclose(x, y, rtol=rtol, atol=atol, err_msg=f"{case.name}: {what}: {k} ({why})")
            continue
        diff = _differ(x, y)
        assert diff is None, f"{case.name}: {what}: {k}: {diff}"
    assert hidden <= MAX_UNDEFINED * total, f"{case.name}: {hidden} of {total} output bytes are declared undefined"


def _on_device(arrays, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}


def _plain(case, dev):
    out = _to_host(case.run(_on_device(case.inputs, dev)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):
    from trajectory_optimization_amd import ops
    # ---- a. plain, twice
    want = _plain(case, dev)
    t0 = time.perf_counter()
    again = _plain(case, dev)
    wall_ms = 1e3 * (time.perf_counter() - t0)
    assert_same(case, again, want, "the second plain run against the first")
    assert want

    # ---- b. guarded, poison 0xFF then 0x00
    for poison in (0xFF, 0x00):
        ops.release_scratch()
        with GuardedAlloc(dev, poison=poison) as guard:
            got = _to_host(case.run(_on_device(case.inputs, dev)))
            torch.cuda.synchronize()
            bad = guard.violations()
        assert len(guard.arenas) > 0
        assert not bad, f"{case.name}: poison {poison:#04x}: canary bytes changed:\n" + "\n".join(map(repr, bad))
        assert_same(case, got, want, f"the guarded run with poison {poison:#04x} against the plain run")
        del guard
    ops.release_scratch()

    # ---- c. side stream, behind a sleep, over buffers that held the decoys
    delay_ms = max(4.0 * wall_ms, MIN_DELAY_MS)
    bufs, real = _on_device(case.decoys, dev), _on_device(case.inputs, dev)
    torch.cuda.synchronize()
    side = side_stream
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(delay_ms * cycles_per_ms))
        for k in bufs:
            bufs[k].copy_(real[k])
        got = _to_host(case.run(bufs))
        side.synchronize()
    torch.cuda.synchronize()
    ops.release_scratch()
    print(f"{case.name}: plain run {wall_ms:.1f} ms on the host, side-stream delay {delay_ms:.1f} ms")
    assert_same(case, got, want, "the side-stream run against the plain run")


def test_case_table_is_well_formed():
    names = [c.name for c in cc.CASES]
    assert len(set(names)) == len(names)
    for c in cc.CASES:
        assert c.inputs.keys() == c.decoys.keys() and c.inputs
        for name, (index, reason) in c.undefined.items():
            assert reason and ("trajopt_hip.h" in reason or "ops.py" in reason or "DESIGN.md" in reason), (c.name, name)
        for name, (rtol, atol, why) in c.loose.items():
            assert ":" in why, (c.name, name)


# ---- d. detection proofs: every access stays in memory the test owns

def test_the_guard_reports_one_element_past_an_output(dev):
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(cc.cloud_path(0)["points"]).to(dev)
    with GuardedAlloc(dev) as guard:
        cloud = ops.PackedCloud(pts)
        d, idx = ops.clearance(cloud, pts[:259].contiguous(), 1.0)
        torch.cuda.synchronize()
        assert guard.violations() == []
        target = guard.owns(idx)
        assert target is not None and guard.arenas[target].nbytes == 259 * 4 and guard.owns(d) != target
        idx.as_strided((260,), (1,))[259] = 7        # what a kernel that ran one lane too far would do
        torch.cuda.synchronize()
        bad = guard.violations()
    assert [v.index for v in bad] == [target]
    assert bad[0].nbytes == 259 * 4 and bad[0].offsets and set(bad[0].offsets) <= {1036, 1037, 1038, 1039}
    assert bad[0].site[0].endswith("ops.py")


def test_the_side_stream_harness_sees_a_launch_on_the_default_stream(dev, cycles_per_ms, side_stream):
    misplaced, placed, real = _misplaced_launch_probe(dev, side_stream, int(20.0 * cycles_per_ms))
    assert torch.equal(placed, real * 2.0)
    assert torch.equal(misplaced, torch.full((259,), -10.0, device=dev))   # the decoy's: the harness would see a misplaced launch


# ---- e. coverage, counted

class _Recorder:
    """The loaded library, noting every tohip_* function that is CALLED through it (fetching one does not count)."""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tohip_"):
            return fn

        def call(*args):
            self._seen.add(name)
            return fn(*args)
        call.__name__ = name
        return call


def _stream_entries():
    """The entry points whose last argument is a stream: a c_void_p that the header names `stream`."""
    import re

    from trajectory_optimization_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    names = {m.group(1) for m in re.finditer(r"\b(tohip_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\s*\)\s*;", text, flags=re.S)}
    assert names and names <= set(_lib.SIGNATURES)
    return names


MAP_LAYER = ("tohip_occ_", "tohip_los_", "tohip_field_", "tohip_evid_", "tohip_travel_", "tohip_components_", "tohip_view_volume", "tohip_cast_",
             "tohip_depth_scan", "tohip_clearance_map", "tohip_assign_greedy")


def test_every_entry_point_is_driven_or_listed(dev):
    from trajectory_optimization_amd import _lib, ops
    real, seen = _lib.lib(), set()
    _lib._lib = _Recorder(real, seen)
    try:
        for case in cc.CASES:
            case.run(_on_device(case.inputs, dev))
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
        ops.release_scratch()
    assert _lib.lib() is real
    entries = _stream_entries()
    missed = entries - seen
    assert len(cc.NOT_DRIVEN) <= 20
    assert not [n for n in cc.NOT_DRIVEN if n.startswith(MAP_LAYER)], "no entry of the map layer may go undriven"
    assert all(reason for reason in cc.NOT_DRIVEN.values())
    assert missed == set(cc.NOT_DRIVEN), (f"neither driven nor listed: {sorted(missed - set(cc.NOT_DRIVEN))}; "
                                          f"listed but driven or unknown: {sorted(set(cc.NOT_DRIVEN) - missed)}")
