"""The dense pass 1 launches as many persistent blocks as the chip holds at once (csrc/traj_kernels.hip: dense_blocks): every one
of them must be resident from the start — a block that waits for another to exit runs alone at the end — and the flat cut of the
(point block, waypoint) range into that many pieces must not change a bit of the result."""
import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _problem(dev, n, w, seed=5):
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(synth.make_cloud(n, seed=seed)).to(dev)
    poses, quats = synth.make_path(w, optical=True, jitter_seed=seed - 1)
    cloud = ops.PackedCloud(pts)
    return dict(pts=pts, cloud=cloud, cam=ops.Camera(K, IW, IH), p=torch.from_numpy(poses).to(dev), q=torch.from_numpy(quats).to(dev),
                ws=ops.TrajWorkspace(cloud, w), gout=torch.ones(1, device=dev))


@pytest.fixture(scope="module")
def stamped_problem(dev):
    return _problem(dev, 262_144, 128)


@pytest.mark.parametrize("occ", [False, True], ids=["plain", "occlusion"])
def test_every_dense_block_is_resident_from_the_start(dev, stamped_problem, occ):
    """262 144 points x 128 waypoints: nine to eleven waypoints of work per block (25-30 us) against a start spread of 1-4 us
    (measured).  Each XCD has its own 100 MHz counter, so per XCD: the latest start stamp is earlier than the earliest end stamp,
    i.e. no block began after another had finished.  The stamps of the third step are read, as bench.py's in_kernel_span does."""
    from trajectory_optimization_amd import _lib, ops
    L, c, n, w = _lib.lib(), stamped_problem, 262_144, 128
    bits = torch.full((w, c["cloud"].npad // 32), -1, dtype=torch.int32, device=dev) if occ else None
    nb = int(L.tohip_profile_clock_blocks(n, w, ops.DENSE, int(occ)))
    assert nb > 0
    # room for more blocks than any grid of this kernel has (8 per CU), zeroed: a launch whose grid is not nb is seen, not a fault
    cap = max(2 * nb, 8 * torch.cuda.get_device_properties(dev).multi_processor_count + 1)
    buf = torch.zeros(6 * cap, dtype=torch.int64, device=dev)
    L.tohip_profile_clock(buf.data_ptr())
    try:
        for _ in range(3):
            ops.traj_forward_backward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], c["gout"], flags=ops.DENSE, occ=bits)
        torch.cuda.synchronize(dev)
    finally:
        L.tohip_profile_clock(None)
    raw = buf.cpu().numpy()
    assert not raw[6 * nb:].any(), "the launch stamped more blocks than tohip_profile_clock_blocks answers"
    pair, ext = raw[:2 * nb].reshape(nb, 2), raw[2 * nb:6 * nb].reshape(nb, 4)
    assert int((ext[:, 1] != 0).sum()) == nb and int((pair[:, 1] > 0).sum()) == nb
    xcd = ext[:, 3] & 0xf
    for x in np.unique(xcd):
        start, end = ext[xcd == x, 0], ext[xcd == x, 1]
        print(f"{'occlusion' if occ else 'plain'} xcd {x}: {len(start)} blocks, start spread {(start.max() - start.min()) * 0.01:.2f} us, "
              f"end spread {(end.max() - end.min()) * 0.01:.2f} us, first start -> last end {(end.max() - start.min()) * 0.01:.2f} us")
        assert start.max() < end.min(), (int(x), int(start.max() - start.min()), int(end.min() - start.min()))


# 50 000 x 37: fewer (point block, waypoint) pairs than resident blocks, a piece is one pair; 200 000 x 37: about two pairs per
# piece, which no waypoint count divides evenly — pieces begin inside one point block and end inside the next
@pytest.mark.parametrize("occ", [False, True], ids=["plain", "occlusion"])
@pytest.mark.parametrize("n,w", [(50_000, 37), (200_000, 37)])
def test_dense_equals_culled_bitwise_where_pieces_straddle_point_blocks(dev, n, w, occ):
    from trajectory_optimization_amd import ops
    c = _problem(dev, n, w)
    bits = ops.occlusion_bits(c["cloud"], c["pts"], c["p"], c["q"], c["cam"], 1.0, 15.0, "zbuffer") if occ else None
    outs = {}
    for name, flags in (("dense", ops.DENSE), ("culled", 0)):
        o = ops.traj_forward_backward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], c["gout"], flags=flags, occ=bits)
        torch.cuda.synchronize(dev)
        rewards, scalars, pg, qg, lo_sum, minmax = (t.cpu().numpy() for t in o)
        outs[name] = dict(rewards=rewards, scalars=scalars, pg=pg, qg=qg, lo_sum=lo_sum[:n], minmax=minmax)
    assert np.isfinite(outs["dense"]["pg"]).all() and np.abs(outs["dense"]["pg"]).max() > 0
    for key, a in outs["dense"].items():
        assert np.array_equal(a.view(np.uint32), outs["culled"][key].view(np.uint32)), key
