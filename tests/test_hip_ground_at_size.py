"""The ground layer on the GPU at size (ground_kernels.hip): columns 501 voxels tall — a floor run of 250 brick words, runs broken on
either side of a word boundary — headroom of 64 levels met exactly and missed by one, and the (2047, 2045, 511) grid through the
window in its far corner.  Every comparison is torch.equal (or integer equality) against synth.ground_ref / ground_snap_ref on the
inputs of tests/ground_size_cases.py, whose conditions tests/test_ground_at_size_cpu.py checks without a GPU."""
import numpy as np
import pytest
import torch

import ground_size_cases as gc
from map_size_cases import ORIGIN, RES

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _load(grid, bits):
    """Write a dense bool array into an OccupancyGrid's words (its header stays as tohip_occ_init left it) -> the grid."""
    grid.buf[256:].view(torch.int32).copy_(_t(synth.ground_pack(bits).view(np.int32), grid.device))
    return grid


def _want_buf(bits):
    """The whole buffer of a plane that holds `bits`: a zero header, the words, zero pad bits."""
    return torch.cat([torch.zeros(256, dtype=torch.uint8), torch.from_numpy(synth.ground_pack(bits).view(np.uint8))])


@pytest.mark.parametrize("unknown", synth.GROUND_UNKNOWN)
@pytest.mark.parametrize("scene", sorted(gc.SCENES))
def test_g1_tall_columns_and_headroom_at_its_cap(dev, scene, unknown):
    from trajectory_optimization_amd import ops
    occ, free = gc.SCENES[scene]()
    g = _load(ops.OccupancyGrid(ORIGIN, RES, occ.shape, device=dev), occ)
    space = ops.SpaceMap(g, _load(g.empty_like(), free))
    for H, s in gc.G1_SETTINGS:
        layer = ops.GroundLayer(space, H=H, step=s, unknown=unknown)
        ref = gc.g1_reference(scene, H, s, unknown)
        for k in gc.PLANES:
            got, want = getattr(layer, k).buf.cpu(), _want_buf(ref[k])
            if not torch.equal(got, want):
                dense = getattr(layer, k).dense().cpu().numpy().astype(bool)
                raise AssertionError((scene, unknown, H, s, k, np.argwhere(dense != ref[k])[:8].tolist()))


def test_g2_the_largest_grid_through_a_window_in_its_far_corner(dev):
    """(2047, 2045, 511): word indices up to 2^26 plus (uz - bz) sz, brick masks at three ragged far edges, every plane counted over
    67 M words.  Six 256 MB planes are alive at once; dense() is never called."""
    from trajectory_optimization_amd import ops
    occ = gc.window_scene()
    g = ops.OccupancyGrid(ORIGIN, RES, gc.G2_DIMS, device=dev)
    free = g.empty_like()
    for grid, bits in ((g, occ), (free, ~occ)):
        ijk = np.argwhere(bits) + gc.G2_OFF
        assert grid.insert(_t(((ijk + 0.5) * RES).astype(np.float32), dev)) == 0 and grid.count() == len(ijk)
    space = ops.SpaceMap(g, free)
    pos = _t(gc.g2_positions(), dev)
    for H, s, unknown in gc.G2_SETTINGS:
        ref = gc.g2_reference(H, s, unknown)
        layer = ops.GroundLayer(space, H=H, step=s, unknown=unknown)
        ijk = _t(ref["ijk"], dev)
        for k in gc.PLANES:
            got, want = getattr(layer, k).lookup(ijk).cpu().numpy(), ref["planes"][k].ravel().astype(np.uint8)
            bad = np.flatnonzero(got != want)
            assert not len(bad), (H, s, unknown, k, len(bad), ref["ijk"][bad[:5]].tolist())
            assert getattr(layer, k).count() == ref["count"][k], (H, s, unknown, k)
        for max_drop in gc.G2_DROPS:
            want_s, want_d, _ = gc.g2_snap(H, s, unknown, max_drop)
            standing, drop = layer.snap(pos, max_drop)
            assert torch.equal(drop.cpu(), torch.from_numpy(want_d)), (H, s, unknown, max_drop)
            assert torch.equal(standing.cpu().view(torch.int32), torch.from_numpy(want_s).view(torch.int32)), (H, s, unknown, max_drop)
        del layer, ijk
    del space, g, free, pos
    torch.cuda.empty_cache()
