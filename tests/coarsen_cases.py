"""The boxes, factors, offsets and fills shared by the tests of coarsening maps (tests/test_coarsen_cpu.py without a GPU,
tests/test_hip_coarsen.py and tests/test_hip_coarsen_contracts.py on one), and a per-voxel loop in Python integers that says what the
two entries compute without numpy.  Computed once per process and never modified.

The boxes are the resample cases' — (13, 10, 7) and (9, 14, 5), off the 4 x 4 x 2 brick in every axis, and one brick — and the fine
frame is theirs: origin a multiple of r = 1/8, so that every coarse origin here is exact in f32."""
import collections
import functools

import numpy as np

import reframe_cases as rfc
import resample_cases as rsc
from trajectory_optimization_amd import synth

ORIGIN, RES = rsc.ORIGIN, rsc.RES
SRC, DST, ONE = rsc.SRC, rsc.DST, rsc.ONE
PARAMS = rsc.PARAMS
FILLS = rsc.FILLS
FACTORS = (2, 3, 4, 8)
EVID_RULES, OCC_RULES = ("cover", "max"), ("any", "all")
EVID_MODES, OCC_MODES = rsc.EVID_MODES, rsc.OCC_MODES
Frame = rsc.Frame
values, bits, moved = rsc.values, rsc.bits, rsc.moved

Case = collections.namedtuple("Case", "name src dst factor offset")


def ceil_dims(n, o, f):
    """ceil((n - o) / f) per axis, at least 1: the coarse voxels that reach the far end of a source of n voxels from offset o."""
    return tuple(max(-((oa - na) // f), 1) for na, oa in zip(n, o))


def coarse_frame(src, f, o, dims):
    """The coarse frame whose voxel d holds the source voxels f d + o + e."""
    return Frame(moved(src.origin, o, src.resolution), f * src.resolution, dims)


def _cases():
    out = []
    for f in FACTORS:
        for tag, dims in (("box", SRC), ("one brick", ONE)):
            s = Frame(ORIGIN, RES, dims)
            table = [("at the origin", (0, 0, 0), None), ("an odd offset", (-1, -3, -1), None),
                     ("into a bigger map", (-3 * f + 1, -2 * f, -f - 1), DST)]
            if dims == SRC:
                table += [("a brick-aligned offset", (4, -8, 2), None), ("wholly outside", (100, 0, -40), DST)]
            for name, o, dd in table:
                out.append(Case(f"f={f} {tag} {name}", s, coarse_frame(s, f, o, dd or ceil_dims(dims, o, f)), f, o))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_IDS = [c.name for c in CASES]


def children(d, f, o):
    """The f^3 source voxels of coarse voxel d."""
    return [(f * d[0] + o[0] + ex, f * d[1] + o[1] + ey, f * d[2] + o[2] + ez) for ez in range(f) for ey in range(f) for ex in range(f)]


def coarsen_loop(src_bits, veto_bits, dst_bits, L_src, L_dst, f, o, params=PARAMS):
    """What the two entries are, voxel by voxel, in Python integers -> {('plane', rule, mode): (new, count)} — rule 'any', 'all' and
    'veto' (ANY with the veto plane) — and {('evid', rule, mode): (new, counts)}."""
    _, _, lmin, lmax, thr = synth.evidence_params(params)
    sd, dd = L_src.shape, L_dst.shape
    Ls, sb, vb = L_src.tolist(), src_bits.tolist(), veto_bits.tolist()
    S_evid = {r: np.zeros(dd, dtype=np.int64) for r in EVID_RULES}
    S_occ = {r: np.zeros(dd, dtype=bool) for r in (*OCC_RULES, "veto")}
    for i in range(dd[0]):
        for j in range(dd[1]):
            for k in range(dd[2]):
                vals, bts, vts = [], [], []
                for x, y, z in children((i, j, k), f, o):
                    if 0 <= x < sd[0] and 0 <= y < sd[1] and 0 <= z < sd[2]:
                        vals.append(Ls[x][y][z]), bts.append(sb[x][y][z]), vts.append(vb[x][y][z])
                    else:
                        vals.append(synth.EVID_UNKNOWN), bts.append(False), vts.append(False)
                occupied = [v for v in vals if v != synth.EVID_UNKNOWN and v > thr]
                S_evid["cover"][i, j, k] = max(occupied) if occupied else (synth.EVID_UNKNOWN if synth.EVID_UNKNOWN in vals else max(vals))
                S_evid["max"][i, j, k] = max(vals)
                S_occ["any"][i, j, k], S_occ["all"][i, j, k] = any(bts), all(bts)
                S_occ["veto"][i, j, k] = any(bts) and not any(vts)
    out = {}
    for rule, S in S_occ.items():
        out["plane", rule, "copy"] = (S, int(S.sum()))
        out["plane", rule, "or"] = (S | dst_bits, int((S & ~dst_bits).sum()))
    for rule, S in S_evid.items():
        for mode in EVID_MODES:
            new, counts = np.array(L_dst, dtype=np.int64), np.zeros(4, dtype=np.int64)
            for idx in np.ndindex(*dd):
                s, D = int(S[idx]), int(L_dst[idx])
                C = s if s == synth.EVID_UNKNOWN else min(max(s, lmin), lmax)
                N = {"copy": s, "add": D if s == synth.EVID_UNKNOWN else min(max((0 if D == synth.EVID_UNKNOWN else D) + s, lmin), lmax),
                     "confident": C if rfc._key(C) > rfc._key(D) else D}[mode]
                old = synth.EVID_UNKNOWN if mode == "copy" else D
                new[idx] = N
                counts += [N != old, old == synth.EVID_UNKNOWN and N != synth.EVID_UNKNOWN, N > thr and not old > thr, old > thr and not N > thr]
            out["evid", rule, mode] = (new, counts)
    return out


def inputs(case, fill):
    """(source bits, veto bits, dst bits, source values, dst values) of a case at a fill."""
    return (bits(case.src.dims, fill), bits(case.src.dims, 0.3, seed=2), bits(case.dst.dims, 0.3, seed=1), values(case.src.dims, fill),
            values(case.dst.dims, 0.6, seed=1))


# A block of the coarsen kernels holds 8, 4, 2 or 1 dst bricks (factor 2, 3, 4, 5 .. 8) and a launch has at most 2 048 blocks
# (occ_grid_blocks' cap): 41 x 41 x 11 = 18 491 dst bricks are a second trip for every factor, with a ragged tail for each of the four
# block sizes (18 491 is odd and 18 491 - 16 384 = 2 107 is no multiple of 8).  The source is small and its image covers dst's LAST
# bricks: the far corner.
BIG_DST = (163, 162, 21)
BIG_BRICKS = 41 * 41 * 11
assert BIG_BRICKS > 8 * 2048 and BIG_BRICKS % 2 == 1 and (BIG_BRICKS - 8 * 2048) % 8 != 0
BIG_SRC = (37, 30, 11)


def big_case(f):
    """The source ends one voxel short of the last child of dst's last voxel: f n_d + o - 1 = n_s per axis, so its image covers dst's
    last bricks and the offset is odd against the brick."""
    o = tuple(ns + 1 - f * nd for nd, ns in zip(BIG_DST, BIG_SRC))
    s = Frame(ORIGIN, RES, BIG_SRC)
    return Case(f"f={f} beyond one grid-stride pass", s, coarse_frame(s, f, o, BIG_DST), f, o)


LIMIT_SRC = (2048, 5, 3)


def limit_case(f):
    o = (-3, -1, 0)
    s = Frame(ORIGIN, RES, LIMIT_SRC)
    return Case(f"f={f} the per-axis limit", s, coarse_frame(s, f, o, ceil_dims(LIMIT_SRC, o, f)), f, o)


@functools.lru_cache(maxsize=None)
def big_values(dims):
    rng = np.random.default_rng(163 + dims[0])
    return np.where(rng.random(dims) < 0.7, rng.integers(PARAMS["lmin"], PARAMS["lmax"] + 1, dims), synth.EVID_UNKNOWN).astype(np.int8)
