"""The seeded inputs shared by the two tests of re-framing and merging maps (tests/test_reframe_cpu.py without a GPU,
tests/test_hip_reframe.py on one): the small boxes — none a multiple of the 4 x 4 x 2 brick —, one shift per residue (rx, ry, rz) of
the brick, the fills, the two parameter sets, the word image of a plane, a per-voxel loop that says what a transfer is without a
slice, and the pair of boxes at size.  Computed once per process and never modified."""
import functools

import numpy as np

from trajectory_optimization_amd import synth

DIMS = [(1, 1, 1), (5, 6, 3), (13, 10, 7), (37, 5, 20)]
PAIRS = [(a, b) for a in DIMS for b in DIMS]                  # every box into every box: grow, crop, and the same dims
FILLS = [0.0, 0.02, 0.3, 1.0]
DEFAULT = dict(hit=17, miss=8, lmin=-40, lmax=70, threshold=0)
WIDE = dict(hit=127, miss=127, lmin=-127, lmax=127, threshold=0)
PARAMS = {"default": DEFAULT, "wide": WIDE}
LOOP_PAIRS = [((5, 6, 3), (9, 11, 5)), ((13, 10, 7), (5, 6, 3))]   # (source dims, destination dims) of the per-voxel check
LOOP_SHIFTS = [(x, y, z) for x in range(-5, 6) for y in range(-5, 6) for z in range(-3, 4)]
NO_OVERLAP = [(40, 0, 0), (0, -40, 0), (0, 0, 21), (-37, 0, 0), (4096, -4096, 4096)]   # shifts that leave no overlap between any two of DIMS

# the map layer's grid-stride launches have 2 048 blocks x 256 lanes: (515, 509, 81) has 129 x 128 x 41 = 676 992 words, a second
# trip with a ragged tail; the shift is unaligned on every axis
LANES = 2048 * 256
SIZE_BIG, SIZE_SMALL, SIZE_SHIFT = (515, 509, 81), (260, 517, 40), (-7, 9, 3)
assert 129 * 128 * 41 > LANES and (129 * 128 * 41 - LANES) % 256 != 0


def _residue_shifts():
    """One shift per residue (sx mod 4, sy mod 4, sz mod 2), 32 in all: the brick offsets vary with the residue so that positive and
    negative shifts, and shifts of more than a brick, all occur."""
    out = []
    for rz in range(2):
        for ry in range(4):
            for rx in range(4):
                k = rx + 4 * ry + 16 * rz
                out.append((rx + 4 * ((k % 4) - 2), ry + 4 * (((k // 3) % 3) - 1), rz + 2 * (((k // 5) % 4) - 2)))
    return out


RESIDUE_SHIFTS = _residue_shifts()
assert len({(x % 4, y % 4, z % 2) for x, y, z in RESIDUE_SHIFTS}) == 32
assert all(any(s[a] < 0 for s in RESIDUE_SHIFTS) and any(s[a] > 0 for s in RESIDUE_SHIFTS) for a in range(3))


@functools.lru_cache(maxsize=None)
def plane_bits(dims, fill, seed=0):
    """A random plane of `dims` with the share `fill` of its bits set (1.0: every bit)."""
    rng = np.random.default_rng(1000 * seed + 7 * dims[0] + dims[2] + int(100 * fill))
    return rng.random(dims) < fill


@functools.lru_cache(maxsize=None)
def evid_values(dims, params, fill=0.7, seed=0):
    """Random evidence values of `dims` for the parameter set named `params`: the share `fill` observed, uniform over [lmin, lmax]
    with both clamps, 0 and +-1 planted where there is room."""
    p = PARAMS[params]
    rng = np.random.default_rng(2000 * seed + 11 * dims[1] + dims[2] + len(params))
    L = np.where(rng.random(dims) < fill, rng.integers(p["lmin"], p["lmax"] + 1, dims), synth.EVID_UNKNOWN).astype(np.int64)
    flat = L.reshape(-1)
    special = [p["lmin"], p["lmax"], 0, 1, -1]
    if flat.size >= 2 * len(special):
        flat[rng.choice(flat.size, len(special), replace=False)] = special
    return L


def plane_words(bits):
    """The words of an occupancy grid holding `bits` (nx,ny,nz) bool -> (words,) uint32 in brick order, pad bits 0: what follows a
    plane's 256-byte header."""
    img = synth.evidence_brick_order(np.asarray(bits).astype(np.int64))[synth.EVID_HEADER:].view(np.int8)   # (1 where set, -128 in the pads)
    return np.packbits((img == 1).reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)   # bit b of a word: its b-th voxel


def _key(L):
    return -1 if L == synth.EVID_UNKNOWN else 2 * abs(L) + (L > 0)


def transfer_loop(bits, dst_bits, L_src, L_dst, shift, params):
    """What the transfers are, voxel by voxel, with no slice: -> {('plane', mode): (new, count)} for 'copy' and 'or', {('evid', mode):
    (new, counts)} for 'copy', 'add' and 'confident'."""
    _, _, lmin, lmax, thr = synth.evidence_params(params)
    sd, dd = bits.shape, dst_bits.shape
    plane = {"copy": np.zeros(dd, dtype=bool), "or": np.array(dst_bits, dtype=bool)}
    evid = {m: np.array(L_dst, dtype=np.int64) for m in ("copy", "add", "confident")}
    count = {"copy": 0, "or": 0}
    counts = {m: np.zeros(4, dtype=np.int64) for m in evid}
    for x in range(dd[0]):
        for y in range(dd[1]):
            for z in range(dd[2]):
                u = (x + shift[0], y + shift[1], z + shift[2])
                inside = all(0 <= u[a] < sd[a] for a in range(3))
                b = bool(bits[u]) if inside else False
                S = int(L_src[u]) if inside else synth.EVID_UNKNOWN
                plane["copy"][x, y, z] = b
                count["copy"] += b
                count["or"] += b and not dst_bits[x, y, z]
                plane["or"][x, y, z] |= b
                D = int(L_dst[x, y, z])
                C = S if S == synth.EVID_UNKNOWN else min(max(S, lmin), lmax)
                new = {"copy": S,
                       "add": D if S == synth.EVID_UNKNOWN else min(max((0 if D == synth.EVID_UNKNOWN else D) + S, lmin), lmax),
                       "confident": C if _key(C) > _key(D) else D}
                for m, N in new.items():
                    old = synth.EVID_UNKNOWN if m == "copy" else D   # (a copy does not read the destination: counted against an empty one)
                    evid[m][x, y, z] = N
                    counts[m] += [N != old, old == synth.EVID_UNKNOWN and N != synth.EVID_UNKNOWN, N > thr and not old > thr, old > thr and not N > thr]
    out = {("plane", m): (plane[m], count[m]) for m in plane}
    out.update({("evid", m): (evid[m], counts[m]) for m in evid})
    return out


@functools.lru_cache(maxsize=None)
def size_case():
    """The two boxes at size, random planes (30 %) and values (default parameters, 70 % observed, int8 to keep them small) ->
    dict(bits: {dims: plane}, vals: {dims: values})."""
    rng = np.random.default_rng(515)
    bits = {d: rng.random(d) < 0.3 for d in (SIZE_BIG, SIZE_SMALL)}
    vals = {d: np.where(rng.random(d) < 0.7, rng.integers(DEFAULT["lmin"], DEFAULT["lmax"] + 1, d), synth.EVID_UNKNOWN).astype(np.int8)
            for d in (SIZE_BIG, SIZE_SMALL)}
    return dict(bits=bits, vals=vals)
