"""Plain numpy restatement of the occupancy grid's derived device state: the walk's 1-bit, bit-interleaved copy
(csrc/walk_layout.h), the 4x4x4 bricks with their coarse mask (csrc/traverse2.hip: pack_bricks_kernel), the flat 1-bit
packing (nfa_pack_bits) and the exact re-binarisation threshold.  Written from the rules, not from the kernels' loops:
the kernels go from a word to its cells (extract), this file goes from a cell to its bit (deposit)."""
import numpy as np


# ----------------------------------------------------------------------------- walk layout
def walk_layout(res):
    """(masks[3], bits): index bits per axis = ceil(log2(res)); positions are handed out in the rotation z, x, y; round 0
    always consumes a position (an axis of one cell leaves its position unused), exhausted axes are skipped in later
    rounds; bits = max(pos, 5) (a level is a whole number of 32-bit words)."""
    nb = [int(r - 1).bit_length() for r in res]
    masks = [0, 0, 0]
    pos = 0
    for rnd in range(max(max(nb), 1)):
        for ax in (2, 0, 1):
            if rnd < nb[ax]:
                masks[ax] |= 1 << pos
            if rnd == 0 or rnd < nb[ax]:
                pos += 1
    return masks, max(pos, 5)


def _mask_positions(mask):
    return [p for p in range(32) if (mask >> p) & 1]


def _deposit(v, mask):
    """Bit k of v goes to the k-th set position of mask (numpy integer arrays, or anything with >>, &, <<, |)."""
    out = v * 0
    for k, p in enumerate(_mask_positions(mask)):
        out = out | (((v >> k) & 1) << p)
    return out


def walk_bit_index(lvl, x, y, z, res):
    """Bit of cell (x, y, z) of level lvl in the walk's grid copy: lvl << bits | dep(x) | dep(y) | dep(z)."""
    masks, bits = walk_layout(res)
    lvl, x, y, z = (np.asarray(v, np.int64) for v in (lvl, x, y, z))
    return (lvl << bits) | _deposit(x, masks[0]) | _deposit(y, masks[1]) | _deposit(z, masks[2])


def walk_bit_index_torch(n_grids, res, device):
    """walk_bit_index of every cell of an [n_grids, *res] grid as an int64 tensor of that shape, in torch integer ops (for
    the one shape too large for the numpy version to be quick; equal to it on every small shape, tests/test_gridstate_cpu.py)."""
    import torch
    masks, bits = walk_layout(res)
    ar = lambda n: torch.arange(n, dtype=torch.int64, device=device)
    lvl = (ar(n_grids) << bits).view(-1, 1, 1, 1)
    x = _deposit(ar(res[0]), masks[0]).view(1, -1, 1, 1)
    y = _deposit(ar(res[1]), masks[1]).view(1, 1, -1, 1)
    z = _deposit(ar(res[2]), masks[2]).view(1, 1, 1, -1)
    return lvl | x | y | z


def walk_bits_words(n_grids, res):
    return ((n_grids << walk_layout(res)[1]) + 31) // 32


def _all_cell_bits(n_grids, res):
    l, x, y, z = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in (n_grids, *res)), indexing="ij")
    return walk_bit_index(l, x, y, z, res)


def _words_from_bits(bit_index, on, n_words):
    """uint32 words with bit (i & 31) of word (i >> 5) set for every i = bit_index[k] with on[k] (indices distinct: a sum of
    distinct powers of two below 2^32 is exact in float64)."""
    bit_index, on = np.asarray(bit_index).reshape(-1), np.asarray(on).reshape(-1) != 0
    sel = bit_index[on]
    w = np.bincount(sel >> 5, weights=np.ldexp(1.0, (sel & 31).astype(np.int64)), minlength=n_words)
    assert w.shape[0] == n_words
    return w.astype(np.uint64).astype(np.uint32)


def pack_walk_bits(binaries):
    """[n_grids, rx, ry, rz] bool (any non-zero = occupied) -> the walk's uint32 words, every padding bit 0."""
    b = np.asarray(binaries)
    return _words_from_bits(_all_cell_bits(b.shape[0], b.shape[1:]), b, walk_bits_words(b.shape[0], b.shape[1:]))


def _bits_of_words(words):
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32).reshape(-1)).astype("<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")


def unpack_walk_bits(words, n_grids, res):
    """-> (bool grid [n_grids, *res], the bits at the positions that belong to no cell)."""
    bits = _bits_of_words(words)
    assert bits.shape[0] == walk_bits_words(n_grids, res) * 32
    idx = _all_cell_bits(n_grids, res)
    is_cell = np.zeros(bits.shape[0], bool)
    is_cell[idx.reshape(-1)] = True
    return bits[idx].astype(bool), bits[~is_cell]


# ----------------------------------------------------------------------------- bricks
def brick_dims(res):
    return tuple((int(r) + 3) // 4 for r in res)


def bricks_words(n_grids, res):
    bx, by, bz = brick_dims(res)
    return n_grids * bx * by * bz


def pack_flat_bits(flags):
    """Cell i (non-zero = occupied) -> bit i & 31 of word i >> 5; unused bits of the last word 0."""
    f = (np.asarray(flags).reshape(-1) != 0).astype(np.uint8)
    by = np.packbits(f, bitorder="little")
    by = np.concatenate([by, np.zeros((-by.shape[0]) % 4, np.uint8)])
    return by.view("<u4").astype(np.uint32)


def pack_bricks(binaries):
    """-> (bricks uint64 [n_grids*bx*by*bz], coarse uint32): brick ((lvl*bx + kx)*by + ky)*bz + kz holds cell
    (4kx + i, 4ky + j, 4kz + k) at bit (i << 4) | (j << 2) | k; coarse bit b & 31 of word b >> 5 = brick b is not empty."""
    b = np.asarray(binaries) != 0
    n_grids, res = b.shape[0], b.shape[1:]
    bx, by, bz = brick_dims(res)
    w = np.zeros((n_grids, bx, by, bz), np.uint64)
    for i in range(4):
        for j in range(4):
            for k in range(4):
                part = b[:, i::4, j::4, k::4]
                if part.size:
                    w[:, :part.shape[1], :part.shape[2], :part.shape[3]] |= part.astype(np.uint64) << np.uint64((i << 4) | (j << 2) | k)
    w = w.reshape(-1)
    return w, pack_flat_bits(w != 0)


def unpack_bricks(bricks, n_grids, res):
    """-> (bool grid [n_grids, *res], the brick bits of positions beyond the grid's edge)."""
    bx, by, bz = brick_dims(res)
    w = np.asarray(bricks).view(np.uint64).reshape(n_grids, bx, by, bz)
    full = np.zeros((n_grids, 4 * bx, 4 * by, 4 * bz), bool)
    for i in range(4):
        for j in range(4):
            for k in range(4):
                full[:, i::4, j::4, k::4] = (w >> np.uint64((i << 4) | (j << 2) | k)) & np.uint64(1)
    inside = np.zeros(full.shape, bool)
    inside[:, :res[0], :res[1], :res[2]] = True
    return full[:, :res[0], :res[1], :res[2]].copy(), full[~inside]


# ----------------------------------------------------------------------------- threshold
def exact_threshold(occs, occ_thre):
    """(thre, mean) as float32: mean = float32(float64 sum / float64 count) over the entries >= 0 (NaN entries are not >= 0),
    NaN when there are none; thre = min(mean, occ_thre), NaN kept."""
    o = np.asarray(occs, np.float32).reshape(-1)
    sel = o[o >= 0]
    if sel.size == 0:
        return np.float32(np.nan), np.float32(np.nan)
    with np.errstate(all="ignore"):
        mean = np.float32(sel.astype(np.float64).sum() / np.float64(sel.size))
    thre = mean if np.isnan(mean) else np.float32(min(mean, np.float32(occ_thre)))
    return thre, mean


# ----------------------------------------------------------------------------- shapes and inputs shared by the two tiers
SHAPES = [(1, (1, 1, 1)), (2, (1, 1, 4)), (3, (2, 3, 5)), (1, (4, 4, 4)), (1, (5, 4, 3)), (2, (7, 1, 9)), (2, (16, 12, 20)),
          (1, (33, 31, 35)), (1, (3, 512, 2)), (2, (512, 1, 3)), (2, (130, 2, 66))]
LARGE = (3, (257, 129, 129))      # 25 index bits per level, 3 * 2^20 words: the word index passes the launch cap three times
BEYOND_WALK = (1, (513, 2, 2))    # more than 512 cells on an axis: the generic kernels and the torch re-binarisation
THIN = [s for s in SHAPES if min(s[1]) < 8] + [BEYOND_WALK]
PATTERNS = ("random", "none", "all", "last", "first")


def pattern(name, levels, res, seed=0):
    shape = (levels, *res)
    if name == "random":
        return np.random.default_rng(seed).random(shape) < 0.5
    b = np.full(shape, name == "all")
    if name == "last":
        b.reshape(-1)[-1] = True
    if name == "first":
        b.reshape(-1)[0] = True
    return b


def thin_grid(levels, res):
    """Contents of a THIN case: the random pattern; the one-cell grid is all True (an empty one gives no samples)."""
    return pattern("all" if tuple(res) == (1, 1, 1) else "random", levels, res, seed=7)


def level_aabbs(levels):
    """OccGridEstimator's boxes for roi [-1, 1]^3: level k is the roi scaled by 2^k about its centre."""
    return np.stack([np.array([-1, -1, -1, 1, 1, 1], np.float32) * np.float32(2.0 ** k) for k in range(levels)])


def thin_rays(n=600, seed=11):
    """Origins inside and outside the level-0 box, 10 % of the directions with a zero component."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * 3 - 1.5).astype(np.float32)
    o[: n // 2] *= np.float32(0.3)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    zero = rng.random(n) < 0.1
    d[zero, rng.integers(0, 3, int(zero.sum()))] = 0.0
    d /= np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-6).astype(np.float32)
    return o, d
