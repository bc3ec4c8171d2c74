"""GPU tier of the occupancy grid's device state: the packers (nfa_pack_walk_bits, nfa_pack_bricks, nfa_pack_bits) against
the cell-to-bit restatement of tests/gridstate_reference.py on every cell and every padding bit, nfa_grid_rebinarize on
inputs whose mean is exact, nfa_grid_ema_update / nfa_grid_cell_points against the oracle bit for bit (special values,
duplicates, a second trip of the grid-stride loops), and thin / over-wide grids through the traversal and the estimator."""
import ctypes as C

import numpy as np
import pytest
import torch

import gridstate_reference as R
import nerfacc_amd as na
from nerfacc_amd import _backend as B

pytestmark = pytest.mark.gpu

CAP = 4096 * 256          # threads of the largest launch grid_1d gives (csrc/common.hip.h): beyond it a loop takes a second trip


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _res(res):
    return (C.c_int32 * 3)(*[int(v) for v in res])


def _u32(t):
    """A device int32 / int64 word tensor as numpy unsigned words."""
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint64)


def _same_floats(a, b):
    """NaN against NaN, values by ==."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _neg(f):
    """f with the sign bit set (a NaN keeps its payload)."""
    return (np.float32(f).view(np.uint32) | np.uint32(0x80000000)).view(np.float32)


def dev_pack_walk_bits(b):
    """nfa_pack_walk_bits of a device bool / uint8 grid [levels, rx, ry, rz] into words that start as all ones."""
    levels, res = b.shape[0], b.shape[1:]
    n_words = int(B.load().nfa_walk_bits_words(levels, _res(res)))
    assert n_words == R.walk_bits_words(levels, res)
    bits = torch.full((n_words + 1,), -1, dtype=torch.int32, device=b.device)      # (+1: a guard word)
    B.call("nfa_pack_walk_bits", B.ptr(b), levels, _res(res), B.ptr(bits), B.stream())
    assert int(bits[-1]) == -1
    return bits[:-1]


def dev_pack_bricks(b):
    levels, res = b.shape[0], b.shape[1:]
    n = int(B.load().nfa_bricks_words(levels, _res(res)))
    assert n == R.bricks_words(levels, res)
    bricks = torch.full((n + 1,), -1, dtype=torch.int64, device=b.device)
    coarse = torch.full(((n + 31) // 32 + 1,), -1, dtype=torch.int32, device=b.device)
    B.call("nfa_pack_bricks", B.ptr(b), levels, _res(res), B.ptr(bricks), B.ptr(coarse), B.stream())
    assert int(bricks[-1]) == -1 and int(coarse[-1]) == -1
    return bricks[:-1], coarse[:-1]


def dev_pack_bits(flat):
    n = flat.numel()
    bits = torch.full(((n + 31) // 32 + 1,), -1, dtype=torch.int32, device=flat.device)
    B.call("nfa_pack_bits", B.ptr(flat), n, B.ptr(bits), B.stream())
    assert int(bits[-1]) == -1
    return bits[:-1]


def dev_expected_walk_words(b):
    """The walk's words of a device grid from the torch-integer cell-to-bit map (distinct bits: the sum is the or)."""
    levels, res = b.shape[0], tuple(b.shape[1:])
    idx = R.walk_bit_index_torch(levels, res, b.device).reshape(-1)
    words = torch.zeros(R.walk_bits_words(levels, res), dtype=torch.int64, device=b.device)
    words.index_add_(0, idx >> 5, (b.reshape(-1) != 0).to(torch.int64) << (idx & 31))
    return words


_LARGE = {}


def large_grids(dev):
    """The patterns of LARGE on the device, made once and never written."""
    if not _LARGE:
        for name in R.PATTERNS:
            _LARGE[name] = T(R.pattern(name, *R.LARGE, seed=5), dev)
    return _LARGE


# ----------------------------------------------------------------------------- a. packers
@pytest.mark.parametrize("levels,res", R.SHAPES)
def test_packers_every_cell_and_padding_bit(dev, levels, res):
    for name in R.PATTERNS:
        b = R.pattern(name, levels, res, seed=3)
        words = _u32(dev_pack_walk_bits(T(b, dev)))
        back, pad = R.unpack_walk_bits(words, levels, res)
        assert (back == b).all(), name
        assert not pad.any(), name
        assert (words == R.pack_walk_bits(b)).all(), name
        bricks, coarse = dev_pack_bricks(T(b, dev))
        rb, rc = R.pack_bricks(b)
        assert (_u32(bricks) == rb).all() and (_u32(coarse) == rc).all(), name
        assert (_u32(dev_pack_bits(T(b, dev).view(-1))) == R.pack_flat_bits(b)).all(), name


def test_walk_packer_large_second_loop_trip(dev):
    levels, res = R.LARGE
    assert R.walk_bits_words(levels, res) == 3 << 20 and (3 << 20) > 2 * CAP
    for name, b in large_grids(dev).items():
        words = dev_pack_walk_bits(b)
        assert torch.equal(words.to(torch.int64) & 0xFFFFFFFF, dev_expected_walk_words(b)), name


def test_brick_packer_second_loop_trip(dev):
    levels, res = 1, (1, 1, 4194312)
    assert R.bricks_words(levels, res) == 1048578 and R.bricks_words(levels, res) > CAP
    for name in ("random", "last", "all"):
        b = R.pattern(name, levels, res, seed=4)
        bricks, coarse = dev_pack_bricks(T(b, dev))
        rb, rc = R.pack_bricks(b)
        assert (_u32(bricks) == rb).all() and (_u32(coarse) == rc).all(), name


@pytest.mark.parametrize("n_cells", [1, 31, 32, 33, 63, 64, 65, 4097])
def test_pack_bits_flat(dev, n_cells):
    rng = np.random.default_rng(n_cells)
    for flags in (rng.random(n_cells) < 0.5, np.ones(n_cells, bool), np.zeros(n_cells, bool),
                  rng.choice(np.array([0, 1, 2, 255], np.uint8), n_cells)):       # uint8: any non-zero byte is occupied
        assert (_u32(dev_pack_bits(T(flags, dev))) == R.pack_flat_bits(flags)).all()
    src = np.array([0, 1, 2, 255] * 17, np.uint8)[:n_cells]
    assert (_u32(dev_pack_bits(T(src, dev))) == R.pack_flat_bits(src)).all()


def test_pack_bits_large_second_loop_trip(dev):
    for name in ("random", "last", "first"):
        b = large_grids(dev)[name]
        assert b.numel() > 12 * CAP
        assert (_u32(dev_pack_bits(b.view(-1))) == R.pack_flat_bits(b.cpu().numpy())).all(), name


# ----------------------------------------------------------------------------- b. nfa_grid_rebinarize
def dev_rebinarize(occs, levels, res, occ_thre):
    """-> (binaries uint8 [levels, *res], walk words int32, thre, mean): the outputs start as bytes of 2 / words of all ones,
    {thre, mean} are read from the scratch at byte offset scratch_bytes - 16."""
    dev = occs.device
    n_bytes = int(B.load().nfa_grid_rebinarize_scratch_bytes())
    assert n_bytes % 8 == 0 and n_bytes > 16
    binaries = torch.full((levels, *res), 2, dtype=torch.uint8, device=dev)
    bits = torch.full((R.walk_bits_words(levels, res) + 1,), -1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(n_bytes // 8, dtype=torch.float64, device=dev)
    B.call("nfa_grid_rebinarize", B.ptr(occs), levels, _res(res), float(occ_thre), B.ptr(binaries), B.ptr(bits), B.ptr(scratch),
           B.stream())
    assert int(bits[-1]) == -1
    tm = scratch.view(torch.float32)[(n_bytes - 16) // 4:(n_bytes - 16) // 4 + 2].cpu().numpy()
    return binaries, bits[:-1], tm[0], tm[1]


def _same_bits_or_nan(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def exact_occs(levels, res, seed):
    """Multiples of 1/1024 in [0, 1) (their float64 sum is exact in any order) with -1 in a random tenth of the cells; where
    the grid has room, cells exactly at 256/1024 and 257/1024."""
    rng = np.random.default_rng(seed)
    n = levels * res[0] * res[1] * res[2]
    occs = (rng.integers(0, 1024, n).astype(np.float32) / np.float32(1024.0)).astype(np.float32)
    occs[rng.random(n) < 0.1] = -1.0
    if n >= 8:
        occs[[1, n - 2]] = np.float32(256.0 / 1024.0)
        occs[[2, n - 3]] = np.float32(257.0 / 1024.0)
    return occs


def check_rebinarize(dev, occs, levels, res, occ_thre, exact=True):
    binaries, bits, thre, mean = dev_rebinarize(T(occs, dev), levels, res, occ_thre)
    want_thre, want_mean = R.exact_threshold(occs, occ_thre)
    print(f"rebinarize {levels} x {res} occ_thre {occ_thre}: device thre {thre!r} mean {mean!r}, reference thre {want_thre!r} mean {want_mean!r}")
    if exact:
        assert _same_bits_or_nan(thre, want_thre) and _same_bits_or_nan(mean, want_mean), (thre, mean, want_thre, want_mean)
    else:
        # any float64 summation order of <= 2^24 float32 values is within 2^-29 relative of the exact sum, far below half a
        # float32 ulp: only a rounding boundary can move the rounded mean, and then by one ulp
        assert abs(int(np.float32(mean).view(np.int32)) - int(np.float32(want_mean).view(np.int32))) <= 1, (mean, want_mean)
        assert _same_bits_or_nan(thre, min(np.float32(mean), np.float32(occ_thre)))
    with np.errstate(invalid="ignore"):
        want = (occs > np.float32(thre)).reshape(levels, *res)
    got = binaries.cpu().numpy()
    assert (got == want.astype(np.uint8)).all()                  # every cell, the threshold's own neighbours included
    assert torch.equal(bits, dev_pack_walk_bits(binaries))        # word for word
    return got, thre, mean


@pytest.mark.parametrize("levels,res", R.SHAPES)
def test_rebinarize_exact(dev, levels, res):
    occs = exact_occs(levels, res, seed=levels * 1000 + sum(res))
    n = occs.size
    for occ_thre in (0.25, 10.0):
        got, thre, mean = check_rebinarize(dev, occs, levels, res, occ_thre)
        if n >= 1000:
            assert mean > 0.25 and thre == np.float32(min(mean, occ_thre))
            if occ_thre == 0.25:      # below the mean: a cell exactly at the threshold is not occupied, the next float up is
                assert not got.reshape(-1)[1] and not got.reshape(-1)[n - 2] and got.reshape(-1)[2] and got.reshape(-1)[n - 3]


def test_rebinarize_exact_large(dev):
    levels, res = R.LARGE
    occs = exact_occs(levels, res, seed=99)
    for occ_thre in (0.25, 10.0):
        got, thre, mean = check_rebinarize(dev, occs, levels, res, occ_thre)
        assert mean > 0.25 and thre == np.float32(min(mean, occ_thre))
        if occ_thre == 0.25:
            assert not got.reshape(-1)[1] and got.reshape(-1)[2]


@pytest.mark.parametrize("levels,res", [(2, (7, 1, 9)), (2, (16, 12, 20)), (1, (3, 512, 2))])
def test_rebinarize_special_values(dev, levels, res):
    n = levels * res[0] * res[1] * res[2]
    for occ_thre in (0.25, 10.0):
        # all cells marked invisible: a NaN threshold, nothing occupied
        got, thre, mean = check_rebinarize(dev, np.full(n, -1.0, np.float32), levels, res, occ_thre)
        assert np.isnan(thre) and np.isnan(mean) and not got.any()
        # a single non-negative cell
        occs = np.full(n, -1.0, np.float32)
        occs[n // 2] = 0.5
        got, thre, mean = check_rebinarize(dev, occs, levels, res, occ_thre)
        assert mean == 0.5 and int(got.sum()) == (1 if occ_thre == 0.25 else 0)
        # NaN (never >= 0: left out of the mean, never occupied) and +inf entries
        occs = exact_occs(levels, res, seed=8)
        occs[[0, n - 1]] = np.nan
        occs[3] = _neg(np.nan)
        got, thre, mean = check_rebinarize(dev, occs, levels, res, occ_thre)
        assert np.isfinite(mean) and not got.reshape(-1)[[0, 3, n - 1]].any()
        occs[5] = np.inf
        got, thre, mean = check_rebinarize(dev, occs, levels, res, occ_thre)
        assert mean == np.inf and thre == np.float32(occ_thre) and got.reshape(-1)[5]


@pytest.mark.parametrize("levels,res", [(2, (16, 12, 20)), R.LARGE])
def test_rebinarize_random_floats(dev, levels, res):
    rng = np.random.default_rng(17)
    n = levels * res[0] * res[1] * res[2]
    assert n <= 1 << 24
    occs = rng.random(n, dtype=np.float32)
    occs[rng.random(n) < 0.1] = -1.0
    for occ_thre in (0.25, 10.0):
        check_rebinarize(dev, occs, levels, res, occ_thre, exact=False)


# ----------------------------------------------------------------------------- c. EMA update and cell positions
STORED_SPECIALS = np.array([-1.0, 0.0, 1e-45, 1e-39, np.inf, np.nan, _neg(np.nan), 0.5, -0.475], np.float32)
CAND_SPECIALS = np.array([0.0, -0.0, -0.475, -1.0, -1e-45, np.inf, -np.inf, np.nan, _neg(np.nan), 1.0, 0.5], np.float32)


def duplicated_indices(rng, n, n_cells):
    """n cell ids of [0, n_cells), every one of them listed 1 to 8 times, in random order."""
    n_distinct = min(n_cells, max(1, n // 4))
    cells = rng.choice(n_cells, n_distinct, replace=False) if n_cells <= (1 << 20) else np.unique(rng.integers(0, n_cells, n_distinct))
    reps = rng.integers(1, 9, cells.size)
    idx = np.repeat(cells, reps)
    while idx.size < n:                                           # (few cells: fill up without passing 8 per cell)
        more = cells[reps < 8][: n - idx.size]
        if more.size == 0:
            break
        reps[np.isin(cells, more)] += 1
        idx = np.concatenate([idx, more])
    idx = rng.permutation(idx)[:n]
    assert idx.size == n and np.bincount(idx).max() <= 8
    return idx.astype(np.int64)


def ema_case(n, levels, res, lvl, seed):
    rng = np.random.default_rng(seed)
    cells = res[0] * res[1] * res[2]
    idx = duplicated_indices(rng, n, cells)
    occs = (rng.random(levels * cells, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    touched = np.unique(idx)
    pick = rng.random(touched.size) < 0.5
    occs[lvl * cells + touched[pick]] = rng.choice(STORED_SPECIALS, int(pick.sum()))
    occ = (rng.random(n, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    pick = rng.random(n) < 0.4
    occ[pick] = rng.choice(CAND_SPECIALS, int(pick.sum()))
    if n >= 4:
        occ[:4] = CAND_SPECIALS[[1, 2, 7, 8]]                     # -0.0, a negative value, the two NaNs: always present
    return occs, idx, occ


EMA_CASES = [(1, 2, (7, 1, 9)), (255, 2, (7, 1, 9)), (257, 2, (7, 1, 9)), (257, 2, (16, 12, 20)), ((1 << 20) + 777, *R.LARGE)]


@pytest.mark.parametrize("n,levels,res", EMA_CASES)
def test_ema_update_bit_for_bit(dev, oracle, n, levels, res):
    lvl, cells = 1, res[0] * res[1] * res[2]
    occs, idx, occ = ema_case(n, levels, res, lvl, seed=n)
    for decay in (0.95, 1.0, 0.0):
        with np.errstate(invalid="ignore"):
            want = oracle.grid_ema_update(occs, lvl * cells + idx, occ, decay)
        runs = []
        d_idx, d_occ = T(idx, dev), T(occ, dev)
        for _ in range(2):
            d_occs, scratch = T(occs, dev).clone(), torch.empty(n, dtype=torch.float32, device=dev)
            B.call("nfa_grid_ema_update", B.ptr(d_occs), lvl * cells, B.ptr(d_idx), n, B.ptr(d_occ), float(decay),
                   B.ptr(scratch), B.stream())
            runs.append(d_occs.cpu().numpy())
        assert runs[0].tobytes() == runs[1].tobytes(), decay      # the same bytes whatever order the atomics took
        assert _same_floats(runs[0], want), (decay, int((~((runs[0] == want) | (np.isnan(runs[0]) & np.isnan(want)))).sum()))
        untouched = np.ones(occs.size, bool)
        untouched[lvl * cells + idx] = False
        assert runs[0][untouched].tobytes() == occs[untouched].tobytes()
        assert (runs[0][np.isnan(runs[0])].view(np.uint32) == 0x7FC00000).all()   # (the untouched cells hold no NaN)


def test_ema_update_written_nans_are_canonical(dev):
    """What the update stores for a NaN is the one positive-sign pattern a later atomic max leaves alone."""
    occs = np.array([0.5, _neg(np.nan), np.inf, 0.25, -1.0], np.float32)
    idx = np.array([0, 0, 1, 2, 3, 3, 4, 4], np.int64)
    occ = np.array([_neg(np.nan), 1.0, 0.5, 0.0, 1.0, _neg(np.nan), -0.0, -0.5], np.float32)
    for decay, want in ((1.0, [np.nan, np.nan, np.inf, np.nan, 0.0]), (0.0, [np.nan, np.nan, np.nan, np.nan, 0.0])):
        d_occs, d_idx, d_occ, scratch = T(occs, dev).clone(), T(idx, dev), T(occ, dev), torch.empty(8, dtype=torch.float32, device=dev)
        B.call("nfa_grid_ema_update", B.ptr(d_occs), 0, B.ptr(d_idx), 8, B.ptr(d_occ), decay, B.ptr(scratch), B.stream())
        got = d_occs.cpu().numpy()
        assert _same_floats(got, np.array(want, np.float32)), (decay, got)
        assert (got[np.isnan(got)].view(np.uint32) == 0x7FC00000).all(), (decay, got.view(np.uint32))


CELL_CASES = [(1, 2, (7, 1, 9)), (255, 3, (2, 3, 5)), (257, 2, (16, 12, 20)), ((1 << 20) + 777, *R.LARGE)]


@pytest.mark.parametrize("n,levels,res", CELL_CASES)
def test_cell_points_bit_for_bit(dev, oracle, n, levels, res):
    rng = np.random.default_rng(n + 1)
    lvl, cells = 1, res[0] * res[1] * res[2]
    idx = rng.integers(0, cells, n).astype(np.int64)
    jit = rng.random((n, 3), dtype=np.float32)
    idx[0] = cells - 1                                            # the last cell, with the largest jitter below 1
    jit[0] = np.nextafter(np.float32(1.0), np.float32(0.0))
    if n > 2:
        idx[1], idx[2] = 0, cells - 1                             # cell 0 and the last cell, jitter exactly 0
        jit[1] = jit[2] = 0.0
        jit[n // 2] = [0.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.0]
    # an asymmetric box per level whose extents are no powers of two; the kernel gets the level's six floats by pointer
    aabbs = np.stack([np.array([-1.3, -0.7, 0.1, 2.9, 0.55, 3.7], np.float32) * np.float32(1.0 + 0.37 * k) for k in range(levels)])
    d_aabbs = T(aabbs, dev)
    want = oracle.grid_cell_points(idx, jit, res, aabbs[lvl])
    runs = []
    d_idx, d_jit = T(idx, dev), T(jit, dev)
    for _ in range(2):
        x = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        B.call("nfa_grid_cell_points", B.ptr(d_idx), B.ptr(d_jit), n, _res(res), d_aabbs.data_ptr() + 24 * lvl, B.ptr(x),
               B.stream())
        runs.append(x.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()
    assert runs[0].tobytes() == want.tobytes()


# ----------------------------------------------------------------------------- d. thin and over-wide grids
THIN_CASES = R.THIN + [(3, (1, 1, 1))]
_REFS = {}


def thin_reference(oracle, levels, res, cone):
    """The oracle's traversals of a THIN case, computed once per case: the API form (default planes) and the sampler's form
    (near 0, far 1e10)."""
    key = (levels, tuple(res), cone)
    if key not in _REFS:
        o, d = R.thin_rays()
        b, ab = R.thin_grid(levels, res), R.level_aabbs(levels)
        api = oracle.traverse_grids(o, d, b, ab, step_size=0.01, cone_angle=cone)
        near, far = np.zeros(o.shape[0], np.float32), np.full(o.shape[0], 1e10, np.float32)
        smp = oracle.traverse_grids(o, d, b, ab, near_planes=near, far_planes=far, step_size=0.01, cone_angle=cone)
        _REFS[key] = (o, d, b, ab, api, smp)
    return _REFS[key]


def _cmp_traversal(res, ref):
    iv, sm, term = res
    riv, rsm, rterm = ref
    assert (iv.packed_info.cpu().numpy() == riv["packed_info"]).all(), "interval packed_info"
    assert (sm.packed_info.cpu().numpy() == rsm["packed_info"]).all(), "sample packed_info"
    assert (iv.vals.cpu().numpy() == riv["vals"]).all(), "interval vals (bit-exact)"
    assert (iv.is_left.cpu().numpy() == riv["is_left"]).all() and (iv.is_right.cpu().numpy() == riv["is_right"]).all()
    assert (iv.ray_indices.cpu().numpy() == riv["ray_indices"]).all()
    assert (sm.vals.cpu().numpy() == rsm["vals"]).all() and (sm.ray_indices.cpu().numpy() == rsm["ray_indices"]).all()
    assert (sm.is_valid.cpu().numpy() == rsm["is_valid"]).all()
    assert (term.cpu().numpy() == rterm).all(), "terminate planes"


@pytest.mark.parametrize("cone", [0.0, 0.004])
@pytest.mark.parametrize("levels,res", THIN_CASES)
def test_thin_grid_traversal_bit_exact(dev, oracle, levels, res, cone):
    o, d, b, ab, api, smp = thin_reference(oracle, levels, res, cone)
    assert na.grid._walk_supported(T(b, dev)) == (max(res) <= 512)
    got = na.traverse_grids(T(o, dev), T(d, dev), T(b, dev), T(ab, dev), step_size=0.01, cone_angle=cone)
    _cmp_traversal(got, api)
    assert got[1].vals.numel() >= 5000
    riv, rsm, _ = smp
    left, right = riv["vals"][riv["is_left"]], riv["vals"][riv["is_right"]]
    n = o.shape[0]
    near, far = torch.zeros(n, device=dev), torch.full((n,), 1e10, device=dev)
    for near_hint in (0.0, None):
        ri, ts, te, pi = na.grid._traverse_samples(T(o, dev), T(d, dev), T(b, dev), T(ab, dev), near, far, 0.01, cone,
                                                   near_hint=near_hint)
        assert (ri.cpu().numpy() == rsm["ray_indices"]).all(), near_hint
        assert (ts.cpu().numpy() == left).all() and (te.cpu().numpy() == right).all(), near_hint
        assert (pi.cpu().numpy() == rsm["packed_info"]).all(), near_hint


@pytest.mark.parametrize("levels,res", THIN_CASES)
def test_thin_grid_estimator_update(dev, oracle, levels, res):
    """One OccGridEstimator._update (warm-up step: every cell) on a thin grid: occupancies as the oracle's, binaries against
    the device's own threshold on every cell, and sampling through the grid copy the update left behind."""
    torch.manual_seed(levels * 100 + sum(res))
    est = na.OccGridEstimator(roi_aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=list(res), levels=levels).to(dev)
    ab = est.aabbs.cpu().numpy()
    assert (ab == R.level_aabbs(levels)).all()
    rng = np.random.default_rng(23)
    est.occs = T((rng.random(est.occs.numel(), dtype=np.float32) * np.float32(0.05)).astype(np.float32), dev)
    field = lambda p: torch.exp(-4.0 * (p.norm(dim=-1, keepdim=True) - 0.7) ** 2) * 0.05
    seen_x, seen_idx = [], []
    orig = est._get_all_cells
    def wrapped(*a, **k):
        r = orig(*a, **k); seen_idx.append([t.cpu().numpy() for t in r]); return r
    est._get_all_cells = wrapped
    def occ_eval(p):
        seen_x.append(p.cpu().numpy()); return field(p)
    before = est.occs.cpu().numpy().copy()
    est._update(0, occ_eval, occ_thre=0.02, ema_decay=0.9, warmup_steps=256)
    est._get_all_cells = orig
    assert len(seen_idx) == 1 and len(seen_idx[0]) == levels == len(seen_x)
    exp = before
    for lvl, (ids, px) in enumerate(zip(seen_idx[0], seen_x)):
        assert np.array_equal(np.sort(ids), np.arange(est.cells_per_lvl)) and px.shape == (ids.size, 3)
        lo, hi = ab[lvl, :3], ab[lvl, 3:]
        assert (px >= lo).all() and (px <= hi).all()
        occ = field(T(px, dev)).squeeze(-1).cpu().numpy()
        exp = oracle.grid_ema_update(exp, lvl * est.cells_per_lvl + ids, occ, 0.9)
    occs = est.occs.cpu().numpy()
    assert (occs == exp).all()
    if max(res) <= 512:
        assert getattr(est.binaries, "_nfa_walk_bits", None) is not None
        binaries, bits, thre, mean = dev_rebinarize(est.occs, levels, res, 0.02)
        assert torch.equal(est.binaries.view(torch.uint8), binaries) and torch.equal(est.binaries._nfa_walk_bits[1], bits)
        want_thre, _ = R.exact_threshold(occs, 0.02)
        assert abs(int(np.float32(thre).view(np.int32)) - int(np.float32(want_thre).view(np.int32))) <= 1
    else:     # beyond the walk: the reference's expression on the device
        thre = torch.clamp(est.occs[est.occs >= 0].mean(), max=0.02).cpu().numpy()
        assert abs(float(thre) - float(R.exact_threshold(occs, 0.02)[0])) <= 1e-6 * float(thre)
    assert est.binaries.dtype == torch.bool and (est.binaries.cpu().numpy() == (occs > np.float32(thre)).reshape(levels, *res)).all()
    o, d = R.thin_rays()
    for cone in (0.0, 0.004):
        got = est.sampling(T(o, dev), T(d, dev), render_step_size=0.01, cone_angle=cone)
        ori, ots, ote = oracle.occgrid_sampling(o, d, est.binaries.cpu().numpy(), ab, render_step_size=0.01, cone_angle=cone)
        assert (got[0].cpu().numpy() == ori).all() and (got[1].cpu().numpy() == ots).all() and (got[2].cpu().numpy() == ote).all()
