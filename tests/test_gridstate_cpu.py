"""CPU tier of the occupancy grid's device state (tests/gridstate_reference.py): the Python restatement of the walk layout
against csrc/walk_layout.h compiled on the host, the layout's properties on the shapes the GPU tier packs, a bit-level model
of gridupd.hip's atomic_max_f32 -- the rule the kernel must follow -- and the floors that make the thin-grid traversals of
the GPU tier mean something."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import gridstate_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_HARNESS = r'''
#define __host__
#define __device__
#include "walk_layout.h"
extern "C" void layout_of(const int32_t *res, uint32_t *out)
{
    const nfa::WalkLayout L = nfa::walk_layout(res);
    out[0] = L.mask[0]; out[1] = L.mask[1]; out[2] = L.mask[2]; out[3] = (uint32_t)L.bits;
}
'''
AXIS_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 20, 31, 32, 33, 50, 64, 100, 128, 129, 255, 256, 257, 511, 512]


def test_walk_layout_restatement_equals_the_header(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_HARNESS)
    so = tmp_path / "liblayout_of.so"
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "nerfacc_amd", "csrc"), str(src),
                    "-o", str(so)], check=True)
    fn = C.CDLL(str(so)).layout_of
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    fn.restype = None
    out = (C.c_uint32 * 4)()
    n = 0
    for res in itertools.product(AXIS_SIZES, repeat=3):
        fn((C.c_int32 * 3)(*res), out)
        masks, bits = R.walk_layout(res)
        assert (list(out[:3]), int(out[3])) == (masks, bits), res
        n += 1
    assert n == 25 ** 3


@pytest.mark.parametrize("levels,res", R.SHAPES + [R.BEYOND_WALK])
def test_walk_layout_properties(levels, res):
    masks, bits = R.walk_layout(res)
    assert masks[0] & masks[1] == 0 and masks[0] & masks[2] == 0 and masks[1] & masks[2] == 0
    assert all(bin(m).count("1") == int(r - 1).bit_length() for m, r in zip(masks, res))
    assert bits >= 5 and (masks[0] | masks[1] | masks[2]) < (1 << bits)
    idx = R._all_cell_bits(levels, res)
    assert idx.shape == (levels, *res)
    for lvl in range(levels):     # every cell of a level sits in the level's own 1 << bits positions
        assert (idx[lvl] >> bits == lvl).all() and ((idx[lvl] & ((1 << bits) - 1)) < (1 << bits)).all()
    assert np.unique(idx).size == idx.size                       # injective
    assert int(idx.max()) < R.walk_bits_words(levels, res) * 32
    # the torch-integer version (used on the device for the one large shape) is the same map
    assert (R.walk_bit_index_torch(levels, res, "cpu").numpy() == idx).all()
    for name in R.PATTERNS:
        b = R.pattern(name, levels, res, seed=3)
        words = R.pack_walk_bits(b)
        assert words.dtype == np.uint32 and words.shape == (R.walk_bits_words(levels, res),)
        back, pad = R.unpack_walk_bits(words, levels, res)
        assert (back == b).all() and not pad.any() and pad.size == words.size * 32 - b.size
        assert int(np.unpackbits(words.view(np.uint8)).sum()) == int(b.sum())
        bricks, coarse = R.pack_bricks(b)
        assert bricks.shape == (R.bricks_words(levels, res),) and coarse.shape == ((bricks.size + 31) // 32,)
        back, pad = R.unpack_bricks(bricks, levels, res)
        assert (back == b).all() and not pad.any()
        assert (R._bits_of_words(coarse)[:bricks.size].astype(bool) == (bricks != 0)).all()
        assert not R._bits_of_words(coarse)[bricks.size:].any()


def test_reference_packers_on_hand_made_cells():
    """The restatement itself, on cells whose bits can be written down by hand."""
    # 2 x 3 x 5: nb = (1, 2, 3); round 0: z->0, x->1, y->2; round 1: z->3, y->4; round 2: z->5
    assert R.walk_layout((2, 3, 5)) == ([0b10, 0b10100, 0b101001], 6)
    assert int(R.walk_bit_index(1, 1, 2, 4, (2, 3, 5))) == (1 << 6) | 0b10 | 0b10000 | 0b100000
    # one cell: the three positions of round 0 are consumed and unused, a level is padded to one word
    assert R.walk_layout((1, 1, 1)) == ([0, 0, 0], 5) and R.walk_bits_words(3, (1, 1, 1)) == 3
    # 512 x 1 x 3: z->0, x->1, (y: position 2 unused), z->3, x->4, x->5 ... x->11
    assert R.walk_layout((512, 1, 3)) == ([0b111111110010, 0, 0b1001], 12)
    b = np.zeros((1, 5, 4, 3), bool)
    b[0, 4, 3, 2] = True                                         # brick (1, 0, 0), cell (0, 3, 2)
    bricks, coarse = R.pack_bricks(b)
    assert bricks.tolist() == [0, 1 << ((0 << 4) | (3 << 2) | 2)] and coarse.tolist() == [0b10]
    assert R.pack_flat_bits([0, 1, 2, 255] + [0] * 29 + [7]).tolist() == [0b1110, 0b10]


# ----------------------------------------------------------------------------- atomic_max_f32
def _u(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def _f(u):
    return np.frombuffer(struct.pack("<I", u), np.float32)[0]


NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000
SPECIALS = [_u(0.0), _u(-0.0), _u(1.0), _u(-1.0), _u(0.5), _u(-0.475), _u(float("inf")), _u(float("-inf")), 0x00000001, 0x80000001,
            NAN_POS, NAN_NEG]


def _is_nan(u):
    return (u & 0x7F800000) == 0x7F800000 and (u & 0x007FFFFF) != 0


def _s32(u):
    return u - (1 << 32) if u & 0x80000000 else u


def old_model(stored, cands):
    """gridupd.hip before the fix: the stored value as the multiplication left it, a NaN candidate exchanged in as it is,
    the branch chosen by `v >= 0`."""
    for v in cands:
        if _is_nan(v):
            stored = v
        elif _f(v) >= 0:                                          # -0.0 comes here, as INT_MIN
            stored = max(_s32(stored), _s32(v)) & 0xFFFFFFFF      # atomicMax on the int view
        else:
            stored = min(stored, v)                               # atomicMin on the unsigned view
    return stored


def new_model(stored, cands):
    """The fixed rule: ema_gather_kernel stores a NaN as NAN_POS; a NaN candidate is exchanged in as NAN_POS; the branch goes
    by the sign bit."""
    if _is_nan(stored):
        stored = NAN_POS
    for v in cands:
        if _is_nan(v):
            stored = NAN_POS
        elif v >> 31 == 0:
            stored = max(_s32(stored), _s32(v)) & 0xFFFFFFFF
        else:
            stored = min(stored, v)
    return stored


def _same(a, b):
    """NaN against NaN, values by == (so -0 equals +0)."""
    a, b = _f(a), np.float32(b)
    return bool(np.isnan(a) and np.isnan(b)) or bool(a == b)


def _failures(model):
    bad = []
    for s in SPECIALS:
        for a, b in itertools.product(SPECIALS, repeat=2):
            with np.errstate(invalid="ignore"):
                want = np.maximum(np.maximum(_f(s), _f(a)), _f(b))
            r1, r2, single = model(s, [a, b]), model(s, [b, a]), model(s, [a])
            if not (_same(r1, want) and _same(r2, want) and _same(r1, _f(r2)) and _same(single, np.maximum(_f(s), _f(a)))):
                bad.append((s, a, b))
    return bad


def test_atomic_max_model_is_torch_maximum_in_every_order():
    assert _failures(new_model) == []
    # what the fixed rule leaves behind is a value a later update can start from: never a NaN other than the canonical one
    for s in SPECIALS:
        for a, b in itertools.product(SPECIALS, repeat=2):
            r = new_model(s, [a, b])
            assert not _is_nan(r) or r == NAN_POS


def test_old_atomic_max_model_fails_in_the_two_classes():
    """The defects the fix removes, so that the model above is known to be able to fail: a NaN with the sign bit set is
    overwritten by a later finite candidate, and a candidate -0.0 never replaces a stored negative value.  Nothing else."""
    bad = _failures(old_model)
    neg_nan = [c for c in bad if NAN_NEG in c]
    neg_zero = [c for c in bad if NAN_NEG not in c and _u(-0.0) in c[1:]]
    assert neg_nan and neg_zero and len(neg_nan) + len(neg_zero) == len(bad)
    assert (_u(-0.475), _u(-0.0), _u(-0.0)) in neg_zero           # maximum(-0.475, -0.0) stays -0.475
    assert (_u(0.5), NAN_NEG, _u(1.0)) in neg_nan                 # NaN then 1.0 gives 1.0


# ----------------------------------------------------------------------------- traversal floors
@pytest.mark.parametrize("cone", [0.0, 0.004])
@pytest.mark.parametrize("levels,res", R.THIN + [(3, (1, 1, 1))])
def test_thin_grid_traversals_have_samples(oracle, levels, res, cone):
    """The GPU tier compares these traversals with the oracle bit for bit; that says something only if there are samples."""
    o, d = R.thin_rays()
    _, sm, _ = oracle.traverse_grids(o, d, R.thin_grid(levels, res), R.level_aabbs(levels), step_size=0.01, cone_angle=cone)
    n, hit = sm["vals"].size, int((sm["packed_info"][:, 1] > 0).sum())
    assert n >= 5000 and hit >= 300, (n, hit)
    if tuple(res) == (1, 1, 1):
        assert R.thin_grid(levels, res).all() and n >= 1000
