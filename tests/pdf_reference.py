"""Float64 restatements of csrc/pdf.hip (inverse-CDF resampling, per-ray searchsorted, the interlevel loss) in plain
numpy, and generators of rows on which the float32 kernels are EXACT, for tests/test_pdf_variants_gpu.py.

Nothing from nerfacc_amd or the oracle is used here.  ``tests/test_pdf_reference_cpu.py`` checks these functions against
the C oracle and against a per-ray, per-sample Python loop.

Why ``exact_rows`` makes every float32 operation of the resampling exact (so that a float64 restatement gives the same
number and a test can ask for equality).  With the unit q = 2^-7, a row's CDF is ``(c0 + cumsum(steps)) * q`` with integer
steps that add up to 2 S units, each non-zero step a power of two, and its values are integers / 256 in [0, 1].  With
bias = 0.5 (not stratified):

* ``u_ceil - u_floor`` = 2 S q: a difference of multiples of q below 2^10 q.  Exact.
* ``u_step = (u_ceil - u_floor) / S`` = 2 q: the quotient is representable, and IEEE division returns it.
* ``sid + bias`` = sid + 1/2, ``(sid + bias) * u_step`` = (2 sid + 1) q, ``u = u_floor + ...`` = (c0 + 2 sid + 1) q: small
  integers times a power of two.  Exact.  Sample ``sid`` therefore sits on the ODD unit c0 + 2 sid + 1, and every CDF entry
  on an odd unit is hit exactly by one sample (the comparison ``data[mid] > u`` then decides between two brackets that are
  an empty region apart).
* ``du = u_upper - u_lower``: one step, a power of two 2^k q (k <= 8), or zero on a tie.
* ``t_upper - t_lower`` = n / 256 with an integer n in [0, 256]; ``/ du`` divides by a power of two.  Exact.
* ``u - u_lower`` = m q with an integer m < 2^k; ``(u - u_lower) * scaling`` = m n / 2^(k + 8) with m n < 2^17.  Exact.
* ``+ t_lower``: a multiple of 2^-(k + 8) >= 2^-16 in [0, 1]: at most 17 significant bits.  Exact.
* a tie takes ``(t_lower + t_upper) * 0.5``: integers / 512.  Exact.
* the edges: ``(t + t_prev) * 0.5`` is a multiple of 2^-17 below 1 (exact); ``t -/+ (t' - t) * 0.5`` is a multiple of 2^-17
  of magnitude below 1.5 (18 bits, exact); ``fmaxf`` / ``fminf`` pick one of two exact numbers.

Error scales for float32 kernels on inputs where the arithmetic is not exact are derived where they are used.
"""
from __future__ import annotations

import numpy as np

Q_UNIT = 2.0 ** -7
FLAT32 = float(np.float32(1e-10))      # the kernels' "flat CDF step" threshold, as float32 holds it
U32 = 2.0 ** -24                       # float32 unit roundoff (round to nearest)


# ----------------------------------------------------------------------------- inputs
def _pow2_composition(rng, n_units: int, k: int):
    """n_units as a sum of exactly k powers of two (popcount(n_units) <= k <= n_units), in random order."""
    parts = [1 << b for b in range(n_units.bit_length()) if (n_units >> b) & 1]
    assert len(parts) <= k <= n_units
    while len(parts) < k:
        big = [i for i, p in enumerate(parts) if p > 1]
        i = big[int(rng.integers(len(big)))]
        parts[i] >>= 1
        parts.append(parts[i])
    return [parts[i] for i in rng.permutation(len(parts))]


def exact_rows(rng, R: int, E: int, S, lead_ties: bool = True, saturated_tail: bool = True, tied_vals: bool = True,
               flat_rows: bool = True):
    """(vals, cdfs, info): R float32 rows of E entries on which resampling to S samples (an int, or one count per ray; a count
    of 0 is laid out as 1) with bias 0.5 is exact in float32 -- see the module docstring.

    Of a row's E - 1 CDF steps, k are the powers of two of a random composition of 2 S units and the others are zero
    (ties); k is uniform over its possible range popcount(2 S) .. min(E - 1, 2 S), so ties are frequent and steps of one
    unit, which put a CDF entry on a sample's odd unit, occur at every size.
    ``lead_ties``: about a third of the rows put a run of their zero steps first (u_floor is repeated).
    ``saturated_tail``: about a third put at least two zero steps last (the CDF reaches its maximum 3 or more entries
    before the row ends), whenever the row has two zero steps to spare; row 1 always does.
    ``flat_rows``: row 0, and further rows at random (one in eight; 45 % when E <= 2, where nothing else can tie),
    are wholly flat, cdf[0] == cdf[-1].
    ``tied_vals``: the values are drawn with repeats (sorted integers in [0, 256] / 256); otherwise without, which needs
    E <= 257.
    ``info``: dict of the boolean row masks ``flat``, ``tail`` (a trailing run of 3 or more equal entries), ``lead``."""
    S_ray = np.broadcast_to(np.maximum(np.asarray(S, np.int64), 1), (R,))
    cdfs = np.zeros((R, E), np.float64)
    flat = np.zeros(R, bool)
    lead = np.zeros(R, bool)
    p_flat = 0.45 if E <= 2 else 0.125
    for r in range(R):
        c0 = int(rng.integers(0, 3))
        n_units = 2 * int(S_ray[r])
        steps = np.zeros(max(E - 1, 0), np.int64)
        kind = rng.random(3)
        flat[r] = E == 1 or (flat_rows and (r == 0 or kind[0] < p_flat))
        if not flat[r]:
            k_min, k_max = bin(n_units).count("1"), min(E - 1, n_units)
            assert k_min <= k_max, f"2 S = {n_units} units have no composition into {E - 1} power-of-two steps"
            k_hi = k_max
            if saturated_tail and r == 1 and k_min <= E - 3:
                k_hi = min(k_hi, E - 3)     # row 1 keeps two zero steps for its tail
            k = int(rng.integers(k_min, k_hi + 1))
            parts = _pow2_composition(rng, n_units, k)
            n_zero = E - 1 - k
            z_tail = 0
            if saturated_tail and n_zero >= 2 and (r == 1 or kind[1] < 1.0 / 3.0):
                z_tail = int(rng.integers(2, n_zero + 1))
            z_lead = 0
            if lead_ties and n_zero - z_tail >= 1 and kind[2] < 1.0 / 3.0:
                z_lead = int(rng.integers(1, n_zero - z_tail + 1))
                lead[r] = True
            mid = np.zeros(E - 1 - z_lead - z_tail, np.int64)
            mid[rng.choice(mid.size, k, replace=False)] = parts
            # (the first and the last entry of `mid` may still be zero: runs can be longer than asked for)
            steps[z_lead:E - 1 - z_tail] = mid
        cdfs[r] = (c0 + np.concatenate([[0], np.cumsum(steps)])) * Q_UNIT
    if tied_vals:
        ints = np.sort(rng.integers(0, 257, (R, E)), -1)
    else:
        ints = np.stack([np.sort(rng.choice(257, E, replace=False)) for _ in range(R)])
    vals = ints / 256.0
    tail = (cdfs[:, max(E - 3, 0)] == cdfs[:, -1]) if E >= 3 else np.zeros(R, bool)
    out_v, out_c = vals.astype(np.float32), cdfs.astype(np.float32)
    assert np.array_equal(out_v.astype(np.float64), vals) and np.array_equal(out_c.astype(np.float64), cdfs)
    return out_v, out_c, dict(flat=flat, tail=tail, lead=lead)


def value_rows(rng, R: int, n: int, keys=None, p_shared: float = 0.5):
    """(R, n) float32 rows of sorted edge values as a proposal level has them: the first entry is exactly 0 and the last
    exactly 1 (n == 1: a single 0 or 1).  Without ``keys`` the interior entries are integers in [0, 256] / 256, with
    repeats.  With ``keys`` (R, K) an interior entry is, with probability ``p_shared``, a copy of a random entry of the
    ray's key row, and otherwise an integer in [0, 512] / 512 (which is a key value only by chance)."""
    if n == 1:
        pick = rng.integers(0, 2, (R, 1)).astype(np.float64)
        if keys is not None:
            j = rng.integers(0, keys.shape[1], (R, 1))
            own = np.take_along_axis(np.asarray(keys, np.float64), j, -1)
            pick = np.where(rng.random((R, 1)) < p_shared, own, pick)
        return pick.astype(np.float32)
    if keys is None:
        v = rng.integers(0, 257, (R, n)) / 256.0
    else:
        v = rng.integers(0, 513, (R, n)) / 512.0
        j = rng.integers(0, keys.shape[1], (R, n))
        v = np.where(rng.random((R, n)) < p_shared, np.take_along_axis(np.asarray(keys, np.float64), j, -1), v)
    v = np.sort(v, -1)
    v[:, 0], v[:, -1] = 0.0, 1.0
    return v.astype(np.float32)


def loss_rows(rng, R: int, Q1: int, K1: int, p_tie: float = 0.4, key_scale: float = 0.25):
    """(q_vals, q_cdfs, k_vals, k_cdfs) float32 rows for the interlevel loss on which w, w_outer and w - w_outer are exact.

    Values: ``value_rows`` -- key and query rows share 0, 1 and about a third of the query's interior entries.
    CDFs: dyadic with ties.  A query step is 0 with probability ``p_tie`` and otherwise 1..8 units of 2^-13 (at most
    8 * 1023 < 2^13 units: the row stays below 1, 13 bits).  The key row spreads the SAME number of units over its steps,
    about ``p_tie`` of them (and any step the multinomial draw leaves empty) zero, and is then scaled by ``key_scale`` = 1/4,
    so that the key's mass around a query interval is below the interval's own on a good share of intervals.  Every CDF
    entry is a multiple of 2^-15 below 1: differences, and differences of differences, are exact in float32."""
    unit = 2.0 ** -13
    kv = value_rows(rng, R, K1)
    qv = value_rows(rng, R, Q1, keys=kv, p_shared=1.0 / 3.0)
    q_steps = rng.integers(1, 9, (R, Q1 - 1)) * (rng.random((R, Q1 - 1)) >= p_tie)
    qc = np.concatenate([np.zeros((R, 1)), np.cumsum(q_steps, -1)], -1) * unit
    kc = np.zeros((R, K1))
    for r in range(R):
        total = int(q_steps[r].sum())
        if K1 > 1:
            live = rng.random(K1 - 1) >= p_tie
            if not live.any():
                live[int(rng.integers(K1 - 1))] = True
            steps = np.zeros(K1 - 1, np.int64)
            steps[live] = rng.multinomial(total, np.full(int(live.sum()), 1.0 / live.sum()))
            kc[r, 1:] = np.cumsum(steps)
    kc = kc * unit * key_scale
    out = [a.astype(np.float32) for a in (qv, qc, kv, kc)]
    assert np.array_equal(out[1].astype(np.float64), qc) and np.array_equal(out[3].astype(np.float64), kc)
    return tuple(out)


# ----------------------------------------------------------------------------- the bracket
def upper_bound64(row, x):
    """For each x: the first index i in [0, len(row) - 1) with row[i] > x, or len(row) - 1 if there is none -- the
    kernels' ``upper_bound(data, first, last, x)``, whose range excludes the row's last entry."""
    return np.searchsorted(np.asarray(row)[:-1], x, side="right")


def _bracket_rows(rows, x):
    """Batched ``upper_bound`` + clamped bracket: rows (R, E), x (R, N) -> (lower, upper) indices (R, N)."""
    E = rows.shape[1]
    p = (rows[:, None, :E - 1] <= x[:, :, None]).sum(-1) if E > 1 else np.zeros(x.shape, np.int64)
    # rows are sorted, so the count of entries <= x among the first E - 1 is the first index whose entry is > x
    return np.clip(p - 1, 0, E - 1), np.clip(p, 0, E - 1)


def inverse_cdf64(vals, cdfs, u):
    """G(u) of batched rows: vals, cdfs (R, E), u (R, N).  The entries around ``upper_bound(cdfs, u)`` clamped to the row;
    linear in between; the midpoint of the two values when the CDF step is flat (below 1e-10).  Non-decreasing in u."""
    vals, cdfs, u = (np.asarray(a, np.float64) for a in (vals, cdfs, u))
    lo, hi = _bracket_rows(cdfs, u)
    ul, uh = np.take_along_axis(cdfs, lo, -1), np.take_along_axis(cdfs, hi, -1)
    tl, th = np.take_along_axis(vals, lo, -1), np.take_along_axis(vals, hi, -1)
    du = uh - ul
    flat = du < FLAT32
    return np.where(flat, (tl + th) * 0.5, (u - ul) * ((th - tl) / np.where(flat, 1.0, du)) + tl)


def sample_positions64(cdfs, S: int, bias):
    """u (R, S) of the S samples of each row: u_floor + (sid + bias) * (u_ceil - u_floor) / S; bias a scalar or (R,)."""
    cdfs = np.asarray(cdfs, np.float64)
    bias = np.broadcast_to(np.asarray(bias, np.float64), cdfs.shape[:1])
    step = (cdfs[:, -1] - cdfs[:, 0]) / S
    return cdfs[:, :1] + (np.arange(S)[None, :] + bias[:, None]) * step[:, None]


def edges64(samples, t_min, t_max):
    """The S + 1 interval edges of (R, S) samples: midpoints between neighbours; the outer two mirror the first / last
    half-width and are clipped to the ray's range [t_min, t_max].  S == 1: the ray's whole range."""
    t = np.asarray(samples, np.float64)
    t_min, t_max = np.asarray(t_min, np.float64), np.asarray(t_max, np.float64)
    R, S = t.shape
    e = np.empty((R, S + 1))
    if S == 1:
        e[:, 0], e[:, 1] = t_min, t_max
        return e
    e[:, 1:S] = (t[:, 1:] + t[:, :-1]) * 0.5
    e[:, 0] = np.maximum(t[:, 0] - (t[:, 1] - t[:, 0]) * 0.5, t_min)
    e[:, S] = np.minimum(t[:, -1] + (t[:, -1] - t[:, -2]) * 0.5, t_max)
    return e


def importance_sampling64(vals, cdfs, S, bias=0.5, packed_info=None):
    """Inverse-CDF resampling as csrc/pdf.hip defines it, in float64.

    Input rows are batched, ``vals`` / ``cdfs`` (R, E), or packed: flat arrays and ``packed_info`` (R, 2) = (start, count).
    ``bias`` is a scalar or one value per ray.
    ``S`` an int: returns ``(samples (R, S), edges (R, S + 1))``.
    ``S`` an (R,) array of per-ray counts: returns two dicts of PACKED outputs, ``samples`` with ``vals``, ``packed_info``,
    ``ray_indices`` and ``edges`` with those and ``is_left`` / ``is_right``; ray r has S[r] samples and S[r] + 1 edges
    (none for S[r] == 0); every edge but a ray's last is a left edge, every edge but its first a right edge."""
    vals, cdfs = np.asarray(vals, np.float64), np.asarray(cdfs, np.float64)
    per_ray = np.ndim(S) > 0
    if packed_info is None and not per_ray:
        t = inverse_cdf64(vals, cdfs, sample_positions64(cdfs, int(S), bias))
        return t, edges64(t, vals[:, 0], vals[:, -1])
    if packed_info is None:
        rows = [(vals[r], cdfs[r]) for r in range(vals.shape[0])]
    else:
        pi = np.asarray(packed_info, np.int64)
        rows = [(vals[a:a + n], cdfs[a:a + n]) for a, n in pi]
    R = len(rows)
    counts = np.broadcast_to(np.asarray(S, np.int64), (R,))
    bias = np.broadcast_to(np.asarray(bias, np.float64), (R,))
    sm, ed = [], []
    for r, (v, c) in enumerate(rows):
        if counts[r] == 0:
            sm.append(np.zeros(0)); ed.append(np.zeros(0))
            continue
        t = inverse_cdf64(v[None], c[None], sample_positions64(c[None], int(counts[r]), bias[r:r + 1]))
        sm.append(t[0]); ed.append(edges64(t, v[0], v[-1])[0])
    if not per_ray:
        return np.stack(sm), np.stack(ed)
    n_ed = (counts + 1) * (counts > 0)
    ids = np.arange(R)
    left = [np.arange(n) < n - 1 for n in n_ed]
    right = [np.arange(n) > 0 for n in n_ed]
    samples = dict(vals=np.concatenate(sm), packed_info=np.stack([np.cumsum(counts) - counts, counts], -1),
                   ray_indices=np.repeat(ids, counts))
    edges = dict(vals=np.concatenate(ed), packed_info=np.stack([np.cumsum(n_ed) - n_ed, n_ed], -1),
                 ray_indices=np.repeat(ids, n_ed), is_left=np.concatenate(left).astype(bool),
                 is_right=np.concatenate(right).astype(bool))
    return samples, edges


# ----------------------------------------------------------------------------- searchsorted, s -> t
def searchsorted64(keys, queries):
    """Ray-relative ``(left, right)`` ids of batched rows, keys (R, K) and queries (R, Q): with p = upper_bound over the
    key row without its last entry, left = clamp(p - 1) and right = clamp(p), both to [0, K - 1]."""
    return _bracket_rows(np.asarray(keys, np.float64), np.asarray(queries, np.float64))


def stot64(kind: str, s, t_min: float, t_max: float):
    """uniform: t = s t_max + (1 - s) t_min;  lindisp: t = 1 / (s / t_max + (1 - s) / t_min)."""
    s = np.asarray(s, np.float64)
    if kind == "uniform":
        return s * t_max + (1.0 - s) * t_min
    if kind == "lindisp":
        return 1.0 / (s * (1.0 / t_max) + (1.0 - s) * (1.0 / t_min))
    raise ValueError(kind)


# ----------------------------------------------------------------------------- the interlevel loss
def pdf_loss64(qv, qc, kv, kc, eps: float, g):
    """The interlevel loss of batched rows and its gradients for an incoming gradient g (R, Q1 - 1), float64:

        l_j = max(w_j - wo_j, 0)^2 / (w_j + eps),  w_j = qc[j + 1] - qc[j],  wo_j = kc[right_j] - kc[left_j],
        left_j = left id of qv[j],  right_j = right id of qv[j + 1]   (``searchsorted64``)
        where d_j = w_j - wo_j > 0:  d l_j / d wo_j = -2 d / (w + eps),  d l_j / d w_j = 2 d / (w + eps) - d^2 / (w + eps)^2

    The gradients are scatter-adds: g_kc[right_j] += gwo_j, g_kc[left_j] -= gwo_j, g_qc[j + 1] += gw_j, g_qc[j] -= gw_j.
    Returns a dict: ``loss``, ``left``, ``right``, ``w``, ``wo``, ``g_kc``, ``g_qc``; ``abs_kc`` / ``abs_qc``, per output element
    the sum of the magnitudes added to it (for g_qc a term's magnitude is (2 d / (w + eps) + d^2 / (w + eps)^2) |g|, the
    size of what its difference is formed from); ``n_kc`` / ``n_qc``, the number of terms added to each element."""
    qv, qc, kv, kc, g = (np.asarray(a, np.float64) for a in (qv, qc, kv, kc, g))
    il, ir = searchsorted64(kv, qv)
    left, right = il[:, :-1], ir[:, 1:]
    w = qc[:, 1:] - qc[:, :-1]
    wo = np.take_along_axis(kc, right, -1) - np.take_along_axis(kc, left, -1)
    d = np.maximum(w - wo, 0.0)
    inv = 1.0 / (w + eps)
    loss = d * d * inv
    live = d > 0
    gwo = np.where(live, -2.0 * d * inv * g, 0.0)
    gw = np.where(live, (2.0 * d * inv - d * d * inv * inv) * g, 0.0)
    gw_abs = np.where(live, (2.0 * d * inv + d * d * inv * inv) * np.abs(g), 0.0)
    rows = np.broadcast_to(np.arange(qv.shape[0])[:, None], left.shape)
    j = np.broadcast_to(np.arange(left.shape[1])[None, :], left.shape)
    out = dict(loss=loss, left=left, right=right, w=w, wo=wo)
    for name, shape, hi, lo, term, mag in (("kc", kc.shape, right, left, gwo, np.abs(gwo)), ("qc", qc.shape, j + 1, j, gw, gw_abs)):
        grad, mags, n = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        np.add.at(grad, (rows, hi), term)
        np.add.at(grad, (rows, lo), -term)
        for idx in (hi, lo):
            np.add.at(mags, (rows, idx), mag)
            np.add.at(n, (rows, idx), live.astype(np.float64))
        out["g_" + name], out["abs_" + name], out["n_" + name] = grad, mags, n
    return out


# ----------------------------------------------------------------------------- float32 error bounds
# The loss on ``loss_rows``: w, wo and d = w - wo are exact, so l = fl(fl(d d) / fl(w + eps)) carries three roundings.
LOSS_ROUNDINGS = 3
# gwo = fl(fl(fl(-2 d) inv) g) with inv = fl(1 / fl(w + eps)): w + eps, the reciprocal, two products (-2 d is exact).
GWO_ROUNDINGS = 4
# gw = fl(fl(fl(fl(2 d) inv) - fl(fl(fl(d d) inv) inv)) g): the first product carries 3 roundings (inv's two and its own),
# the second 7 (d d, and twice inv's two plus the product's); the larger of the two, the difference and the product with g
# act on a magnitude of at most (2 d inv + d^2 inv^2) |g|.
GW_ROUNDINGS = 7 + 2


def loss_bounds(ref: dict, extra: int = 0):
    """Per-element tolerances (loss, g_kc, g_qc) for float32 kernels against ``pdf_loss64`` on ``loss_rows``: the number of
    roundings counted above, times 2, times 2^-24, times the magnitude they act on.  A gradient entry that is a sum of n
    terms carries n more roundings of at most 2^-24 times the sum of the terms' magnitudes (any order of additions).
    ``extra``: further roundings of the incoming gradient (the mean form divides it by the element count: 1)."""
    return (2 * LOSS_ROUNDINGS * U32 * np.abs(ref["loss"]),
            2 * (GWO_ROUNDINGS + extra + ref["n_kc"]) * U32 * ref["abs_kc"],
            2 * (GW_ROUNDINGS + extra + ref["n_qc"]) * U32 * ref["abs_qc"])


def loss_mean_bound(ref: dict, n_partials: int):
    """Tolerance of the mean form's value: each term's three roundings (times 2), the summation -- per-lane chains and the
    wave reduction (at most 64 additions deep together), then the partial sums in any order -- bounded by
    (n_partials + 64) 2^-24 sum|l|, and the final division's one rounding."""
    total = float(np.abs(ref["loss"]).sum())
    return (n_partials + 64 + 2 * LOSS_ROUNDINGS + 1) * U32 * total / ref["loss"].size


def stratified_band(vals, cdfs, S: int, bias):
    """(lo, hi, straddles, delta, tau): a float32 kernel's sample for the float32 jitter ``bias`` lies in [lo, hi] =
    [G(u - delta) - tau, G(u + delta) + tau], G = ``inverse_cdf64`` (non-decreasing in u) and u the exact position.

    delta, the error of the float32 ``u = u_floor + (sid + bias) * u_step`` with ``u_step = (u_ceil - u_floor) / S``, for
    M = u_ceil - u_floor (itself exact on ``exact_rows``): the division rounds u_step by at most 2^-24 u_step, which moves
    u by at most 2^-24 M; ``sid + bias`` <= S rounds by at most 2^-24 S, which moves u by at most 2^-24 S u_step = 2^-24 M; the
    product is at most M and rounds by at most 2^-24 M; the sum is at most u_ceil (+ delta) and rounds by at most
    2^-24 u_ceil.  First order: delta = 2^-24 (3 M + u_ceil); the second-order terms are below 2^-45 and a factor 1 + 2^-20
    covers them.  A wholly flat row has M = 0: u_step and the product are exactly zero and u = u_floor + 0 exactly, delta = 0.

    tau, the error of ``t = (u - u_lower) * ((t_upper - t_lower) / du) + t_lower`` evaluated at the float32 u, whose bracket
    the exact comparisons of the search determine: the difference, the quotient, the product and the sum round once each.
    For u inside its bracket the first three act on a product of at most t_upper - t_lower <= v_max and the last on a
    result of at most v_max (u beyond the row's last entry by delta extrapolates by a negligible delta / du): tau =
    4 * 2^-24 v_max, again times 1 + 2^-20.  A flat step takes (t_lower + t_upper) * 0.5: one rounding of at most
    2^-24 * 2 v_max / 2, smaller.

    ``straddles``: samples whose band spans a jump of G: u - delta and u + delta fall into different brackets (inside one
    bracket G is linear and continuous) and G(u + delta) - G(u - delta) > 2 tau.  There the band is as wide as an empty
    region and says little; the tests cap the share of such samples."""
    vals, cdfs = np.asarray(vals, np.float64), np.asarray(cdfs, np.float64)
    slack = 1.0 + 2.0 ** -20
    mass = cdfs[:, -1] - cdfs[:, 0]
    delta = np.where(mass == 0.0, 0.0, U32 * (3.0 * mass + np.abs(cdfs[:, -1])) * slack)[:, None]
    tau = 4.0 * U32 * float(np.abs(vals).max()) * slack
    u = sample_positions64(cdfs, S, bias)
    g_lo, g_hi = inverse_cdf64(vals, cdfs, u - delta), inverse_cdf64(vals, cdfs, u + delta)
    other_bracket = _bracket_rows(cdfs, u - delta)[1] != _bracket_rows(cdfs, u + delta)[1]
    return g_lo - tau, g_hi + tau, other_bracket & ((g_hi - g_lo) > 2.0 * tau), delta, tau


# ----------------------------------------------------------------------------- which kernel a shape selects
IS_STAGE_MAX = 512      # csrc/pdf.hip: CDF entries a wave may stage in LDS

# (instance, S values, E values): every (S, E) of a row must select the instance named -- ``resampling_instance``
INSTANCE_TABLE = [
    ("rows<2,1>", (1, 2), (1, 2, 9)),
    ("rows<4,1>", (3, 4), (5,)),
    ("rows<8,1>", (5, 8), (9,)),
    ("rows<16,1>", (9, 16), (33,)),
    ("rows<16,2>", (17, 24, 32), (65, 128)),
    ("rows<16,4>", (33, 48, 63, 64), (65, 128)),
    ("rows<32,1>", (17, 32), (129, 200)),
    ("rows<64,1>", (33, 64), (200, 512)),
    ("general<staged>", (65, 150), (300, 512)),
    ("general<not staged>", (16, 150), (513, 700)),
]


def resampling_instance(S: int, E: int, batched: bool = True) -> str:
    """The kernel instance ``launch_importance_sampling`` (csrc/pdf.hip) picks for S samples from rows of E entries,
    restated from its host code: L = the power of two in [2, 64] covering S lanes, 64 / L rays per wave; the rows are
    staged when the input is batched and a wave's rows fit IS_STAGE_MAX; staged rows of at most 64 samples take the rows
    kernel, with 16 lanes and 2 or 4 samples per lane when S > 16 and four rows fit the stage."""
    L = 2
    while L < 64 and L < S:
        L <<= 1
    staged = batched and (64 // L) * E <= IS_STAGE_MAX
    if staged and S <= 64:
        blocks = S > 16 and 4 * E <= IS_STAGE_MAX
        return f"rows<{16 if blocks else L},{(4 if S > 32 else 2) if blocks else 1}>"
    return "general<staged>" if staged else "general<not staged>"


def rays_per_block(n_rays: int, rays_per_wave: int) -> int:
    """csrc/pdf.hip: the rays whose Philox draws one wave shares out over its lanes -- doubled up to 64 while that leaves
    at least 4096 waves."""
    rb = rays_per_wave
    while rb < 64 and n_rays // (2 * rb) >= 4096:
        rb <<= 1
    return rb


def searchsorted_staged(q_per: int, k_per: int) -> bool:
    """csrc/pdf.hip, nfa_searchsorted with batched queries and keys: the key rows of the rays that 64 consecutive queries
    touch (at most 63 / q_per + 2) are staged when they fit."""
    return (63 // q_per + 2) * k_per <= IS_STAGE_MAX


def loss_instance(Q1: int, K1: int) -> str:
    """The kernels ``pdf_loss_plan`` (csrc/pdf.hip) picks for rows of Q1 query and K1 key edges: L lanes per ray cover the
    Q1 - 1 intervals (a power of two in [2, 64]), doubled until a wave's rows fit 1024 entries; the rows kernels run when a
    lane has one interval and the wave's key rows fit 512."""
    L = 2
    while L < 64 and L < Q1 - 1:
        L <<= 1
    while L < 64 and (64 // L) * max(K1, Q1) > 1024:
        L <<= 1
    return f"rows<{L}>" if Q1 - 1 <= L and (64 // L) * K1 <= 512 else f"general, {L} lanes"


def case_rng(*key):
    """The generator of a test case: the CPU checks and the GPU tests draw the same rows from the same key."""
    return np.random.default_rng([7, *key])
