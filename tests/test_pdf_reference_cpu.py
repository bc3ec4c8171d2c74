"""CPU: tests/pdf_reference.py is checked here before it judges a kernel (tests/test_pdf_variants_gpu.py).

On ``exact_rows`` the float64 restatement must EQUAL the C oracle's float32 resampling bit for bit and be representable in
float32; the inputs must really be the awkward ones (ties, flat rows, saturated tails, samples on CDF entries), asserted per
case; searchsorted and the loss are compared with the oracle on rows full of equal values; and the vectorised code is
compared with a per-ray, per-sample loop written from the operation's description."""
import numpy as np
import pytest

import pdf_reference as PR

R_CASE = 131

# the (S, E) pairs the construction was first checked on, E = 1, S = 1, and every pair of the kernel-instance table
PAIRS = [(2, 2), (2, 9), (3, 9), (4, 5), (5, 9), (8, 9), (12, 9), (16, 33), (24, 65), (32, 65), (33, 65), (48, 128), (63, 200),
         (64, 200), (64, 65), (150, 300), (2, 1), (16, 1), (1, 1), (1, 2), (1, 9)]
PAIRS += [(S, E) for _, Ss, Es in PR.INSTANCE_TABLE for S in Ss for E in Es if (S, E) not in PAIRS]

LOSS_SHAPES = [(3, 2), (3, 16), (5, 32), (9, 64), (17, 128), (33, 256), (65, 512), (66, 65), (129, 33), (4, 100), (2, 1)]


case_rng = PR.case_rng


def tie_statistics(v, c, info, S):
    """(share of tied CDF steps, flat rows, non-flat rows with a trailing run of >= 3, share of samples on a CDF entry
    among the rows that are not flat)."""
    steps = np.diff(c.astype(np.float64), axis=-1)
    tied = float((steps == 0).mean()) if steps.size else float("nan")
    u = PR.sample_positions64(c, S, 0.5)
    on_entry = (u[:, :, None] == c.astype(np.float64)[:, None, :]).any(-1)
    live = ~info["flat"]
    hit = float(on_entry[live].mean()) if live.any() else float("nan")
    return tied, int(info["flat"].sum()), int((info["tail"] & live).sum()), hit


@pytest.mark.parametrize("S,E", PAIRS)
def test_exact_rows_equal_the_oracle(oracle, S, E):
    v, c, info = PR.exact_rows(case_rng(S, E), R_CASE, E, S)
    t64, e64 = PR.importance_sampling64(v, c, S)
    if S >= 2:
        o_e, o_t = oracle.importance_sampling(v, c, S)
    else:   # the oracle's int overload refuses S = 1
        iv, sm = oracle.importance_sampling_packed(v, c, np.ones(R_CASE, np.int64))
        o_e, o_t = iv["vals"].reshape(R_CASE, 2), sm["vals"].reshape(R_CASE, 1)
    for got, want in ((t64, o_t), (e64, o_e)):
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)      # representable
        assert np.array_equal(got.astype(np.float32), want)                       # and what float32 arithmetic gives
    if S == 1:
        assert np.array_equal(e64, v[:, [0, -1]].astype(np.float64))
    tied, n_flat, n_tail, hit = tie_statistics(v, c, info, S)
    print(f"S={S} E={E}: tied steps {tied:.3f}, flat rows {n_flat}, saturated tails {n_tail}, samples on an entry {hit:.3f}")
    assert n_flat >= 1
    if E >= 2:
        assert tied >= 0.25
    if E - 1 - bin(2 * S).count("1") >= 2:      # the row has two zero steps to spare
        assert n_tail >= 1
    if E >= 3:                                  # a row with an interior entry
        assert hit >= 0.03


def loop_resample(v, c, S, bias):
    """One ray, one sample at a time, from the description: find the first entry before the last that exceeds u, take the
    entries on both sides of it (clamped to the row), interpolate, or take the midpoint where the CDF does not rise."""
    v, c = [float(x) for x in v], [float(x) for x in c]
    n = len(c)
    ts = []
    for sid in range(S):
        u = c[0] + (sid + float(bias)) * ((c[-1] - c[0]) / S)
        p = n - 1
        for i in range(n - 1):
            if c[i] > u:
                p = i
                break
        lo, hi = min(max(p - 1, 0), n - 1), min(max(p, 0), n - 1)
        du = c[hi] - c[lo]
        ts.append((v[lo] + v[hi]) * 0.5 if du < PR.FLAT32 else (u - c[lo]) * ((v[hi] - v[lo]) / du) + v[lo])
    if S == 1:
        return ts, [v[0], v[-1]]
    edges = [max(ts[0] - (ts[1] - ts[0]) * 0.5, v[0])]
    for sid in range(1, S):
        edges.append((ts[sid] + ts[sid - 1]) * 0.5)
    edges.append(min(ts[-1] + (ts[-1] - ts[-2]) * 0.5, v[-1]))
    return ts, edges


@pytest.mark.parametrize("S,E", [(1, 1), (2, 2), (1, 9), (5, 9), (17, 33), (33, 65)])
def test_vectorised_resampling_equals_the_loop(S, E):
    rng = case_rng(S, E, 1)
    v, c, _ = PR.exact_rows(rng, 23, E, S)
    for bias in (0.5, rng.random(23).astype(np.float32)):
        t64, e64 = PR.importance_sampling64(v, c, S, bias)
        b = np.broadcast_to(np.asarray(bias, np.float64), (23,))
        for r in range(23):
            t, e = loop_resample(v[r], c[r], S, b[r])
            assert np.array_equal(t64[r], np.asarray(t)) and np.array_equal(e64[r], np.asarray(e)), r
    # packed input rows give what the same rows give batched
    pi = np.stack([np.arange(23) * E, np.full(23, E)], -1)
    tp, ep = PR.importance_sampling64(v.reshape(-1), c.reshape(-1), S, 0.5, packed_info=pi)
    tb, eb = PR.importance_sampling64(v, c, S, 0.5)
    assert np.array_equal(tp, tb) and np.array_equal(ep, eb)


def test_per_ray_counts_equal_the_oracle(oracle):
    rng = case_rng(3)
    counts = np.array([0, 0, 0, 0, 0, 33, 1, 16] + list(rng.choice([0, 1, 2, 15, 16, 17, 33], 60)), np.int64)
    R, E = counts.size, 40
    v, c, _ = PR.exact_rows(rng, R, E, counts)
    sm, ed = PR.importance_sampling64(v, c, counts)
    o_ed, o_sm = oracle.importance_sampling_packed(v, c, counts)
    for got, want in ((sm, o_sm), (ed, o_ed)):
        assert np.array_equal(got["vals"].astype(np.float32), want["vals"])
        assert np.array_equal(got["vals"].astype(np.float32).astype(np.float64), got["vals"])
        assert np.array_equal(got["packed_info"], want["packed_info"]) and np.array_equal(got["ray_indices"], want["ray_indices"])
    assert np.array_equal(ed["is_left"], o_ed["is_left"]) and np.array_equal(ed["is_right"], o_ed["is_right"])
    # ragged packed input rows: every ray's own length, each row exact for its own count
    lens = rng.integers(8, 41, R)
    rows = [PR.exact_rows(rng, 1, int(n), int(k), flat_rows=False) for n, k in zip(lens, counts)]
    pi = np.stack([np.cumsum(lens) - lens, lens], -1)
    fv = np.concatenate([x[0][0] for x in rows]); fc = np.concatenate([x[1][0] for x in rows])
    sm, ed = PR.importance_sampling64(fv, fc, counts, packed_info=pi)
    o_ed, o_sm = oracle.importance_sampling_packed(fv, fc, counts, packed_info=pi)
    assert np.array_equal(sm["vals"].astype(np.float32), o_sm["vals"]) and np.array_equal(ed["vals"].astype(np.float32), o_ed["vals"])
    assert np.array_equal(ed["packed_info"], o_ed["packed_info"])


@pytest.mark.parametrize("S,E", [(4, 5), (16, 33), (33, 65), (64, 200), (150, 300)])
def test_stratified_band_holds_the_oracle(oracle, S, E):
    """The derived band [G(u - delta) - tau, G(u + delta) + tau] contains the float32 oracle's stratified samples, and few
    samples straddle a jump of G."""
    v, c, _ = PR.exact_rows(case_rng(S, E), R_CASE, E, S)
    seed, offset = 1234 + S, 8
    bias = np.array([oracle.philox_uniform(seed, r, offset) for r in range(R_CASE)], np.float32)
    _, o_t = oracle.importance_sampling(v, c, S, True, seed=seed, offset=offset)
    lo, hi, straddles, _, tau = PR.stratified_band(v, c, S, bias)
    assert float(straddles.mean()) < 0.005
    assert bool(((o_t >= lo) & (o_t <= hi)).all())
    mid = PR.importance_sampling64(v, c, S, bias)[0]
    worst = np.abs(o_t - mid)[~straddles].max() / tau
    print(f"S={S} E={E}: straddling {straddles.mean():.4f}, worst |oracle - G(u)| / tau away from jumps {worst:.3f}")


@pytest.mark.parametrize("Q,K", [(1, 1), (1, 2), (2, 33), (17, 1), (17, 33), (64, 2), (64, 33), (300, 700)])
def test_searchsorted64_equals_the_oracle(oracle, Q, K):
    rng = case_rng(Q, K, 2)
    kv = PR.value_rows(rng, R_CASE, K)
    qv = PR.value_rows(rng, R_CASE, Q, keys=kv)
    share = float((qv[:, :, None] == kv[:, None, :]).any(-1).mean())
    assert share >= 0.30, share
    if Q >= 2:
        assert (qv[:, 0] == 0).all() and (qv[:, -1] == 1).all()
    if K >= 2:
        assert (kv[:, 0] == 0).all() and (kv[:, -1] == 1).all()
    l, r = PR.searchsorted64(kv, qv)
    ol, orr = oracle.searchsorted(kv, qv)
    assert np.array_equal(l, ol) and np.array_equal(r, orr)
    for ray in range(0, R_CASE, 13):      # the definition, element by element
        for j in range(Q):
            p = next((i for i in range(K - 1) if kv[ray, i] > qv[ray, j]), K - 1)
            assert l[ray, j] == min(max(p - 1, 0), K - 1) and r[ray, j] == min(max(p, 0), K - 1)


@pytest.mark.parametrize("Q1,K1", LOSS_SHAPES + [(1024, 1024)])
def test_pdf_loss64_agrees_with_the_oracle(oracle, Q1, K1):
    R = 3 if Q1 == 1024 else R_CASE
    rng = case_rng(Q1, K1, 3)
    qv, qc, kv, kc = PR.loss_rows(rng, R, Q1, K1)
    g = rng.normal(size=(R, Q1 - 1)).astype(np.float32)
    eps = np.float32(1e-7)
    ref = PR.pdf_loss64(qv, qc, kv, kc, float(eps), g)
    share = float((ref["w"] - ref["wo"] > 0).mean())
    print(f"Q1={Q1} K1={K1}: share of intervals with w > w_outer {share:.3f}")
    assert 0.20 <= share <= 0.80
    # exact on these rows: w, w_outer and their difference
    w32 = qc[:, 1:] - qc[:, :-1]
    assert np.array_equal(w32.astype(np.float64), ref["w"])
    loss, saved = oracle.pdf_loss_batched(qv, qc, kv, kc, eps=eps)
    assert np.array_equal(saved[0], ref["left"]) and np.array_equal(saved[1], ref["right"])
    assert np.array_equal(saved[3].astype(np.float64), np.maximum(ref["w"] - ref["wo"], 0.0))
    g_kc = oracle.pdf_loss_batched_backward(g, saved)
    tol_l, tol_k, _ = PR.loss_bounds(ref)
    assert bool((np.abs(loss - ref["loss"]) <= tol_l).all())
    assert bool((np.abs(g_kc - ref["g_kc"]) <= tol_k).all())
    # the scatter-added gradients are the derivative of sum(g l): central differences in float64 on a few entries, with the
    # set of intervals where w > w_outer held fixed (w == w_outer == 0 is common on these rows, and l has a kink there).
    # l is quadratic in kc; in qc the differences' error is about h^2 / w^2 with w >= 2^-13 where w > w_outer.
    live = ref["w"] - ref["wo"] > 0
    h = 2.0 ** -26

    def total(r, qc_r, kc_r):
        w = np.diff(qc_r)
        wo = kc_r[ref["right"][r]] - kc_r[ref["left"][r]]
        return float((np.where(live[r], (w - wo) ** 2 / (w + float(eps)), 0.0) * g[r]).sum())

    for name, base, grad in (("kc", kc, ref["g_kc"]), ("qc", qc, ref["g_qc"])):
        for _ in range(6):
            r, i = int(rng.integers(R)), int(rng.integers(base.shape[1]))
            up, dn = base[r].astype(np.float64), base[r].astype(np.float64)
            up[i] += h; dn[i] -= h
            q64, k64 = qc[r].astype(np.float64), kc[r].astype(np.float64)
            num = ((total(r, up, k64) - total(r, dn, k64)) if name == "qc" else (total(r, q64, up) - total(r, q64, dn))) / (2 * h)
            assert abs(num - grad[r, i]) <= 1e-5 * max(1.0, ref["abs_" + name][r, i]), (name, r, i, num, grad[r, i])


def test_stot64_and_the_instance_table():
    s = np.array([0.0, 0.25, 1.0])
    assert np.array_equal(PR.stot64("uniform", s, 2.0, 6.0), [2.0, 3.0, 6.0])
    assert np.allclose(PR.stot64("lindisp", s, 2.0, 6.0), [2.0, 1 / (0.25 / 6 + 0.75 / 2), 6.0], rtol=1e-15)
    for name, Ss, Es in PR.INSTANCE_TABLE:
        for S in Ss:
            for E in Es:
                assert PR.resampling_instance(S, E) == name, (name, S, E)
                assert PR.resampling_instance(S, E, batched=False) == "general<not staged>"
    assert PR.rays_per_block(262144 + 37, 16) == 64 and PR.rays_per_block(262143, 16) == 32 and PR.rays_per_block(131, 1) == 1
    rows = {(3, 2): 2, (3, 16): 2, (5, 32): 4, (9, 64): 8, (17, 128): 16, (33, 256): 32, (65, 512): 64, (2, 1): 2}
    for Q1, K1 in LOSS_SHAPES + [(1024, 1024)]:
        want = f"rows<{rows[(Q1, K1)]}>" if (Q1, K1) in rows else "general"
        assert PR.loss_instance(Q1, K1).startswith(want), (Q1, K1, PR.loss_instance(Q1, K1))
    assert [PR.searchsorted_staged(q, 33) for q in (1, 2, 17, 64)] == [False, False, True, True]
    assert PR.searchsorted_staged(1, 2) and not PR.searchsorted_staged(300, 700)
