"""GPU: every kernel of csrc/pdf.hip on rows with tied, flat and saturated CDFs, against tests/pdf_reference.py.

The other PDF tests draw sorted random rows: no two CDF entries are equal, no query equals a key, no sample lands on a CDF
entry.  Here the rows come from ``pdf_reference.exact_rows`` -- most CDF steps are ties, rows are flat or saturate early,
and a good share of the samples sit exactly on a CDF entry, where ``upper_bound`` decides between two brackets an empty
region apart.  On these rows every float32 operation of the not-stratified resampling is exact, so the outputs must EQUAL
the float64 restatement (checked on the CPU against the C oracle by test_pdf_reference_cpu.py, which also asserts the
tie / flat / saturated / on-an-entry shares of the very rows used here: same ``case_rng`` keys).  Stratified resampling,
searchsorted and the loss are compared with float64 within bounds derived from the float32 operations.

Which kernel instance a shape selects cannot be seen from Python; ``pdf_reference.resampling_instance`` /
``loss_instance`` / ``searchsorted_staged`` restate the host-side launch rules of pdf.hip (read off
``launch_importance_sampling``, ``pdf_loss_plan`` and ``nfa_searchsorted``), each table row below is asserted against
them, and ``CallLog`` shows which C entry point ran and whether it was given packed input rows.
"""
import numpy as np
import pytest
import torch

import nerfacc_amd as na
import pdf_reference as PR
from nerfacc_amd import _backend as B
from nerfacc_amd.estimators.prop_net import _pdf_loss, _pdf_loss_mean, _transform_stot

pytestmark = pytest.mark.gpu

R_CASE = 131      # leaves every instance (64, 32, 16, 8, 4, 2, 1 rays per group) a ragged last group
TABLE = [(name, S, E) for name, Ss, Es in PR.INSTANCE_TABLE for S in Ss for E in Es]
TRANSFORMS = (("uniform", 2.0, 6.0), ("lindisp", 0.2, 7.3))


class CallLog:
    """Records every native call (name, arguments) while installed, as test_kernel_variants_gpu.CallLog does."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self):
        return [n for n, _ in self.calls]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def generator_state(dev, seed):
    """Seed the device's generator; (seed, offset) of the next stratified call."""
    torch.manual_seed(seed)
    gen = torch.cuda.default_generators[dev.index or 0]
    return int(gen.initial_seed()), int(gen.get_offset())


def resample_forms(dev, v, c, S, stratified=False, seed=0, log=None):
    """The same rows through every form of the library: {form: (samples (R, S), edges (R, S + 1))} as numpy.
    ``batched`` (the rows kernel or the staged general kernel), ``flattened`` (the same rows flat with packed_info:
    importance_sampling_kernel<false>) and ``counts`` (n_intervals_per_ray a constant Tensor: importance_sampling_packed_kernel,
    which refuses samples on rows without an interval, so E >= 2).  The generator is re-seeded before every call."""
    R, E = v.shape
    tv, tc = T(v, dev), T(c, dev)
    pi = torch.stack([torch.arange(R, device=dev) * E, torch.full((R,), E, device=dev)], -1)
    out = {}
    if stratified:
        generator_state(dev, seed)
    iv, sm = na.importance_sampling(na.RayIntervals(vals=tv), tc, S, stratified)
    out["batched"] = (N(sm.vals), N(iv.vals))
    if stratified:
        generator_state(dev, seed)
    iv, sm = na.importance_sampling(na.RayIntervals(vals=tv.reshape(-1), packed_info=pi), tc.reshape(-1), S, stratified)
    out["flattened"] = (N(sm.vals), N(iv.vals))
    if E >= 2:
        if stratified:
            generator_state(dev, seed)
        iv, sm = na.importance_sampling(na.RayIntervals(vals=tv), tc, torch.full((R,), S, dtype=torch.int64, device=dev), stratified)
        assert iv.vals.numel() == R * (S + 1) and sm.vals.numel() == R * S
        out["counts"] = (N(sm.vals).reshape(R, S), N(iv.vals).reshape(R, S + 1))
    if log is not None:
        calls = [(n, a) for n, a in log.calls if n.startswith("nfa_importance_sampling")]
        assert [n for n, _ in calls] == ["nfa_importance_sampling"] * 2 + ["nfa_importance_sampling_packed"] * (E >= 2)
        assert calls[0][1][2] is None and calls[1][1][2] is not None      # packed_info of the input rows
    return out


def assert_forms_agree(forms):
    ref_name = "batched"
    for name, (sm, iv) in forms.items():
        assert np.array_equal(sm, forms[ref_name][0]), (name, "samples")
        assert np.array_equal(iv, forms[ref_name][1]), (name, "edges")


# ----------------------------------------------------------------------------- a. resampling, exact
def check_exact(dev, monkeypatch, S, E, R):
    v, c, _ = PR.exact_rows(PR.case_rng(S, E) if R == R_CASE else PR.case_rng(S, E, R), R, E, S)
    t64, e64 = PR.importance_sampling64(v, c, S)
    want_t, want_e = t64.astype(np.float32), e64.astype(np.float32)
    log = CallLog(monkeypatch)
    forms = resample_forms(dev, v, c, S, log=log)
    # a form that agrees with the others but not with the reference points at the reference or the inputs (see
    # test_pdf_reference_cpu.py); a form that disagrees with the others is a kernel bug
    bad = {name: (int((sm != want_t).sum()), int((iv != want_e).sum())) for name, (sm, iv) in forms.items()
           if not (np.array_equal(sm, want_t) and np.array_equal(iv, want_e))}
    assert not bad, f"S={S} E={E}: forms off the float64 reference (samples, edges wrong): {bad}"
    tv, tc = T(v, dev), T(c, dev)
    for kind, lo, hi in TRANSFORMS:
        iv, sm, ts, te = na.importance_sampling(na.RayIntervals(vals=tv), tc, S, transform=(kind, lo, hi))
        assert np.array_equal(N(iv.vals), want_e) and np.array_equal(N(sm.vals), want_t), kind
        t_ref = _transform_stot(kind, iv.vals, lo, hi)
        assert ts.is_contiguous() and te.is_contiguous() and ts.shape == (R, S)
        assert torch.equal(ts, t_ref[:, :-1]) and torch.equal(te, t_ref[:, 1:]), kind
        t64 = PR.stot64(kind, e64, lo, hi)      # the mapping itself rounds: three products / sums and a reciprocal
        assert np.abs(N(t_ref) - t64).max() <= 8 * PR.U32 * np.abs(t64).max()
    assert log.names().count("nfa_importance_sampling_t") == 2


@pytest.mark.parametrize("name,S,E", TABLE)
def test_resampling_exact(dev, monkeypatch, name, S, E):
    assert PR.resampling_instance(S, E) == name and PR.resampling_instance(S, E, batched=False) == "general<not staged>"
    check_exact(dev, monkeypatch, S, E, R_CASE)


@pytest.mark.parametrize("R", [3, 1])
@pytest.mark.parametrize("S,E", [(2, 9), (24, 65), (64, 200), (150, 300)])
def test_resampling_exact_few_rays(dev, monkeypatch, S, E, R):
    check_exact(dev, monkeypatch, S, E, R)


def philox_biases(oracle, seed, offset, R):
    return np.array([oracle.philox_uniform(seed, r, offset) for r in range(R)], np.float32)


def edges32(t, t_min, t_max):
    """The edge formulas of pdf.hip in float32, operation for operation, on the kernel's own samples."""
    half = np.float32(0.5)
    R, S = t.shape
    e = np.empty((R, S + 1), np.float32)
    if S == 1:
        e[:, 0], e[:, 1] = t_min, t_max
        return e
    e[:, 1:S] = (t[:, 1:] + t[:, :-1]) * half
    e[:, 0] = np.maximum(t[:, 0] - (t[:, 1] - t[:, 0]) * half, t_min)
    e[:, S] = np.minimum(t[:, -1] + (t[:, -1] - t[:, -2]) * half, t_max)
    return e


def check_stratified(dev, oracle, v, c, S, seed, what):
    """Stratified resampling of tied rows: the forms agree bit for bit; every sample lies in the band
    [G(u - delta) - tau, G(u + delta) + tau] that ``pdf_reference.stratified_band`` derives from the float32 operations
    (delta, tau are not fitted to the kernel); fewer than 0.5 % of the samples straddle a jump of G; the edges are the
    float32 edge formulas applied to the samples."""
    R = v.shape[0]
    s, off = generator_state(dev, seed)
    bias = philox_biases(oracle, s, off, R)
    forms = resample_forms(dev, v, c, S, stratified=True, seed=seed)
    assert_forms_agree(forms)
    sm, iv = forms["batched"]
    lo, hi, straddles, delta, tau = PR.stratified_band(v, c, S, bias)
    share = float(straddles.mean())
    assert share < 0.005, (what, share)
    inside = (sm >= lo) & (sm <= hi)
    mid = PR.importance_sampling64(v, c, S, bias)[0]
    ratio = float((np.abs(sm - mid)[~straddles] / ((hi - lo)[~straddles] * 0.5)).max())
    print(f"{what}: straddling {share:.5f}, delta <= {float(delta.max()):.3e}, tau {tau:.3e}, "
          f"worst |sample - G(u)| / band half-width {ratio:.3f}")
    assert bool(inside.all()), (what, int((~inside).sum()))
    assert np.array_equal(iv, edges32(sm, v[:, 0], v[:, -1])), what
    return bias


# ----------------------------------------------------------------------------- b. resampling, stratified
@pytest.mark.parametrize("name,S,E", TABLE)
def test_resampling_stratified(dev, oracle, name, S, E):
    v, c, _ = PR.exact_rows(PR.case_rng(S, E), R_CASE, E, S)
    check_stratified(dev, oracle, v, c, S, 1000 + 7 * S + E, f"S={S} E={E}")


def test_resampling_stratified_bias_at_the_edge(dev, oracle):
    """A ray whose jitter is within 2^-12 of 1: sid + bias rounds towards sid + 1 and u sits just below the next sample's
    stratum.  The seed is found on the CPU by a bounded search of the Philox stream."""
    S, E = 16, 33
    _, off = generator_state(dev, 0)
    found = None
    for seed in range(1, 513):
        b = philox_biases(oracle, seed, off, R_CASE)
        if b.max() >= 1.0 - 2.0 ** -12:
            found = seed
            break
    assert found is not None, "no Philox draw >= 1 - 2^-12 among 512 seeds x 131 rays (probability e^-16)"
    v, c, _ = PR.exact_rows(PR.case_rng(S, E), R_CASE, E, S, flat_rows=False)
    bias = check_stratified(dev, oracle, v, c, S, found, f"edge bias, seed {found}")
    assert bias.max() >= 1.0 - 2.0 ** -12


def test_resampling_philox_block_of_64_rays(dev, oracle):
    """262144 + 37 rays of E = 3, S = 4: rows<4,1> with 16 rays per group, and enough rays that a wave's block is 64 rays
    whose Philox draws the lanes share out (the last block is ragged)."""
    R, E, S = 262144 + 37, 3, 4
    assert PR.resampling_instance(S, E) == "rows<4,1>" and PR.rays_per_block(R, 16) == 64
    rng = PR.case_rng(S, E, R)
    bv, bc, _ = PR.exact_rows(rng, 1024, E, S)
    pick = rng.integers(0, 1024, R)
    v, c = bv[pick], bc[pick]
    t64, e64 = PR.importance_sampling64(v, c, S)
    forms = resample_forms(dev, v, c, S)
    for name, (sm, iv) in forms.items():
        assert np.array_equal(sm, t64.astype(np.float32)) and np.array_equal(iv, e64.astype(np.float32)), name
    check_stratified(dev, oracle, v, c, S, 4242, "64-ray Philox block")


def test_resampling_per_ray_counts_exact(dev, monkeypatch):
    """Per-ray counts from {0, 1, 2, 15, 16, 17, 33} on exact rows, batched and flattened (ragged) input: a wave (4 rays)
    whose rays all have count 0, a wave with counts 0 / 33 / 1 / 16; values, packed_info, ray_indices and both masks."""
    rng = PR.case_rng(3, 1)
    counts = np.array([0, 0, 0, 0, 0, 33, 1, 16] + list(rng.choice([0, 1, 2, 15, 16, 17, 33], R_CASE - 8)), np.int64)
    E = 40
    v, c, _ = PR.exact_rows(rng, R_CASE, E, counts)
    lens = rng.integers(8, 41, R_CASE)
    rows = [PR.exact_rows(rng, 1, int(n), int(k), flat_rows=False) for n, k in zip(lens, counts)]
    pi = np.stack([np.cumsum(lens) - lens, lens], -1)
    fv = np.concatenate([x[0][0] for x in rows]); fc = np.concatenate([x[1][0] for x in rows])
    log = CallLog(monkeypatch)
    tcounts = T(counts, dev)
    for what, intervals, cdfs, ref in (
            ("batched", na.RayIntervals(vals=T(v, dev)), T(c, dev), PR.importance_sampling64(v, c, counts)),
            ("flattened", na.RayIntervals(vals=T(fv, dev), packed_info=T(pi, dev)), T(fc, dev),
             PR.importance_sampling64(fv, fc, counts, packed_info=pi))):
        iv, sm = na.importance_sampling(intervals, cdfs, tcounts)
        r_sm, r_iv = ref
        for got, want in ((sm, r_sm), (iv, r_iv)):
            assert np.array_equal(N(got.vals), want["vals"].astype(np.float32)), what
            assert np.array_equal(want["vals"].astype(np.float32).astype(np.float64), want["vals"])
            assert np.array_equal(N(got.packed_info), want["packed_info"]) and np.array_equal(N(got.ray_indices), want["ray_indices"])
        assert np.array_equal(N(iv.is_left), r_iv["is_left"]) and np.array_equal(N(iv.is_right), r_iv["is_right"]), what
    assert log.names().count("nfa_importance_sampling_packed") == 2


# ----------------------------------------------------------------------------- c. searchsorted
@pytest.mark.parametrize("Q,K", [(q, k) for q in (1, 2, 17, 64) for k in (1, 2, 33)] + [(300, 700)])
def test_searchsorted_tied_rows(dev, Q, K):
    """Batched queries and keys with 0, 1 and about half of the interior values in common: a wave spans 64, 32, 4 and 1
    rays for Q = 1, 2, 17, 64; (1, 33), (2, 33) and (300, 700) are too long for the stage (``searchsorted_staged``)."""
    assert PR.searchsorted_staged(Q, K) == ((Q, K) not in ((1, 33), (2, 33), (300, 700)))
    rng = PR.case_rng(Q, K, 2)
    kv = PR.value_rows(rng, R_CASE, K)
    qv = PR.value_rows(rng, R_CASE, Q, keys=kv)
    assert float((qv[:, :, None] == kv[:, None, :]).any(-1).mean()) >= 0.30
    want_l, want_r = PR.searchsorted64(kv, qv)
    l, r = na.searchsorted(na.RayIntervals(vals=T(kv, dev)), na.RayIntervals(vals=T(qv, dev)))
    assert np.array_equal(N(l), want_l) and np.array_equal(N(r), want_r)


@pytest.mark.parametrize("with_ray_indices", [False, True])
def test_searchsorted_packed_query_tied_rows(dev, with_ray_indices):
    """Packed queries (ragged: 0-40 per ray) on packed keys (ragged: 2-40 per ray): absolute ids into the flat key array."""
    rng = PR.case_rng(9, int(with_ray_indices))
    kn = rng.integers(2, 41, R_CASE); qn = rng.integers(0, 41, R_CASE)
    kv = PR.value_rows(rng, R_CASE, 40)
    qv = PR.value_rows(rng, R_CASE, 40, keys=kv)
    k_rows = [np.concatenate([kv[r, :n - 1], [1.0]]).astype(np.float32) for r, n in enumerate(kn)]
    q_rows = [qv[r, :n] for r, n in enumerate(qn)]
    k_start = np.cumsum(kn) - kn; q_start = np.cumsum(qn) - qn
    want = [PR.searchsorted64(k[None], q[None]) if q.size else (np.zeros((1, 0), np.int64),) * 2 for k, q in zip(k_rows, q_rows)]
    want_l = np.concatenate([w[0][0] + s for w, s in zip(want, k_start)])
    want_r = np.concatenate([w[1][0] + s for w, s in zip(want, k_start)])
    keys = na.RayIntervals(vals=T(np.concatenate(k_rows), dev), packed_info=T(np.stack([k_start, kn], -1), dev))
    ri = T(np.repeat(np.arange(R_CASE), qn), dev) if with_ray_indices else None
    query = na.RayIntervals(vals=T(np.concatenate(q_rows), dev), packed_info=T(np.stack([q_start, qn], -1), dev), ray_indices=ri)
    l, r = na.searchsorted(keys, query)
    assert np.array_equal(N(l), want_l) and np.array_equal(N(r), want_r)


# ----------------------------------------------------------------------------- c. the loss
LOSS_ROWS = [(3, 2), (3, 16), (5, 32), (9, 64), (17, 128), (33, 256), (65, 512)]      # one per lane count of the rows kernels
LOSS_GENERAL = [(66, 65), (129, 33), (4, 100), (1024, 1024), (2, 1)]
# (2, 1) is listed with the general shapes but pdf_loss_plan gives it to rows<2>: one interval per lane, 32 key entries.


def worst_ratio(got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    ok = err <= tol
    return bool(ok.all()), float((err / np.maximum(tol, 1e-300))[tol > 0].max()) if (tol > 0).any() else 0.0


@pytest.mark.parametrize("Q1,K1", LOSS_ROWS + LOSS_GENERAL)
def test_pdf_loss_against_float64(dev, monkeypatch, Q1, K1):
    """``_pdf_loss`` with an incoming gradient and ``_pdf_loss_mean`` against ``pdf_loss64``: the loss interval by interval
    (which also checks the key ids the forward saves for the backward), d / d k_cdfs and d / d q_cdfs entry by entry, within
    ``pdf_reference.loss_bounds`` (rounding counts times 2, derived there)."""
    inst = PR.loss_instance(Q1, K1)
    assert inst.startswith("rows") == ((Q1, K1) in LOSS_ROWS + [(2, 1)]), inst
    R = 3 if Q1 == 1024 else R_CASE
    rng = PR.case_rng(Q1, K1, 3)
    qv, qc, kv, kc = PR.loss_rows(rng, R, Q1, K1)
    g = rng.normal(size=(R, Q1 - 1)).astype(np.float32)
    eps32 = float(np.float32(1e-7))       # what the kernels hold
    ref = PR.pdf_loss64(qv, qc, kv, kc, eps32, g)
    share = float((ref["w"] - ref["wo"] > 0).mean())
    assert 0.20 <= share <= 0.80, share
    log = CallLog(monkeypatch)
    tqc, tkc = T(qc, dev).requires_grad_(True), T(kc, dev).requires_grad_(True)
    loss = _pdf_loss(na.RayIntervals(vals=T(qv, dev)), tqc, na.RayIntervals(vals=T(kv, dev)), tkc)
    (loss * T(g, dev)).sum().backward()
    assert log.names() == ["nfa_pdf_loss_fwd", "nfa_pdf_loss_bwd"]
    report, fine = [], True
    for name, got, want, tol in zip(("loss", "g_kc", "g_qc"), (loss, tkc.grad, tqc.grad), (ref["loss"], ref["g_kc"], ref["g_qc"]),
                                    PR.loss_bounds(ref)):
        ok, ratio = worst_ratio(N(got), want, tol)
        report.append(f"{name} {ratio:.3f}")
        fine &= ok
    # the mean form: g = 3 / count for every interval, one more rounding (the division) in the incoming gradient
    count = R * (Q1 - 1)
    ref_m = PR.pdf_loss64(qv, qc, kv, kc, eps32, np.full((R, Q1 - 1), 3.0 / count))
    n_part = int(B.load().nfa_pdf_loss_partials(R, Q1, K1))
    log.calls.clear()
    mqc, mkc = T(qc, dev).requires_grad_(True), T(kc, dev).requires_grad_(True)
    m = _pdf_loss_mean(na.RayIntervals(vals=T(qv, dev)), mqc, na.RayIntervals(vals=T(kv, dev)), mkc)
    (m * 3.0).backward()
    assert log.names() == ["nfa_pdf_loss_sum_fwd", "nfa_pdf_loss_mean_bwd"]
    _, tol_k, tol_q = PR.loss_bounds(ref_m, extra=1)
    tol_m = PR.loss_mean_bound(ref_m, n_part)
    err_m = abs(float(m.detach()) - float(ref_m["loss"].mean()))
    report.append(f"mean {err_m / tol_m:.3f} ({n_part} partials)")
    fine &= err_m <= tol_m
    for name, got, want, tol in (("mean g_kc", mkc.grad, ref_m["g_kc"], tol_k), ("mean g_qc", mqc.grad, ref_m["g_qc"], tol_q)):
        ok, ratio = worst_ratio(N(got), want, tol)
        report.append(f"{name} {ratio:.3f}")
        fine &= ok
    print(f"Q1={Q1} K1={K1} {inst}: share w > w_outer {share:.3f}; worst error / bound: " + ", ".join(report))
    assert fine, report
