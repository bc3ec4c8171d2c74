"""CPU: the preconditions that make the test-mode loop's GPU comparisons (tests/test_testmode_gpu.py) exact and
non-vacuous, asserted on the oracle alone -- so that an edit of a scene (tests/testmode_scenes.py) cannot quietly empty them:
no ray near the early-termination threshold, iterations that fill the padded loop's sample arrays to the last slot, rays
with more run records than the walk keeps, an alive list built by several workgroups and by one.
"""
import numpy as np
import pytest
import torch

import testmode_scenes as S


@pytest.mark.parametrize("scene", S.all_scenes(), ids=lambda s: s.name)
def test_no_ray_near_the_termination_threshold(oracle, scene):
    rgb, opa, dep, total, info = S.reference(scene)
    assert info["guard_rays"].sum() == 0
    assert np.isin(opa, (0.0, 1.0)).all()                       # exactly 0 or 1: the schedule cannot depend on an ulp
    assert sum(t[0] for t in info["trace"]) == total


@pytest.mark.parametrize("n_rays", S.FULL_SIZES)
def test_full_reaches_the_capacity(oracle, n_rays):
    """``n_alive * n_samples == n_rays``: the iteration's samples fill the padded loop's arrays (cap = max(n_rays, 4) slots,
    of which the tile table covers the iteration's total)."""
    mod, max_samples = S.FULL_SETTINGS[0]
    assert mod == 1
    _, _, _, total, info = S.reference(S.full(n_rays, mod, max_samples))
    at_capacity = sum(1 for t in info["trace"] if t[0] == n_rays)
    assert at_capacity >= (5 if n_rays == 128 else 1)
    assert all(t[0] <= n_rays for t in info["trace"])
    assert info["iterations"] > at_capacity                      # ... and iterations below it


@pytest.mark.parametrize("n_rays", S.FULL_SIZES)
def test_full_exhausts_max_samples(oracle, n_rays):
    """``mod = 3, max_samples = 6``: the loop ends because the budget is spent, with rays still alive, and the schedule
    overshoots ``max_samples`` where the last iteration's step limit does not divide what is left."""
    mod, max_samples = S.FULL_SETTINGS[1]
    sc = S.full(n_rays, mod, max_samples)
    _, _, _, total, info = S.reference(sc)
    tr = info["trace"]
    assert len(tr) == info["iterations"]                         # every iteration produced samples: rays were alive throughout
    handed_out = sum(max(min(n_rays // t[2], 64), 1) for t in tr)
    assert handed_out >= max_samples
    if n_rays == 128:
        assert info["iterations"] == 4 and handed_out == 7       # 1 + 2 + 2 + 2: past max_samples, as the reference's while


def test_checker_overflows_the_run_records(oracle):
    _, _, _, total, info = S.reference(S.checker())
    long_iterations = [i for i, t in enumerate(info["trace"]) if t[1] >= 10]
    assert len(long_iterations) >= 2       # (so at least one of them starts from termination planes, not from the near plane)


def test_checker_with_a_density_keeps_the_schedule(oracle):
    """``checker(0.5)``: the long-lived rays weigh something (the depth image sees the fill pass's sample positions), nobody
    comes near the termination threshold, and the iterations are those of the exact scene."""
    _, opa, dep, total, info = S.reference(S.checker(0.5), guard=2e-6)
    _, _, _, total0, info0 = S.reference(S.checker())
    assert info["guard_rays"].sum() == 0
    assert total == total0 and info["iterations"] == info0["iterations"]
    assert [t[:2] for t in info["trace"]] == [t[:2] for t in info0["trace"]]
    long_lived = np.arange(S.checker().n_rays) % S.checker().mod == 0
    assert (opa[long_lived] > 0.05).all() and (opa[long_lived] < 0.99).all() and (dep[long_lived] > 0).all()


def test_multi_alive_list_on_both_sides_of_a_workgroup(oracle):
    sc = S.multi()
    _, _, _, total, info = S.reference(sc)
    assert info["iterations"] >= 20 and total > 100_000
    alive = [t[2] for t in info["trace"]]
    assert alive[0] == sc.n_rays > 2 * S.ALIVE_PER_WG             # three workgroups
    assert any(0 < a < S.ALIVE_PER_WG for a in alive) and any(a > S.ALIVE_PER_WG for a in alive)


def test_multi_general_field_keeps_the_guard_band_small(oracle):
    _, opa, _, total, info = S.reference(S.multi(8.0), guard=2e-6)
    assert info["guard_rays"].mean() < 0.1 and total > 100_000
    assert ((opa > 0.01) & (opa < 0.99)).mean() > 0.05            # opacities that are neither 0 nor 1: the general arithmetic


def test_miss_has_no_samples(oracle):
    sc = S.miss()
    rgb, opa, dep, total, info = S.reference(sc)
    assert total == 0 and info["trace"] == ()
    assert (opa == 0).all() and (dep == 0).all() and (rgb == S.BKGD).all()


@pytest.mark.parametrize("scene", [S.full(128, 3, 6), S.full(5, 1, 600), S.multi(), S.multi(8.0), S.checker(), S.checker(0.5)], ids=lambda s: s.name)
def test_callbacks_agree_bit_for_bit(scene):
    rng = np.random.default_rng(7)
    n = 4096
    ri = np.sort(rng.integers(0, scene.n_rays, n))
    ts = rng.random(n).astype(np.float32)
    te = ts + np.float32(scene.step)
    rgbs, sig = S.field_np(scene)(ts, te, ri)
    rgbs_t, sig_t = S.field_torch(scene)(torch.from_numpy(ts), torch.from_numpy(te), torch.from_numpy(ri))
    assert rgbs_t.dtype == sig_t.dtype == torch.float32 and rgbs.dtype == sig.dtype == np.float32
    assert rgbs_t.shape == (n, 3) and sig_t.shape == (n,)
    assert np.array_equal(rgbs_t.numpy(), rgbs) and np.array_equal(sig_t.numpy(), sig)
    # exact in both half formats
    for half in (torch.float16, torch.bfloat16):
        assert torch.equal(rgbs_t.to(half).float(), rgbs_t) and torch.equal(sig_t.to(half).float(), sig_t)
    if scene.keep_sigma == 0:
        assert (np.float32(1) - np.exp(-(sig * (te - ts)).astype(np.float32)) == np.where(sig > 0, np.float32(1), np.float32(0))).all()
