"""CPU: the fused optimiser's restatement (tests/optim_reference.py) against torch, and nerfacc_amd.optim's CPU path, scaler,
schedule, state dict, work list and ABI against the restatement and torch."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from nerfacc_amd import optim as O   # the module under test: the restatement below is its written-down operation order
from optim_reference import RefAdam, RefScaler

CASES = {   # name: (weight_decay, decoupled)
    "adam": (0.0, False), "adam_l2": (1e-6, False), "adamw": (1e-2, True),
}


def _grads(rng, shape, lo=-8, hi=8):
    """Magnitudes in [2^lo, 2^hi], random signs: m, v and g^2 stay in float32's normal range."""
    return (np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_against_torch_float64(case):
    """30 steps at lr = 1e-2.  The restatement's largest deviation from torch's float64 run (p, m and v, over all steps) must
    not exceed twice the deviation of torch's own float32 run (foreach=False) from that float64 run, measured here on the same
    inputs.  (Bit equality with torch's float32 is not expected: its operation order differs.)"""
    wd, decoupled = CASES[case]
    assert O.CHUNK % 4 == 0
    rng = np.random.default_rng(7)
    n, steps, lr = 2000, 30, 1e-2
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [_grads(rng, n) for _ in range(steps)]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    runs = {}
    for dt in (torch.float64, torch.float32):
        p = torch.tensor(p0, dtype=dt, requires_grad=True)
        opt = cls([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
        runs[dt] = (p, opt)
    ref = RefAdam([p0], [dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, decoupled=decoupled, params=[0])])
    dev_ref, dev_t32 = np.zeros(3), np.zeros(3)
    for g in grads:
        for dt, (p, opt) in runs.items():
            p.grad = torch.tensor(g, dtype=dt)
            opt.step()
        ref.step([g.copy()])
        p64, o64 = runs[torch.float64]
        p32, o32 = runs[torch.float32]
        exact = [p64.detach().numpy(), o64.state[p64]["exp_avg"].numpy(), o64.state[p64]["exp_avg_sq"].numpy()]
        t32 = [p32.detach().numpy(), o32.state[p32]["exp_avg"].numpy(), o32.state[p32]["exp_avg_sq"].numpy()]
        mine = [ref.p[0], ref.m[0], ref.v[0]]
        for k in range(3):
            dev_ref[k] = max(dev_ref[k], np.abs(mine[k].astype(np.float64) - exact[k]).max())
            dev_t32[k] = max(dev_t32[k], np.abs(t32[k].astype(np.float64) - exact[k]).max())
    print(f"{case}: deviation from float64 (p, m, v): restatement {dev_ref}, torch float32 {dev_t32}")
    assert (dev_t32 > 0).all()
    assert (dev_ref <= 2 * dev_t32).all(), (dev_ref, dev_t32)


def _two_group_setup(rng, scaler=False, schedule=False, zero_grad=True):
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam, WarmupMultiStepLR
    # (20011 elements: enough that an operation that is not correctly rounded somewhere -- torch's CPU sqrt is off by an ulp on
    # 0.7 % to 17 % of random values, depending on the host -- cannot slip through)
    sizes = [(20011,), (33,), (4, 4, 3), (129,), (6,)]
    p0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    params = [torch.nn.Parameter(torch.tensor(p)) for p in p0]
    g0 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    g1 = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-15, weight_decay=1e-2)
    sch = dict(start_factor=0.01, warmup_iters=3, milestones=(4, 6), gamma=0.33) if schedule else None
    opt = FusedAdam([dict(params=params[:2], **g0), dict(params=params[2:], decoupled_weight_decay=True, skip_zero_grad=True, **g1)],
                    zero_grad=zero_grad, scaler=DeviceGradScaler(2.0 ** 10, growth_interval=2) if scaler else None,
                    schedule=WarmupMultiStepLR(**sch) if schedule else None)
    ref = RefAdam(p0, [dict(params=[0, 1], **g0), dict(params=[2, 3, 4], decoupled=True, skip_zero_grad=True, **g1)],
                  scaler=RefScaler(2.0 ** 10, growth_interval=2) if scaler else None, schedule=sch, zero_grad=zero_grad)
    return params, opt, ref


def _assert_same_bits(params, opt, ref, what):
    for i, p in enumerate(params):
        assert np.array_equal(p.detach().cpu().numpy().view(np.uint32), ref.p[i].view(np.uint32)), (what, "p", i)
        if p in opt.state and "exp_avg" in opt.state[p]:
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy().view(np.uint32), ref.m[i].view(np.uint32)), (what, "m", i)
            assert np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy().view(np.uint32), ref.v[i].view(np.uint32)), (what, "v", i)
        else:
            assert not ref.m[i].any() and not ref.v[i].any(), (what, "untouched", i)


@pytest.mark.parametrize("with_scaler", [False, True])
def test_fused_adam_cpu_equals_the_restatement(with_scaler):
    """Two param groups with different settings (L2 decay; decoupled decay with skip_zero_grad), a parameter whose grad is None
    (always, and another one on one step), zero_grad; with the scaler also a schedule and an overflow step: bit for bit."""
    rng = np.random.default_rng(11)
    params, opt, ref = _two_group_setup(rng, scaler=with_scaler, schedule=with_scaler)
    for step in range(7):
        scale = float(ref.scaler.scale) if with_scaler else 1.0
        grads = []
        for i, p in enumerate(params):
            if i == 1 or (i == 3 and step == 2):
                grads.append(None)
                p.grad = None
                continue
            g = _grads(rng, p.shape, -6, 6) * np.float32(scale)
            if i >= 2:
                g[rng.random(p.shape) < 0.5] = 0.0
            if with_scaler and step == 3 and i == 4:
                g.reshape(-1)[1] = np.inf
            grads.append(g)
            if p.grad is None:
                p.grad = torch.tensor(g)
            else:
                p.grad.copy_(torch.tensor(g))
        before = [p.detach().clone() for p in params]
        zeros = [None if g is None else torch.tensor(g == 0) for g in grads]   # (zero_grad clears the arrays)
        opt.step()
        ref.step(grads)
        _assert_same_bits(params, opt, ref, f"step {step}")
        for i, p in enumerate(params):
            if p.grad is not None:
                assert not p.grad.any(), "zero_grad leaves the gradients zero, on a skipped step too"
                if i >= 2 and not ref.last_skip:   # skip_zero_grad: bitwise untouched where the gradient was zero
                    z = zeros[i]
                    assert torch.equal(p.detach()[z], before[i][z])
                    if i == 3:   # (129 elements: both kinds are there)
                        assert z.any() and not z.all() and not (p.detach()[~z] == before[i][~z]).any()
        if with_scaler:
            assert opt.scaler.get_scale() == float(ref.scaler.scale) and opt.scaler.growth_tracker() == ref.scaler.tracker
            assert opt.last_factor() == float(ref.last_factor)
    if with_scaler:
        assert opt.scaler.skipped_steps() == 1 and opt.performed_steps() == 6 and opt.schedule_calls() == 7
        assert ref.step_count == 6 and ref.scaler.skipped == 1
    assert params[1].grad is None and params[1] not in opt.state


def test_zero_grad_off_keeps_the_gradients():
    rng = np.random.default_rng(3)
    params, opt, ref = _two_group_setup(rng, zero_grad=False)
    grads = [_grads(rng, p.shape) for p in params]
    for p, g in zip(params, grads):
        p.grad = torch.tensor(g)
    opt.step()
    ref.step([g.copy() for g in grads])
    _assert_same_bits(params, opt, ref, "zero_grad=False")
    for p, g in zip(params, grads):
        assert np.array_equal(p.grad.numpy(), g)


def test_scaler_policy_equals_torch_gradscaler():
    """The scale sequence and the set of skipped steps of DeviceGradScaler + FusedAdam equal torch.amp.GradScaler("cpu") driving
    torch.optim.Adam, an infinity injected at steps 3 and 4, growth_interval=2.  Scales are powers of two: equality is exact."""
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(50).astype(np.float32)
    pt = torch.nn.Parameter(torch.tensor(p0))
    pf = torch.nn.Parameter(torch.tensor(p0))
    topt = torch.optim.Adam([pt], lr=1e-2)
    tsc = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_interval=2)
    fsc = DeviceGradScaler(2.0 ** 10, growth_interval=2)
    fopt = FusedAdam([pf], lr=1e-2, scaler=fsc)
    t_scales, f_scales, t_skipped, f_skipped = [], [], set(), set()
    for step in range(10):
        g = _grads(rng, 50, -4, 4)
        if step in (3, 4):
            g[7] = np.inf
        assert tsc.get_scale() == fsc.get_scale()
        pt.grad = pf.grad = None
        with np.errstate(all="ignore"):
            tsc.scale((pt * torch.tensor(g)).sum()).backward()
            fsc.scale((pf * torch.tensor(g)).sum()).backward()
        assert torch.equal(pt.grad, pf.grad)
        bt, bf = pt.detach().clone(), pf.detach().clone()
        tsc.step(topt)
        tsc.update()
        fopt.step()
        if torch.equal(bt, pt.detach()):
            t_skipped.add(step)
        if torch.equal(bf, pf.detach()):
            f_skipped.add(step)
        t_scales.append(tsc.get_scale())
        f_scales.append(fsc.get_scale())
    assert f_scales == t_scales and f_skipped == t_skipped == {3, 4}, (f_scales, t_scales, f_skipped, t_skipped)
    assert len(set(f_scales)) > 2 and fsc.skipped_steps() == 2 and fopt.performed_steps() == 8
    # growth_interval=None: fixed on clean steps
    fixed = DeviceGradScaler(2.0 ** 10, growth_interval=None)
    fo = FusedAdam([torch.nn.Parameter(torch.tensor(p0))], scaler=fixed)
    for _ in range(3):
        fo.param_groups[0]["params"][0].grad = torch.ones(50)
        fo.step()
    assert fixed.get_scale() == 2.0 ** 10 and fixed.growth_tracker() == 0
    # the scaler's own state dict, loaded before and after its device state exists
    sd = fsc.state_dict()
    assert sd["scale"] == f_scales[-1] and sd["skipped_steps"] == 2
    for used in (False, True):
        other = DeviceGradScaler(4.0, growth_interval=7)
        if used:
            other.scale(torch.ones(()))
        other.load_state_dict(sd)
        assert other.state_dict() == sd


def test_schedule_equals_torch_chained_scheduler():
    """factor_at(t) against the LR sequence of ChainedScheduler([LinearLR, MultiStepLR]) at base lr 1, for every t to past the
    last milestone, within one float32 ulp (both are double computations rounded once)."""
    from nerfacc_amd.optim import WarmupMultiStepLR
    from torch.optim.lr_scheduler import ChainedScheduler, LinearLR, MultiStepLR
    for start, warm, ms, gamma in ((0.01, 100, (150, 200, 230), 0.33), (0.1, 7, (3, 9), 0.5), (1.0, 0, (2,), 0.1)):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        scheds = ([LinearLR(opt, start_factor=start, total_iters=warm)] if warm else []) + [MultiStepLR(opt, milestones=list(ms), gamma=gamma)]
        sch = ChainedScheduler(scheds)
        mine = WarmupMultiStepLR(start, warm, ms, gamma)
        for t in range(max(ms) + 30):
            want = np.float32(opt.param_groups[0]["lr"])
            got = np.float32(mine.factor_at(t))
            assert abs(float(got) - float(want)) <= float(np.spacing(want)), (t, got, want)
            opt.step()
            sch.step()


def test_state_dict_round_trip_with_torch_adam():
    """torch.optim.Adam -> FusedAdam and back through state_dict() / load_state_dict(), then one more step on each side from
    the same state and gradient.  The two implementations cannot agree bit for bit (torch forms g + wd p, the lerp, addcmul
    and addcdiv in its own order and with fused multiply-adds), so "equal" here is a TOLERANCE, per element, from the count of
    roundings: m and v take at most 4 roundings on each side, each 2^-24 of a quantity no larger than |g| + |m| (g^2 + v), so
    they differ by at most 8 * 2^-24 = 2^-21 of that; the update u = step_size m / (sqrt(v) / c + eps) takes at most 6 more
    on each side on top of those inputs, at most 2^-20 |u| between the sides, and p - u rounds once on each side: one ulp of
    p.  The largest observed difference over tolerance is printed.  A lost `step` would be off by 1 / (1 - beta^t): orders of
    magnitude more.  FusedAdam -> FusedAdam is exact."""
    from nerfacc_amd.optim import FusedAdam
    rng = np.random.default_rng(9)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in ((5, 3), (40,))]
    gs = [[_grads(rng, p.shape, -3, 3) for p in p0] for _ in range(8)]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)

    def run(opt, params, steps):
        for g in steps:
            for p, gi in zip(params, g):
                p.grad = torch.tensor(gi)
            opt.step()

    def close(a_params, a_opt, b_params, b_opt, before, g_last):
        worst = 0.0
        for a, b, p_old, g in zip(a_params, b_params, before, g_last):
            a64, b64, g64 = a.detach().double(), b.detach().double(), torch.tensor(g).double()
            ma, mb = a_opt.state[a]["exp_avg"].double(), b_opt.state[b]["exp_avg"].double()
            va, vb = a_opt.state[a]["exp_avg_sq"].double(), b_opt.state[b]["exp_avg_sq"].double()
            ulp_p = torch.tensor(np.spacing(np.abs(a.detach().numpy())).astype(np.float64))
            for diff, tol in (((a64 - b64).abs(), ulp_p + 2.0 ** -20 * (a64 - p_old.double()).abs()),
                              ((ma - mb).abs(), 2.0 ** -21 * (g64.abs() + ma.abs())),
                              ((va - vb).abs(), 2.0 ** -21 * (g64 * g64 + va))):
                assert (diff <= tol).all(), float((diff / tol).max())
                worst = max(worst, float((diff / tol).max()))
        print(f"state-dict round trip: largest difference / tolerance {worst:.3f}")

    # torch (3 steps) -> fused, one more step on both
    tp = [torch.nn.Parameter(torch.tensor(p)) for p in p0]
    topt = torch.optim.Adam(tp, foreach=False, **kw)
    run(topt, tp, gs[:3])
    fp = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    fopt = FusedAdam(fp, **kw)
    fopt.load_state_dict(copy.deepcopy(topt.state_dict()))   # (torch's load_state_dict shares same-dtype state tensors)
    assert fopt.performed_steps() == 3 and fopt.schedule_calls() == 3
    before = [p.detach().clone() for p in fp]
    run(topt, tp, gs[3:4])
    run(fopt, fp, gs[3:4])
    close(fp, fopt, tp, topt, before, gs[3])
    # fused (3 more) -> torch, one more step on both
    run(fopt, fp, gs[4:7])
    sd = copy.deepcopy(fopt.state_dict())
    assert all(float(s["step"]) == 7.0 for s in sd["state"].values())
    tp2 = [torch.nn.Parameter(p.detach().clone()) for p in fp]
    topt2 = torch.optim.Adam(tp2, foreach=False, **kw)
    topt2.load_state_dict(sd)
    before = [p.detach().clone() for p in fp]
    run(fopt, fp, gs[7:8])
    run(topt2, tp2, gs[7:8])
    close(fp, fopt, tp2, topt2, before, gs[7])
    # fused -> fused is exact
    fp3 = [torch.nn.Parameter(p.detach().clone()) for p in fp]
    fopt3 = FusedAdam(fp3, **kw)
    fopt3.load_state_dict(copy.deepcopy(fopt.state_dict()))
    run(fopt, fp, gs[0:1])
    run(fopt3, fp3, gs[0:1])
    for a, b in zip(fp, fp3):
        assert torch.equal(a.detach(), b.detach()) and torch.equal(fopt.state[a]["exp_avg_sq"], fopt3.state[b]["exp_avg_sq"])
    # per-parameter steps that differ cannot be loaded
    sd = fopt.state_dict()
    sd["state"][0]["step"] = torch.tensor(2.0)
    with pytest.raises(ValueError, match="steps differ"):
        fopt3.load_state_dict(sd)


def test_parameter_checks_name_the_parameter():
    from nerfacc_amd.optim import FusedAdam
    with pytest.raises(TypeError, match="parameter 1 of group 0.*float64"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="parameter 0 of group 0.*not contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, 3).t())])
    p = torch.nn.Parameter(torch.zeros(4, 3))
    opt = FusedAdam([p])
    p.grad = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match="gradient of parameter 0 of group 0.*contiguous"):
        opt.step()
    named = FusedAdam([("table", torch.nn.Parameter(torch.zeros(4, 3)))])
    named.param_groups[0]["params"][0].grad = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match="gradient of parameter 'table'"):
        named.step()
    with pytest.raises(ValueError, match="parameter 0 of group 0.*not a leaf"):
        FusedAdam([torch.zeros(3, requires_grad=True) * 2])


def test_work_list_covers_every_element_once():
    from nerfacc_amd.optim import CHUNK, CHUNK_DTYPE, build_work_list
    for c in (CHUNK, 8):
        sizes = [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 3, 0]
        work = build_work_list(sizes, c)
        assert work.dtype == CHUNK_DTYPE and work.dtype.itemsize == 8
        seen = [np.zeros(n, dtype=np.int32) for n in sizes]
        for t, k in zip(work["tensor"].tolist(), work["chunk"].tolist()):
            start, end = k * c, min(sizes[t], (k + 1) * c)
            assert 0 <= start < end <= sizes[t], "a chunk lies inside its tensor and is not empty"
            seen[t][start:end] += 1
        assert all((s == 1).all() for s in seen)
        assert len(work) == sum((n + c - 1) // c for n in sizes)


def test_optim_abi():
    from nerfacc_amd import _backend as B
    from nerfacc_amd import optim as O
    lib = B.load()
    hdr = open(os.path.join(ROOT, "include", "nerfacc_hip.h")).read()
    for fn in ("nfa_optim_chunk_elems", "nfa_optim_scan", "nfa_optim_decide", "nfa_optim_update"):
        assert fn in B.EXPORTED_SYMBOLS and hasattr(lib, fn) and re.search(r"\bint " + fn + r"\(", hdr)
    assert lib.nfa_version() == 403 and B.ABI_VERSION == 403
    assert lib.nfa_optim_chunk_elems() == O.CHUNK == int(re.search(r"#define NFA_OPTIM_CHUNK (\d+)", hdr).group(1))
    assert C.sizeof(B.OptimGroup) == 48 and C.sizeof(B.OptimArgs) == 8 + 16 * 48 + 16 + 8 + 64 + 16
    # host-decided argument errors: nothing is launched
    P = 0x1000
    assert lib.nfa_optim_decide(None, P, None, None) == -1 and b"null pointer" in lib.nfa_last_error()
    assert lib.nfa_optim_decide(C.byref(B.OptimArgs()), None, None, None) == -1
    a = B.OptimArgs()
    a.n_groups = 17
    assert lib.nfa_optim_decide(C.byref(a), P, None, None) == -1 and b"16 param groups" in lib.nfa_last_error()
    assert lib.nfa_optim_scan(1, P, 1, P, 1, P, None) == -1 and b"float32" in lib.nfa_last_error()
    assert lib.nfa_optim_scan(0, P, -1, P, 1, P, None) == -1 and b"negative count" in lib.nfa_last_error()
    assert lib.nfa_optim_scan(0, P, 1, P, 1, None, None) == -1 and b"null scaler" in lib.nfa_last_error()
    assert lib.nfa_optim_scan(0, None, 1, P, 1, P, None) == -1 and b"null pointer" in lib.nfa_last_error()
    assert lib.nfa_optim_update(2, P, 1, P, 1, P, 0, None) == -1 and b"float32" in lib.nfa_last_error()
    assert lib.nfa_optim_update(0, P, 1, P, -1, P, 0, None) == -1 and b"negative count" in lib.nfa_last_error()
    assert lib.nfa_optim_update(0, P, 1, None, 1, P, 0, None) == -1 and b"null pointer" in lib.nfa_last_error()
    assert lib.nfa_optim_update(0, P, 1, P, 1, None, 0, None) == -1 and b"null state" in lib.nfa_last_error()
    assert lib.nfa_optim_update(0, None, 0, None, 0, P, 0, None) == 0


def test_plan_follows_replaced_moments_and_a_changed_schedule():
    """The cached plan of step() is redone when a moment tensor is put into `state` by hand, and the cached argument struct
    when a field of the schedule changes: both against a fresh optimiser given the same state."""
    from nerfacc_amd.optim import FusedAdam, WarmupMultiStepLR
    rng = np.random.default_rng(2)
    p0 = rng.standard_normal(50).astype(np.float32)
    gs = [_grads(rng, 50, -3, 3) for _ in range(3)]
    sch = WarmupMultiStepLR(0.5, 4, (), 0.33)
    p = torch.nn.Parameter(torch.tensor(p0))
    opt = FusedAdam([p], lr=1e-2, schedule=sch)
    p.grad = torch.tensor(gs[0])
    opt.step()
    old_m = opt.state[p]["exp_avg"]
    kept = old_m.clone()
    opt.state[p]["exp_avg"] = torch.full_like(old_m, 0.25)
    sch.start_factor = 0.125
    p_before = p.detach().clone()
    p.grad = torch.tensor(gs[1])
    opt.step()
    assert torch.equal(old_m, kept), "the replaced tensor is no longer written"
    ref = RefAdam([p_before.numpy()], [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, params=[0])],
                  schedule=dict(start_factor=0.125, warmup_iters=4, milestones=(), gamma=0.33))
    ref.m[0][...] = 0.25
    ref.v[0] = None
    # the second step of a run whose first step left v as the optimiser has it
    ref.calls = ref.step_count = 1
    ref.pow = [[0.9, 0.999]]
    v_after_first = (np.float32(1.0 - 0.999) * (gs[0] * gs[0])).astype(np.float32)   # beta2 * 0 + (1 - beta2) g^2
    ref.v[0] = v_after_first
    ref.step([gs[1].copy()])
    assert np.array_equal(p.detach().numpy().view(np.uint32), ref.p[0].view(np.uint32))
    assert np.array_equal(opt.state[p]["exp_avg"].numpy().view(np.uint32), ref.m[0].view(np.uint32))
    assert opt.last_factor() == np.float32(0.125 + 0.875 * 1.0 / 4.0)
