"""GPU: the fused optimiser's kernels (csrc/optim.hip) against the numpy restatement (tests/optim_reference.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from optim_reference import RefAdam, RefScaler

pytestmark = pytest.mark.gpu

G0 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
G1 = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-15)
CASES = {   # name: (group settings of the reference, zero_grad, share of exactly-zero gradients)
    "l2": (dict(weight_decay=1e-6), False, 0.0),
    "decoupled": (dict(weight_decay=1e-2, decoupled=True), False, 0.0),
    "skip_zero_grad": (dict(weight_decay=1e-2, decoupled=True, skip_zero_grad=True), False, 0.5),
    "zero_grad": (dict(weight_decay=0.0), True, 0.0),
}
UNALIGNED = 1027   # elements of the parameter that starts 4 bytes off a 16-byte boundary (and of its aligned twin)


def _sizes():
    from nerfacc_amd.optim import CHUNK as c
    return [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 3]


def _grads(rng, shape, zero_share=0.0, lo=-6, hi=6):
    g = (np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if zero_share:
        g[rng.random(shape) < zero_share] = 0.0
    return g


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _fused_kw(ref_kw):
    kw = dict(ref_kw)
    kw["decoupled_weight_decay"] = kw.pop("decoupled", False)
    return kw


def _build(dev, rng, case, scaler=False):
    """One optimiser over the boundary sizes plus the unaligned leaf view and an aligned twin of it with the same values, in
    two param groups, and its restatement."""
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam
    ref_kw, zero_grad, _ = CASES[case]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in _sizes()]
    p0 += [rng.standard_normal(UNALIGNED).astype(np.float32)]
    p0 += [p0[-1].copy()]
    params = [torch.tensor(p, device=dev).requires_grad_() for p in p0[:-2]]
    base = torch.zeros(UNALIGNED + 1, device=dev)
    base[1:] = torch.tensor(p0[-2], device=dev)
    off = base[1:].requires_grad_()   # a leaf that starts 4 bytes behind a 16-byte boundary
    assert off.is_leaf and off.data_ptr() % 16 == 4 and off.is_contiguous()
    params += [off, torch.tensor(p0[-1], device=dev).requires_grad_()]
    half = len(params) // 2
    idx = list(range(len(params)))
    opt = FusedAdam([dict(params=params[:half], **G0, **_fused_kw(ref_kw)), dict(params=params[half:], **G1, **_fused_kw(ref_kw))],
                    zero_grad=zero_grad, scaler=DeviceGradScaler(2.0 ** 10, growth_interval=2) if scaler else None)
    ref = RefAdam(p0, [dict(params=idx[:half], **G0, **ref_kw), dict(params=idx[half:], **G1, **ref_kw)],
                  scaler=RefScaler(2.0 ** 10, growth_interval=2) if scaler else None, zero_grad=zero_grad)
    return params, opt, ref


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
        p.grad.copy_(torch.from_numpy(g))


def _assert_state_bits(params, opt, ref, what):
    for i, p in enumerate(params):
        assert np.array_equal(_bits(p), _bits(ref.p[i])), (what, "p", i, p.numel())
        assert np.array_equal(_bits(opt.state[p]["exp_avg"]), _bits(ref.m[i])), (what, "m", i, p.numel())
        assert np.array_equal(_bits(opt.state[p]["exp_avg_sq"]), _bits(ref.v[i])), (what, "v", i, p.numel())


@pytest.mark.parametrize("case", list(CASES))
def test_native_step_equals_the_restatement(dev, case):
    """p, m and v bit for bit over 5 steps; the parameter on the scalar path (4 bytes off alignment) and its aligned twin on
    the vector path get the same values and gradients and must agree with each other too."""
    rng = np.random.default_rng(21)
    params, opt, ref = _build(dev, rng, case)
    _, zero_grad, zero_share = CASES[case]
    for step in range(5):
        grads = [_grads(rng, p.shape, zero_share) for p in params[:-1]]
        grads.append(grads[-1].copy())
        _set_grads(params, grads)
        before = [p.detach().clone() for p in params]
        ref.step([g.copy() for g in grads])
        opt.step()
        _assert_state_bits(params, opt, ref, f"{case} step {step}")
        assert np.array_equal(_bits(params[-2]), _bits(params[-1])), "scalar path and vector path differ"
        if zero_share:   # untouched elements are bitwise unchanged, the others moved
            for p, b, g in zip(params, before, grads):
                z = torch.from_numpy(g == 0).to(dev)
                assert torch.equal(p.detach()[z], b[z])
            z = torch.from_numpy(grads[-1] == 0).to(dev)
            assert z.any() and not z.all() and not (params[-1].detach()[~z] == before[-1][~z]).any()
        for p, g in zip(params, grads):
            if zero_grad:
                assert not p.grad.any()
            else:
                assert np.array_equal(_bits(p.grad), _bits(g)), "the gradients are left alone without zero_grad"
    assert opt.performed_steps() == 5 and opt.schedule_calls() == 5


def test_more_chunks_than_workgroups(dev):
    """A tensor of more chunks than the update launches workgroups (2048): the grid-stride loop over the work list, with whole
    16-byte pieces and whole chunks of zero gradients under skip_zero_grad, one step with zero_grad."""
    from nerfacc_amd.optim import CHUNK, FusedAdam
    rng = np.random.default_rng(4)
    n = 2048 * CHUNK + 3 * CHUNK + 5
    p0 = rng.standard_normal(n).astype(np.float32)
    g = _grads(rng, n)
    g[rng.random(n // 4 + 1).repeat(4)[:n] < 0.5] = 0.0      # pieces
    g[CHUNK * 7:CHUNK * 9] = 0.0                             # chunks
    g[rng.random(n) < 0.1] = 0.0
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=1e-6)
    p = torch.tensor(p0, device=dev).requires_grad_()
    opt = FusedAdam([p], skip_zero_grad=True, zero_grad=True, **kw)
    ref = RefAdam([p0], [dict(params=[0], skip_zero_grad=True, **kw)])
    for _ in range(2):
        _set_grads([p], [g])
        opt.step()
        ref.step([g])
        assert not p.grad.any()
    _assert_state_bits([p], opt, ref, "large")


def test_scaler_on_the_device(dev, monkeypatch):
    """An infinity in one element of the LAST tensor at step 2 and a NaN in the FIRST tensor at step 5: on those steps p, m, v
    and the update counter are bitwise unchanged and the gradients are still zeroed; scale and tracker follow the restatement
    step by step; every step() is at most three native calls, one launch each.  No torch.cuda.synchronize anywhere."""
    from nerfacc_amd import _backend as B
    rng = np.random.default_rng(33)
    params, opt, ref = _build(dev, rng, "zero_grad", scaler=True)
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    performed = 0
    for step in range(8):
        scale = np.float32(ref.scaler.scale)
        grads = [_grads(rng, p.shape) * scale for p in params[:-1]]
        grads.append(grads[-1].copy())
        if step == 2:
            grads[-1][UNALIGNED - 1] = np.inf
        if step == 5:
            grads[0][0] = np.nan
        _set_grads(params, grads)
        before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) if p in opt.state else None
                  for p in params]
        del calls[:]
        opt.step()
        assert calls == ["nfa_optim_scan", "nfa_optim_decide", "nfa_optim_update"], calls
        ref.step(grads)
        performed += step not in (2, 5)
        assert ref.last_skip == (step in (2, 5))
        if ref.last_skip:
            for p, b in zip(params, before):
                assert np.array_equal(_bits(p), _bits(b[0])) and np.array_equal(_bits(opt.state[p]["exp_avg"]), _bits(b[1]))
                assert np.array_equal(_bits(opt.state[p]["exp_avg_sq"]), _bits(b[2]))
        _assert_state_bits(params, opt, ref, f"step {step}")
        assert all(not p.grad.any() for p in params)
        assert opt.performed_steps() == performed == ref.step_count
        assert opt.scaler.get_scale() == float(ref.scaler.scale) and opt.scaler.growth_tracker() == ref.scaler.tracker
    assert opt.scaler.skipped_steps() == 2 and opt.schedule_calls() == 8
    assert len({2.0 ** 10, opt.scaler.get_scale()}) == 2, "the scale moved"


def test_sixty_four_tensors_three_launches(dev, monkeypatch):
    """64 tensors in 3 groups: still three calls, and the restatement's bits."""
    from nerfacc_amd import _backend as B
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam
    rng = np.random.default_rng(8)
    p0 = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(1, 700, 64)]
    params = [torch.tensor(p, device=dev).requires_grad_() for p in p0]
    groups = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6), dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.0),
              dict(lr=5e-3, betas=(0.5, 0.9), eps=1e-10, weight_decay=1e-3)]
    cut = [0, 20, 41, 64]
    opt = FusedAdam([dict(params=params[cut[k]:cut[k + 1]], **groups[k]) for k in range(3)], scaler=DeviceGradScaler(4.0, growth_interval=None))
    ref = RefAdam(p0, [dict(params=list(range(cut[k], cut[k + 1])), **groups[k]) for k in range(3)], scaler=RefScaler(4.0, growth_interval=None))
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for step in range(3):
        grads = [_grads(rng, p.shape) * np.float32(4.0) for p in params]
        _set_grads(params, grads)
        del calls[:]
        opt.step()
        assert len(calls) == 3, calls
        ref.step(grads)
    _assert_state_bits(params, opt, ref, "64 tensors")


def _field_run(dev, inputs, captured):
    """Three warm-up steps on inputs[0], then one step per entry of inputs[1:]; eager or as replays of a CapturedStep."""
    from nerfacc_amd import CapturedStep
    from nerfacc_amd.mlp import FusedMLP
    from nerfacc_amd.optim import DeviceGradScaler, FusedAdam, WarmupMultiStepLR
    mlp = FusedMLP(16, 4, n_neurons=64, n_hidden_layers=1, out_dtype=torch.float32, generator=torch.Generator().manual_seed(5)).to(dev)
    scaler = DeviceGradScaler(2.0 ** 10, growth_interval=2)
    opt = FusedAdam(mlp.parameters(), lr=1e-2, eps=1e-15, weight_decay=1e-6, zero_grad=True, scaler=scaler,
                    schedule=WarmupMultiStepLR(0.01, 4, (6,), 0.33))
    x = torch.from_numpy(inputs[0][0]).to(dev)
    y = torch.from_numpy(inputs[0][1]).to(dev)

    def fwd_bwd():
        if captured == "behind":   # (a host action: the capture sees a stale image cache and holds the rebuild)
            torch.autograd.graph.increment_version(mlp.params)
        loss = ((mlp(x) - y) ** 2).mean()
        scaler.scale(loss).backward()
        return loss

    def fn():
        loss = fwd_bwd()
        opt.step()
        return loss

    if captured == "behind":   # forward + backward as a graph, step() eager behind every replay
        for _ in range(3):
            fn()
        graph = CapturedStep(fwd_bwd, warmup=1)
        mlp.params.grad.zero_()   # (the warm-up run and nothing else accumulated into it)
        step = lambda: (graph(), opt.step())
    elif captured:
        step = CapturedStep(fn, warmup=3)
    else:
        for _ in range(3):
            fn()
        step = fn
    for xi, yi in inputs[1:]:
        x.copy_(torch.from_numpy(xi))
        y.copy_(torch.from_numpy(yi))
        step()
    p = mlp.params
    rec = opt._state_record()
    return dict(p=_bits(p).copy(), m=_bits(opt.state[p]["exp_avg"]).copy(), v=_bits(opt.state[p]["exp_avg_sq"]).copy(),
                scale=scaler.get_scale(), tracker=scaler.growth_tracker(), skipped=scaler.skipped_steps(),
                step=int(rec["step"][0]), calls=int(rec["calls"][0]), factor=float(rec["factor"][0]))


def test_captured_step_equals_eager(dev):
    """A whole step of a small field -- FusedMLP 16 -> 64 -> 4 on 256 points, squared error, FusedAdam with a scaler and a
    schedule -- captured with CapturedStep and replayed 6 times on new inputs, one of them with an infinity in the target, gives
    the bits of the same steps run eagerly: p, m, v, the scale and the counters."""
    rng = np.random.default_rng(17)
    inputs = [(rng.standard_normal((256, 16)).astype(np.float32), rng.standard_normal((256, 4)).astype(np.float32)) for _ in range(7)]
    inputs[4][1][3, 2] = np.inf
    eager = _field_run(dev, inputs, captured=False)
    graph = _field_run(dev, inputs, captured=True)
    assert eager["skipped"] == 1 and eager["step"] == 8 and eager["calls"] == 9, eager
    for k in ("scale", "tracker", "skipped", "step", "calls", "factor"):
        assert eager[k] == graph[k], (k, eager[k], graph[k])
    for k in ("p", "m", "v"):
        assert np.array_equal(eager[k], graph[k]), k
    assert np.isfinite(eager["p"].view(np.float32)).all()
    # A graph of forward + backward ALONE with step() behind each replay trains on the updated weights only because the
    # captured function bumps the masters' version counter (FusedAdam's docstring): then it is the same run bit for bit.
    behind = _field_run(dev, inputs, captured="behind")
    for k in ("scale", "tracker", "skipped", "step", "calls", "factor"):
        assert eager[k] == behind[k], (k, eager[k], behind[k])
    for k in ("p", "m", "v"):
        assert np.array_equal(eager[k], behind[k]), k


def test_argument_errors_return_codes(dev):
    """Null pointers, negative counts and a non-float32 dtype code come back as NFA_EINVAL with real device buffers in the other
    arguments; nothing is launched for them, and a step afterwards still works."""
    from nerfacc_amd import _backend as B
    from nerfacc_amd.optim import FusedAdam
    lib = B.load()
    p = torch.ones(10, device=dev).requires_grad_()
    opt = FusedAdam([p], lr=0.5)
    p.grad = torch.ones(10, device=dev)
    opt.step()
    table, work, state = opt._table.data_ptr(), opt._work.data_ptr(), opt._state_buf.data_ptr()
    scaler = torch.zeros(4, dtype=torch.int64, device=dev).data_ptr()
    s = B.stream()
    bad = [
        ("nfa_optim_scan", (1, table, 1, work, 1, scaler, s), b"float32"),
        ("nfa_optim_scan", (0, table, -1, work, 1, scaler, s), b"negative count"),
        ("nfa_optim_scan", (0, table, 1, work, -1, scaler, s), b"negative count"),
        ("nfa_optim_scan", (0, table, 1, work, 1, None, s), b"null scaler"),
        ("nfa_optim_scan", (0, None, 1, work, 1, scaler, s), b"null pointer"),
        ("nfa_optim_scan", (0, table, 1, None, 1, scaler, s), b"null pointer"),
        ("nfa_optim_decide", (None, state, None, s), b"null pointer"),
        ("nfa_optim_decide", (C.byref(opt._args()), None, None, s), b"null pointer"),
        ("nfa_optim_update", (2, table, 1, work, 1, state, 0, s), b"float32"),
        ("nfa_optim_update", (0, table, -1, work, 1, state, 0, s), b"negative count"),
        ("nfa_optim_update", (0, table, 1, work, -1, state, 0, s), b"negative count"),
        ("nfa_optim_update", (0, table, 1, work, 1, None, 0, s), b"null state"),
        ("nfa_optim_update", (0, None, 1, work, 1, state, 0, s), b"null pointer"),
        ("nfa_optim_update", (0, table, 1, None, 1, state, 0, s), b"null pointer"),
    ]
    for fn, args, text in bad:
        assert getattr(lib, fn)(*args) == -1 and text in lib.nfa_last_error(), (fn, args, lib.nfa_last_error())
    assert lib.nfa_optim_update(0, table, 0, work, 0, state, 0, s) == 0 and lib.nfa_optim_scan(0, table, 0, work, 0, scaler, s) == 0
    before = p.detach().clone()
    p.grad = torch.ones(10, device=dev)
    opt.step()
    assert opt.performed_steps() == 2 and not torch.equal(p.detach(), before) and torch.isfinite(p).all()
