"""CPU: the fused MLPs at the edges of fp16 / bf16 and on non-finite values, through the modules' torch path.  The tables of
tests/mlp_edges_reference.py (scaled exact cases that live among the subnormals or pass MAX, hand-built rows at MAX + ulp/2,
one NaN / inf in one row, a dead neuron under an infinite gradient, a loss scale that overflows inside the backward) against
the float64 restatements by class (NaN, +inf, -inf) and bits; the conditions that make those tables worth running, asserted
on the restatement; and the proof that a restatement which saturates or flushes would be caught.  tests/test_mlp_edges_gpu.py
runs the same tables through the kernels.  Nothing here reaches a GPU."""
import pytest
import torch

import mlp_bias_skip_reference as S
import mlp_edges_reference as E
import mlp_grad2_reference as G
import mlp_reference as R
import mlp_stream_reference as Q
from nerfacc_amd.mlp import FusedMLP, StreamedMLP
from nerfacc_amd.optim import DeviceGradScaler, FusedAdam

F16, BF16, F32 = E.F16, E.BF16, E.F32
dt = lambda d: str(d).split(".")[-1]
ends = lambda f: "f32-ends" if f else "half-ends"


# ---------------------------------------------------------------- running a case through a module (either device)

def make_module(c, device="cpu"):
    out = F32 if c.out_f32 else None
    if c.kind == "stream":
        m = StreamedMLP(*c.shape, dtype=c.dtype, out_dtype=out, bias=c.bs is not None, skip_layer=c.skip_layer)
    else:
        m = FusedMLP(*c.shape, dtype=c.dtype, out_dtype=out, second_order=c.second, bias=c.bs is not None, skip_layer=c.skip_layer)
    m.load_linear_weights(c.ws, c.bs)
    return m.to(device)


def run_module(m, c, x=None, g=None, v=None):
    """dict(y, dx, dp) and, for a case with a second order, (u, d2p) with v as the cotangent of dL/dx: real autograd."""
    dev = m.params.device
    x = (c.x if x is None else x).to(dev).requires_grad_(True)
    y = m(x)
    g = (c.g if g is None else g).to(dev).to(y.dtype)
    if not c.second:
        g_x, g_p = torch.autograd.grad(y, [x, m.params], g)
        return dict(y=y.detach(), dx=g_x, dp=g_p)
    g = g.requires_grad_(True)
    g_x, g_p = torch.autograd.grad(y, [x, m.params], g, create_graph=True)
    d2p, u = torch.autograd.grad(g_x, [m.params, g], (c.v if v is None else v).to(dev))
    return dict(y=y.detach(), dx=g_x.detach(), dp=g_p.detach(), u=u, d2p=d2p)


def wanted(c, r):
    """The restatement's numbers under the names of :func:`run_module`."""
    w = dict(y=r.f["y"], dx=r.b["dx"], dp=r.dp)
    if c.second:
        w.update(u=r.s["u"], d2p=r.d2p)
    return w


def check(got, want, tag, rows=None):
    """Every array of ``want`` by class and bits (only row ``rows`` of the per-point arrays where given)."""
    for k, w in want.items():
        a = got[k]
        if rows is not None and k not in ("dp", "d2p"):
            a, w = a[rows], w[rows]
        assert E.same_class_and_bits(a, w), f"{k}: {tag}: {E.explain(a, w)}"


def bits(t):
    kind = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.detach().cpu().contiguous().clone().view(kind)


def check_isolation(clean, dirty, p, tag, keys):
    """Every row but p has the same bits in the clean and in the poisoned run."""
    for k in keys:
        for a, b in zip(clean[k] if isinstance(clean[k], list) else [clean[k]], dirty[k] if isinstance(dirty[k], list) else [dirty[k]]):
            keep = torch.arange(a.shape[0]) != p
            assert torch.equal(bits(a)[keep], bits(b)[keep]), f"{k}: a row other than {p} changed: {tag}"


# ---------------------------------------------------------------- the helpers themselves

def test_the_restatements_matmul_is_ieee():
    assert E.matmul_is_ieee()


def test_same_class_and_bits():
    a = torch.tensor([1.0, E.NAN, E.INF, -E.INF, 0.0, 65504.0])
    assert E.same_class_and_bits(a, a.clone()) and E.same_class_and_bits(a.half(), a.double())
    assert E.same_class_and_bits(torch.tensor([-0.0]), torch.tensor([0.0]))
    for i, v in [(0, 1.0000001), (1, 0.0), (1, E.INF), (2, -E.INF), (2, 65504.0), (3, E.NAN), (4, E.NAN), (5, E.INF), (5, 65472.0)]:
        b = a.clone()
        b[i] = v
        assert not E.same_class_and_bits(b, a) and not E.same_class_and_bits(a, b), (i, v)
        assert E.explain(b, a) != "equal"
    assert not E.same_class_and_bits(a[:5], a)


# ---------------------------------------------------------------- scaled exact cases

SCALED = [(net, dtype, which) for net in E.NETS for dtype in E.DTYPES for which in ("underflow", "overflow")
          if not (which == "underflow" and dtype == BF16)]


@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("net,dtype,which", SCALED, ids=lambda v: v if isinstance(v, str) else dt(v))
def test_scaled(net, dtype, which, f32_ends):
    """The conditions of the scale set on the restatement (mlp_edges_reference.scale_conditions), then the torch path."""
    cases = E.scaled_cases(net, dtype, which, f32_ends)
    audits, restated = [], []
    for i, c in enumerate(cases):
        r = E.restate(c)
        restated.append(r)
        audits.append(E.audit(c, r))
        check(run_module(make_module(c), c), wanted(c, r), f"{net} {dt(dtype)} {which}[{i}] {ends(f32_ends)}")
    E.scale_conditions(cases[0], which, audits, restated)


# ---------------------------------------------------------------- boundary rows

@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
@pytest.mark.parametrize("net", list(E.NETS))
def test_boundary(net, dtype, f32_ends):
    for probe in E.boundary_probes(net, f32_ends):
        c = E.boundary_case(net, dtype, f32_ends, probe)
        r = E.restate(c)
        E.boundary_conditions(c, probe, E.audit(c, r))
        check(run_module(make_module(c), c), wanted(c, r), f"{net} {dt(dtype)} {ends(f32_ends)} probe {probe}")


# ---------------------------------------------------------------- poison

def poison_targets(net):
    return ["x", "g"] + (["v"] if E.has_second_order(net) else [])


POISON = [(net, target) for net in E.NETS for target in poison_targets(net)]


def run_poison(net, dtype, f32_ends, target, run, keys):
    """The clean and the poisoned twin through ``run(case, x, g, v) -> dict``: rows other than p keep their bits in the arrays
    ``keys``; row p and the parameter gradients match the restatement of the poisoned input by class and bits."""
    clean = {}
    for N, p, value in E.poison_rows(net):
        c = E.base_case(net, dtype, E.FAMILY.get(net, "dense"), f32_ends, N=N)
        if N not in clean:
            clean[N] = run(c, c.x, c.g, c.v)
        inputs = dict(x=c.x, g=c.g, v=c.v)
        inputs[target] = E.poisoned(inputs[target], p, value)
        dirty = run(c, **inputs)
        tag = f"{net} {dt(dtype)} {ends(f32_ends)} {target}[{p}] = {value}, N = {N}"
        check_isolation(clean[N], dirty, p, tag, keys)
        r = E.restate(c, **inputs)
        assert not bool(torch.isfinite(r.dp).all()) or target == "v", f"the poison must reach dL/dparams: {tag}"
        yield c, r, dirty, p, tag


@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
@pytest.mark.parametrize("net,target", POISON)
def test_poison(net, target, dtype, f32_ends):
    modules = {}

    def run(c, x, g, v):
        if c.x.shape[0] not in modules:
            modules[c.x.shape[0]] = make_module(c)
        return run_module(modules[c.x.shape[0]], c, x, g, v)

    keys = ["y", "dx"] + (["u"] if E.has_second_order(net) else [])
    for c, r, dirty, p, tag in run_poison(net, dtype, f32_ends, target, run, keys):
        check(dirty, wanted(c, r), tag, rows=p)


# ---------------------------------------------------------------- a dead neuron under an infinite gradient

@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
def test_dead_neuron(dtype):
    """The mask is a select: 0 at a dead neuron whatever dH (or the tangent) is there.  A mask applied by multiplication gives
    inf * 0 = NaN, in dL/dx, dW_0[1, :] and d2W_2[0, 1]."""
    c = E.dead_neuron_case(dtype)
    r = E.restate(c)
    E.dead_neuron_conditions(c, r, E.audit(c, r))
    check(run_module(make_module(c), c), wanted(c, r), f"dead neuron {dt(dtype)}")


# ---------------------------------------------------------------- the scaler

def scaler_run(device):
    """The steps of mlp_edges_reference.scaler_case on ``device``: the scale before each step, dL/dparams against the
    restatement at that scale, skipped steps that leave p, m, v bit for bit, and the first performed step."""
    ws, x, coef, scales, skips = E.scaler_case()
    assert skips >= 2 and scales[0] == 2.0 ** E.SCALER_LOG2_SCALE
    mlp = FusedMLP(*E.SCALER_SHAPE, dtype=F16, out_dtype=F32)
    mlp.load_linear_weights(ws)
    mlp = mlp.to(device)
    c = E.custom_case("scaler", "plain", F16, E.SCALER_SHAPE, ws, x, coef, x, True, False)
    scaler = DeviceGradScaler(scales[0], growth_interval=None)
    opt = FusedAdam(mlp.parameters(), lr=1e-2, scaler=scaler)
    x, coef, p = x.to(device), coef.to(device), mlp.params
    state = lambda: [bits(p)] + [bits(opt.state[p][k]) for k in ("exp_avg", "exp_avg_sq") if k in opt.state[p]]
    for i, s in enumerate(scales):
        assert scaler.get_scale() == s and scaler.skipped_steps() == i and opt.performed_steps() == 0
        before = state()
        p.grad = None
        scaler.scale((mlp(x) * coef).sum()).backward()
        want = E.restate(c, g=coef.cpu() * s).dp
        assert E.same_class_and_bits(p.grad, want), f"dL/dparams at scale {s}: {E.explain(p.grad, want)}"
        assert bool(torch.isfinite(want).all()) == (i == skips)
        opt.step()
        after = state()
        if i < skips:
            assert scaler.skipped_steps() == i + 1 and scaler.get_scale() == s / 2 and opt.performed_steps() == 0
            assert torch.equal(after[0], before[0]), f"a skipped step moved the parameters (scale {s})"
            assert all(not bool(t.any()) for t in after[1:]), f"a skipped step moved the moments (scale {s})"
    assert i == skips and scaler.skipped_steps() == skips and scaler.get_scale() == scales[skips] and opt.performed_steps() == 1
    assert bool(torch.isfinite(p).all()) and not torch.equal(after[0], before[0]) and len(after) == 3 and bool(after[1].any())


def test_scaler_skips_an_overflow_born_in_the_backward_cpu():
    scaler_run("cpu")


# ---------------------------------------------------------------- a broken restatement is caught

def broken_rnd(kind):
    real = R.rnd

    def rnd(t, dtype, exact=False):
        r = real(t, dtype, exact)
        if dtype == F32:
            return r
        if kind == "saturate":
            return r.clamp(-E.HALF_MAX[dtype], E.HALF_MAX[dtype])
        return torch.where(r.abs() < E.F16_MIN_NORMAL, torch.zeros_like(r), r) if dtype == F16 else r
    return rnd


@pytest.mark.parametrize("kind,which", [("saturate", "overflow"), ("flush", "underflow")])
def test_a_restatement_that_saturates_or_flushes_is_caught(monkeypatch, kind, which):
    """With ``rnd`` clamped to +-MAX the overflow cases and the boundary rows no longer agree with the torch path, and with the
    subnormals zeroed the underflow cases do not: the tables reach what they are for."""
    cases = E.scaled_cases("plain-64x2", F16, which, False)
    if kind == "saturate":
        cases.append(E.boundary_case("plain-64x2", F16, False, "H1"))
    got = [run_module(make_module(c), c) for c in cases]
    for c, o in zip(cases, got):
        check(o, wanted(c, E.restate(c)), "unbroken")
    for mod in (R, S, Q):
        monkeypatch.setattr(mod, "rnd", broken_rnd(kind))
    assert G.R is R
    for c, o in zip(cases, got):
        want = wanted(c, E.restate(c))
        with pytest.raises(AssertionError, match="broken"):
            check(o, want, "broken")
