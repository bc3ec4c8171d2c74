"""GPU: the hash grid's second order on the native op nfa_hashgrid_bwd_bwd[_t] -- ``torch.autograd.grad(enc(x), x, g,
create_graph=True)`` followed by a backward of the resulting dL/dx: that it works and which native calls it makes, the three
gradients against the float64 restatement of tests/hashgrid2_reference.py, reproducibility, the optional outputs, fp16 / bf16
gradients, empty input, the refused derivative of dL/dparams, and an Eikonal loss trained end to end.

The bound: per element (k + 8) * 2^-23 * sum|term|, k the number of summed terms (for a table entry: the number of
contributions it received).  Each term is a product of at most six float32 roundings, each of the k additions adds at most
2^-24 of a running sum that sum|term| bounds; the bound is twice that worst case, as the first-order test's
(cnt + 2) * 2^-23 * absum is."""
import functools

import numpy as np
import pytest
import torch

from hashgrid2_reference import interior_points, restate_grad2
from nerfacc_amd import _backend as B
from nerfacc_amd.encodings import HashGridEncoding, _HashGridBwdFn

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
NS = [1, 63, 65, 4097]
# (n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale): the small entries of
# tests/test_encodings_gpu.py's CONFIGS
CONFIGS = {
    "F1_L1": (1, 1, 14, 16, 2.0),          # one level: no cross-lane sum
    "F1_L32": (32, 1, 12, 16, 1.3),        # 2 points per wave
    "F2_L24": (24, 2, 16, 16, 1.2),        # 16 idle lanes per wave
    "F4_L3": (3, 4, 14, 16, 2.0),          # one idle lane
    "F8_L7_edge": (7, 8, 12, 16, 1.0),     # every level 16^3 = 2^12 entries: exactly on the dense / hashed boundary
    "F2_odd_res": (4, 2, 16, 10.5, 1.5),   # level 0: 11^3 entries, padded to 1336
    "density": (5, 2, 17, 16, np.exp((np.log(128) - np.log(16)) / 4).tolist()),   # NGPDensityField
}
CASES = [pytest.param(kind, n, id=f"{n}-{kind}") for kind in CONFIGS for n in NS]


class CallLog:
    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self):
        return [n for n, _ in self.calls]


def make_grid(kind, out_dtype=None):
    torch.manual_seed(0)
    L, F, log2, base, scale = CONFIGS[kind]
    enc = HashGridEncoding(3, L, F, log2, base, scale, out_dtype=out_dtype)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc


def boundary_points(n, seed, enc):
    """n points in [-0.25, 1.25]^3 with rows on cell boundaries of every level (x * scale_l + 0.5 an integer in float32) and
    the 0.0 / 1.0 corners (tests/test_encodings_gpu.py: with_cell_boundaries)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 1.5 - 0.25
    rows = []
    for s in enc.scales:
        k = torch.arange(0, int(s) + 2, dtype=torch.float32)
        c = (k - 0.5) / s
        c = c[(c * s + 0.5) == torch.floor(c * s + 0.5)]
        if c.numel():
            rows.append(c[torch.randint(0, c.numel(), (max(n // (4 * len(enc.scales)), 1), 3), generator=g)])
    rows.append(torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.5], [0.0, 0.0, 0.0]]))
    b = torch.cat(rows)[: max(n - 1, 1)]
    if n > 1:
        x[1: 1 + b.shape[0]] = b[: n - 1]
    else:
        x[0] = torch.tensor([1.0, 1.0, 1.0])
    return x


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(grid on the CPU, x, g, gg_x, the float64 restatement): computed once per (config, n), never modified."""
    enc = make_grid(kind)
    x = boundary_points(n, n, enc)
    gen = torch.Generator().manual_seed(100 + n)
    g = torch.randn(n, enc.n_output_dims, generator=gen)
    v = torch.randn(n, 3, generator=gen)
    return enc, x, g, v, restate_grad2(x, enc.params.detach(), enc, g, v)


def second_order(enc, x, g, v, need_g=True):
    """enc on the device; returns (x2, G2_T or None, gg_y or None, dL/dx) of one double-backward step."""
    dev = enc.params.device
    enc.params.grad = None
    xd = x.to(dev).requires_grad_(True)
    gd = g.to(dev).requires_grad_(need_g)
    (g_x,) = torch.autograd.grad(enc(xd), xd, gd, create_graph=True)
    g_x.backward(v.to(dev))
    return xd.grad, enc.params.grad, gd.grad, g_x.detach()


def within(got, ref, k, absum, extra=8):
    err = (got.detach().cpu().double() - ref).abs()
    bound = (k + extra) * 2.0 ** -23 * absum
    assert bool((err <= bound).all()), (float((err - bound).max()), int((err > bound).sum()))


def check_against_restatement(r, x2, g2_p, gg_y):
    if gg_y is not None:
        within(gg_y, r["gg_y"], r["gg_y_k"], r["gg_y_abs"])
    if x2 is not None:
        within(x2, r["x2"], r["x2_k"], r["x2_abs"])
    if g2_p is not None:
        F = g2_p.numel() // r["hits"].numel()
        within(g2_p, r["g2_params"], r["hits"].repeat_interleave(F), r["g2_params_abs"])


# ---------------------------------------------------------------- it works, natively
@pytest.mark.parametrize("d", [torch.float32] + HALF)
def test_double_backward_runs_on_the_native_path(dev, monkeypatch, d):
    enc = make_grid("density", None if d == torch.float32 else d).to(dev)
    x = boundary_points(1000, 1, enc).to(dev).requires_grad_(True)
    g = torch.randn(1000, enc.n_output_dims, device=dev).to(d)
    v = torch.randn(1000, 3, device=dev)
    log = CallLog(monkeypatch)
    (g_x,) = torch.autograd.grad(enc(x), x, g, create_graph=True)
    assert g_x.requires_grad and g_x.shape == (1000, 3)
    g_x.backward(v)
    torch.cuda.synchronize()
    t = "" if d == torch.float32 else "_t"
    assert log.names() == ["nfa_hashgrid_fwd" + t, "nfa_hashgrid_bwd" + t, "nfa_hashgrid_bwd_bwd" + t], log.names()
    assert x.grad.shape == (1000, 3) and enc.params.grad.shape == enc.params.shape
    assert bool(torch.isfinite(x.grad).all()) and float(enc.params.grad.abs().sum()) > 0


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("kind,n", CASES)
def test_against_float64_restatement(dev, kind, n):
    enc, x, g, v, r = case(kind, n)
    encd = make_grid(kind).to(dev)
    x2, g2_p, gg_y, _ = second_order(encd, x, g, v)
    assert x2.shape == (n, 3) and gg_y.shape == g.shape and g2_p.shape == enc.params.shape
    check_against_restatement(r, x2, g2_p, gg_y)
    if n == 4097:
        assert int((r["hits"] > 0).sum()) > 1000
        assert int((g2_p != 0).sum()) > 1000


# ---------------------------------------------------------------- reproducibility, optional outputs
@pytest.mark.parametrize("kind", list(CONFIGS))
def test_reproducible_and_optional_outputs(dev, monkeypatch, kind):
    n = 4097
    enc, x, g, v, r = case(kind, n)
    encd = make_grid(kind).to(dev)
    x2, g2_p, gg_y, g_x = second_order(encd, x, g, v)
    g2_p = g2_p.clone()
    # twice the same: gg_y and x2 bit for bit, the table gradient within the bound (the order of the atomic adds varies)
    x2b, g2_pb, gg_yb, _ = second_order(encd, x, g, v)
    assert torch.equal(x2b, x2) and torch.equal(gg_yb, gg_y)
    check_against_restatement(r, None, g2_pb, None)
    # g does not require grad: no gg_y
    x2c, g2_pc, gg_yc, _ = second_order(encd, x, g, v, need_g=False)
    assert gg_yc is None and torch.equal(x2c, x2)
    check_against_restatement(r, None, g2_pc, None)
    # the parameters do not require grad: no table gradient at either order
    encd.params.requires_grad_(False)
    log = CallLog(monkeypatch)
    x2d, g2_pd, gg_yd, _ = second_order(encd, x, g, v)
    assert g2_pd is None and torch.equal(x2d, x2) and torch.equal(gg_yd, gg_y)
    a1, a2 = log.calls[1][1], log.calls[2][1]
    assert log.names()[1:] == ["nfa_hashgrid_bwd", "nfa_hashgrid_bwd_bwd"] and a1[-3] is None and a2[-3] is None
    encd.params.requires_grad_(True)
    # x does not require grad at second order (the first backward as a function of a constant x): no x2
    xd, gd = x.to(dev), g.to(dev).requires_grad_(True)
    encd.params.grad = None
    g_xe, _ = _HashGridBwdFn.apply(xd, encd.params, gd, encd, torch.float32, True, True)
    assert torch.equal(g_xe.detach(), g_x)
    g_xe.backward(v.to(dev))
    assert log.names()[-1] == "nfa_hashgrid_bwd_bwd" and log.calls[-1][1][-2] is None
    assert xd.grad is None and torch.equal(gd.grad, gg_y)
    check_against_restatement(r, None, encd.params.grad, None)
    # only the table gradient: nothing reads the corners
    encd.params.grad = None
    g_xf, _ = _HashGridBwdFn.apply(xd, encd.params, g.to(dev), encd, torch.float32, True, True)
    g_xf.backward(v.to(dev))
    a = log.calls[-1][1]
    assert a[-4] is None and a[-2] is None and a[-3] is not None
    check_against_restatement(r, None, encd.params.grad, None)


# ---------------------------------------------------------------- half gradients
@pytest.mark.parametrize("kind", list(CONFIGS))
@pytest.mark.parametrize("d", HALF)
def test_half_gradients(dev, d, kind):
    n = 4097
    enc, x, g, v, _ = case(kind, n)
    gh = g.to(d)
    ref = make_grid(kind).to(dev)
    x2_32, g2_p32, gg_y32, _ = second_order(ref, x, gh.float(), v)       # the float32 op on the exactly widened gradient
    g2_p32 = g2_p32.clone()
    half = make_grid(kind, d)
    half.params = ref.params
    x2, g2_p, gg_y, _ = second_order(half, x, gh, v)
    assert gg_y.dtype == d and gg_y.shape == g.shape
    assert torch.equal(gg_y, gg_y32.to(d))
    assert torch.equal(x2, x2_32)
    r = restate_grad2(x, enc.params.detach(), enc, gh.float(), v)
    check_against_restatement(r, None, g2_p, None)


# ---------------------------------------------------------------- edge cases
def test_empty_input(dev):
    enc = make_grid("density").to(dev)
    x = torch.zeros(0, 3, device=dev, requires_grad=True)
    g = torch.zeros(0, enc.n_output_dims, device=dev, requires_grad=True)
    (g_x,) = torch.autograd.grad(enc(x), x, g, create_graph=True)
    assert g_x.shape == (0, 3)
    g_x.backward(torch.zeros(0, 3, device=dev))
    assert x.grad.shape == (0, 3) and g.grad.shape == g.shape and float(enc.params.grad.abs().sum()) == 0.0


def test_gradient_of_the_table_gradient_is_refused(dev):
    enc = make_grid("F4_L3").to(dev)
    x = boundary_points(65, 3, enc).to(dev).requires_grad_(True)
    g = torch.randn(65, enc.n_output_dims, device=dev, requires_grad=True)
    (g_p,) = torch.autograd.grad(enc(x), enc.params, g, create_graph=True)
    with pytest.raises(NotImplementedError, match="HashGridEncoding"):
        g_p.sum().backward()


# ---------------------------------------------------------------- an Eikonal loss end to end
def sdf_field():
    torch.manual_seed(0)
    enc = HashGridEncoding(3, 4, 2, 14, 16, 1.5)
    with torch.no_grad():
        enc.params.uniform_(-0.1, 0.1)
    return torch.nn.ModuleList([enc, torch.nn.Linear(8, 1)])


def eikonal_loss(field, x):
    x = x.clone().requires_grad_(True)
    f = field[1](field[0](x))
    (grad,) = torch.autograd.grad(f.sum(), x, create_graph=True)
    return ((grad.norm(dim=-1) - 1.0) ** 2).mean()


def test_eikonal_loss_trains(dev, monkeypatch):
    ref = sdf_field().double()
    x = interior_points(4096, ref[0], seed=5)          # boundary-free: the float32 and float64 cells coincide
    eikonal_loss(ref, x.double()).backward()
    field = sdf_field().to(dev)
    xd = x.to(dev)
    log = CallLog(monkeypatch)
    loss = eikonal_loss(field, xd)
    loss.backward()
    assert log.names() == ["nfa_hashgrid_fwd", "nfa_hashgrid_bwd", "nfa_hashgrid_bwd_bwd"], log.names()
    for got, want in ((field[0].params.grad, ref[0].params.grad), (field[1].weight.grad, ref[1].weight.grad)):
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=1e-3 * float(want.abs().mean()))
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    losses = []
    for _ in range(20):
        loss = eikonal_loss(field, xd)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
