"""GPU: the native sinusoidal encoding (csrc/sinenc.hip) -- forward, backward and second order against the float64
restatement of tests/sinusoidal_reference.py within the accuracy contract stated there, the fixture recorded from the
reference, half element types, freq_weights, var, and one pass through a NeRF-shaped MLP."""
import pytest
import torch
from torch import nn

import sinusoidal_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SECOND_ORDER = [(3, 0, 10, True), (3, 0, 4, True), (3, 0, 16, True), (1, 0, 4, True)]
HALF_EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}   # half an ulp (2^-10, 2^-7 of the binade) over the value


def _enc(cfg, **kw):
    from nerfacc_amd.encodings import SinusoidalEncoding
    return SinusoidalEncoding(*cfg, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _seed(cfg, n=0):
    return 1000 * cfg[0] + 37 * cfg[2] + 11 * (cfg[1] + 16) + n


def _weights(L, dev):
    return torch.linspace(0.25, 1.5, L).to(dev) if L > 1 else torch.tensor([0.75], device=dev)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_forward_within_the_contract(dev, cfg):
    D, lo, hi, ident = cfg
    enc = _enc(cfg)
    for n in R.POINT_COUNTS:
        x = R.draw(n, D, _seed(cfg, n))
        y = enc(x.to(dev))
        assert y.shape == (n, enc.latent_dim) and y.dtype == torch.float32 and y.is_cuda
        R.assert_within(y, R.encode(x, lo, hi, ident), R.forward_bound(x, lo, hi, ident), f"{cfg} n={n}")
        if ident:
            assert torch.equal(_bits(y[:, :D]), _bits(x.to(dev)))


@pytest.mark.parametrize("cfg", [(3, 0, 10, True), (3, 0, 16, True), (4, -2, 6, False)])
def test_forward_large_arguments_and_edge_row(dev, cfg):
    D, lo, hi, ident = cfg
    enc = _enc(cfg)
    x = R.draw(257, D, _seed(cfg), span=1000.0)
    edge = torch.tensor([0.0, -0.0, 1e-40, 1.0])[:D]
    x = torch.cat([x, edge[None]])
    y = enc(x.to(dev))
    R.assert_within(y, R.encode(x, lo, hi, ident), R.forward_bound(x, lo, hi, ident), f"{cfg}")
    if ident:
        assert torch.equal(_bits(y[:, :D]), _bits(x.to(dev)))   # -0.0 and the denormal included


def test_forward_batch_shape_and_non_contiguous_input(dev):
    cfg = (3, 0, 10, True)
    enc = _enc(cfg)
    x = R.draw(35, 3, 5).to(dev)
    flat = enc(x)
    y = enc(x.view(5, 7, 3))
    assert y.shape == (5, 7, 63) and torch.equal(_bits(y.view(35, 63)), _bits(flat))
    wide = torch.zeros(35, 5, device=dev)
    wide[:, 1:4] = x
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    assert torch.equal(_bits(enc(view)), _bits(flat))
    t = x.t().contiguous().t()   # column-major
    assert not t.is_contiguous() and torch.equal(_bits(enc(t)), _bits(flat))


def test_fixture_of_the_reference(dev):
    """The reference's own outputs: its sine block is the same function (two accurate float32 sines: 2^-22 covers both
    roundings), its cosine block carries the rounding of the phase xb + pi/2, 2^-22 max(1, |xb|)."""
    g = load_golden("sinusoidal")
    for i in range(int(g["n_cases"])):
        D, lo, hi, ident = (int(v) for v in g[f"c{i}_cfg"])
        x, want = torch.from_numpy(g[f"c{i}_x"]), torch.from_numpy(g[f"c{i}_y"])
        y = _enc((D, lo, hi, bool(ident)))(x.to(dev)).cpu()
        L, o = hi - lo, D if ident else 0
        xb = (x.double()[:, None, :] * R.scales(lo, hi)[:, None]).flatten(-2)
        if ident:
            assert torch.equal(_bits(y[:, :D]), _bits(want[:, :D]))
        R.assert_within(y[:, o:o + L * D], want[:, o:o + L * D], torch.full_like(xb, R.U), f"case {i} sine")
        R.assert_within(y[:, o + L * D:], want[:, o + L * D:], R.U * xb.abs().clamp(min=1.0), f"case {i} cosine")


# ----------------------------------------------------------------------------- half element types
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cfg", [(3, 0, 10, True), (2, 0, 4, True), (4, -2, 6, False)])
def test_half_outputs_are_the_float32_result_rounded_once(dev, cfg, dtype):
    D = cfg[0]
    full, half = _enc(cfg), _enc(cfg, out_dtype=dtype)
    for n in (1, 63, 65, 1000):
        x = R.draw(n, D, _seed(cfg, n)).to(dev)
        y = half(x)
        assert y.dtype == dtype and torch.equal(_bits(y), _bits(full(x).to(dtype))), (cfg, n)


def test_autocast_and_half_gradients(dev):
    cfg = (3, 0, 10, True)
    x = R.draw(1000, 3, 9).to(dev)
    auto = _enc(cfg, out_dtype="autocast")
    assert auto(x).dtype == torch.float32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = auto(x)
        plain = _enc(cfg)(x)
    assert y.dtype == torch.bfloat16 and plain.dtype == torch.float32
    assert torch.equal(_bits(y), _bits(plain.to(torch.bfloat16)))
    # a half gradient is read as halves: the same float32 arithmetic on the widened values
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.randn(1000, 63, generator=torch.Generator().manual_seed(3)).to(dev).to(dtype)
        xh = x.clone().requires_grad_(True)
        (gh,) = torch.autograd.grad(_enc(cfg, out_dtype=dtype)(xh), xh, g)
        xf = x.clone().requires_grad_(True)
        (gf,) = torch.autograd.grad(_enc(cfg)(xf), xf, g.float())
        assert gh.dtype == torch.float32 and torch.equal(_bits(gh), _bits(gf))


# ----------------------------------------------------------------------------- backward
def _reference_grads(cfg, x, g, var=None, w=None):
    D, lo, hi, ident = cfg
    x64 = x.double().requires_grad_(True)
    v64 = None if var is None else var.double().requires_grad_(True)
    y = R.encode(x64, lo, hi, ident, v64, w)
    return torch.autograd.grad(y, (x64,) if v64 is None else (x64, v64), g.double())


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_backward_within_the_contract_and_reproducible(dev, cfg):
    D, lo, hi, ident = cfg
    enc = _enc(cfg)
    for n in R.POINT_COUNTS[1:]:
        x = R.draw(n, D, _seed(cfg, n))
        g = torch.randn(n, enc.latent_dim, generator=torch.Generator().manual_seed(n))
        xd = x.to(dev).requires_grad_(True)
        (gx,) = torch.autograd.grad(enc(xd), xd, g.to(dev))
        (want,) = _reference_grads(cfg, x, g)
        R.assert_within(gx, want, R.grad_bounds(x, g, lo, hi, ident)[0], f"{cfg} n={n}")
        (again,) = torch.autograd.grad(enc(xd), xd, g.to(dev))
        assert torch.equal(_bits(gx), _bits(again))


def test_backward_large_arguments(dev):
    cfg = (3, 0, 10, True)
    x = R.draw(300, 3, 21, span=1000.0)
    g = torch.randn(300, 63, generator=torch.Generator().manual_seed(4))
    xd = x.to(dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(_enc(cfg)(xd), xd, g.to(dev))
    R.assert_within(gx, _reference_grads(cfg, x, g)[0], R.grad_bounds(x, g, *cfg[1:])[0], "|x| <= 1000")


@pytest.mark.parametrize("cfg", [(3, 0, 4, True), (4, -2, 6, False)])
def test_backward_single_column(dev, cfg):
    """One non-zero column of grad_out gives the one term it belongs to, and exact zeros elsewhere."""
    D, lo, hi, ident = cfg
    enc = _enc(cfg)
    L, o, n, p = hi - lo, (D if ident else 0), 70, 66
    x = R.draw(n, D, _seed(cfg))
    xd = x.to(dev).requires_grad_(True)
    for col in range(enc.latent_dim):
        g = torch.zeros(n, enc.latent_dim)
        g[p, col] = 1.5
        (gx,) = torch.autograd.grad(enc(xd), xd, g.to(dev))
        gx = gx.cpu()
        if col < o:
            d, want = col, 1.5
        else:
            c = col - o
            is_cos, k, d = c >= L * D, (c % (L * D)) // D, c % D
            s = 2.0 ** (lo + k)
            xb = torch.tensor(s * float(x[p, d]), dtype=torch.float64)
            want = float(1.5 * s * (-torch.sin(xb) if is_cos else torch.cos(xb)))
            bound = float(R.grad_bounds(x, g, lo, hi, ident)[0][p, d])
            assert abs(float(gx[p, d]) - want) <= bound, (col, float(gx[p, d]), want, bound)
        if col < o:
            assert float(gx[p, d]) == want
        gx[p, d] = 0.0
        assert (gx == 0).all(), col


# ----------------------------------------------------------------------------- freq_weights
@pytest.mark.parametrize("cfg", [(3, 0, 10, True), (1, 0, 4, True), (4, -2, 6, False)])
def test_freq_weights(dev, cfg):
    from nerfacc_amd.encodings import barf_window
    D, lo, hi, ident = cfg
    L, o, n = hi - lo, (D if ident else 0), 1000
    enc = _enc(cfg)
    x = R.draw(n, D, _seed(cfg))
    g = torch.randn(n, enc.latent_dim, generator=torch.Generator().manual_seed(8))
    xd = x.to(dev).requires_grad_(True)

    def run(w):
        y = enc(xd, freq_weights=w)
        return y, torch.autograd.grad(y, xd, g.to(dev))[0]

    y0, gx0 = run(None)
    y1, gx1 = run(torch.ones(L, device=dev))
    assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(_bits(gx0), _bits(gx1))
    # a zero weight: exact zeros in its columns, no contribution to grad_x
    w = _weights(L, dev)
    w[1] = 0.0
    y, gx = run(w)
    for blk in (o, o + L * D):
        assert (y[:, blk + D: blk + 2 * D] == 0).all()
    g_masked = g.clone()
    for blk in (o, o + L * D):
        g_masked[:, blk + D: blk + 2 * D] = 1e30   # would dominate grad_x if it leaked
    y2 = enc(xd, freq_weights=w)
    assert torch.equal(_bits(torch.autograd.grad(y2, xd, g_masked.to(dev))[0]), _bits(gx))
    # BARF's window at a fractional alpha (exact in float32), against float64: the roundings of pi t <= pi, of the cosine
    # and of 1 - cos <= 2, halved, stay below 2^-22
    wb = barf_window(torch.tensor(L * 0.4375, device=dev), L)
    assert wb.is_cuda and torch.allclose(wb.double().cpu(), R.barf_window(L * 0.4375, L), rtol=0, atol=2.0 ** -22)
    assert ((wb > 0) & (wb < 1)).any()
    yb, gxb = run(wb)
    wc = wb.cpu()
    R.assert_within(yb, R.encode(x, lo, hi, ident, None, wc), R.forward_bound(x, lo, hi, ident, None, wc), "barf forward")
    R.assert_within(gxb, _reference_grads(cfg, x, g, None, wc)[0], R.grad_bounds(x, g, lo, hi, ident, None, wc)[0], "barf backward")
    assert not wb.requires_grad


def test_freq_weights_are_read_through_their_pointer(dev):
    cfg = (3, 0, 4, True)
    enc = _enc(cfg)
    x = R.draw(64, 3, 2).to(dev)
    w = torch.ones(4, device=dev)
    y1 = enc(x, freq_weights=w)
    w[2:] = 0.0
    y2 = enc(x, freq_weights=w)
    assert torch.equal(y1[:, :9], y2[:, :9]) and (y2[:, 9:15] == 0).all() and (y2[:, 21:27] == 0).all() and (y1[:, 21:27] != 0).any()


# ----------------------------------------------------------------------------- var (integrated positional encoding)
@pytest.mark.parametrize("cfg", [(3, 0, 10, True), (2, 0, 4, True), (4, -2, 6, False)])
def test_var(dev, cfg):
    D, lo, hi, ident = cfg
    enc = _enc(cfg)
    for n in (65, 1000):
        x = R.draw(n, D, _seed(cfg, n))
        g = torch.randn(n, enc.latent_dim, generator=torch.Generator().manual_seed(n + 1))
        xd = x.to(dev).requires_grad_(True)
        # var = 0 is the plain result, bit for bit
        y0 = enc(xd)
        yz = enc(xd, var=torch.zeros(n, D, device=dev))
        assert torch.equal(_bits(y0), _bits(yz))
        assert torch.equal(_bits(torch.autograd.grad(y0, xd, g.to(dev))[0]), _bits(torch.autograd.grad(yz, xd, g.to(dev))[0]))
        var = torch.rand(n, D, generator=torch.Generator().manual_seed(n + 2)) * 0.1
        vd = var.to(dev).requires_grad_(True)
        y = enc(xd, var=vd)
        R.assert_within(y, R.encode(x, lo, hi, ident, var), R.forward_bound(x, lo, hi, ident, var), f"{cfg} forward")
        if ident:
            assert torch.equal(_bits(y[:, :D]), _bits(xd.detach()))
        gx, gv = torch.autograd.grad(y, (xd, vd), g.to(dev))
        want_x, want_v = _reference_grads(cfg, x, g, var)
        bx, bv = R.grad_bounds(x, g, lo, hi, ident, var)
        R.assert_within(gx, want_x, bx, f"{cfg} grad_x")
        R.assert_within(gv, want_v, bv, f"{cfg} grad_var")
        # var alone requires a gradient
        (gv2,) = torch.autograd.grad(enc(x.to(dev), var=vd), vd, g.to(dev))
        assert torch.equal(_bits(gv2), _bits(gv))


def test_second_order_with_var_raises(dev):
    enc = _enc((3, 0, 4, True))
    x = R.draw(10, 3, 1).to(dev).requires_grad_(True)
    var = torch.full((10, 3), 0.01, device=dev)
    (gx,) = torch.autograd.grad(enc(x, var=var).sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="SinusoidalEncoding: the second order"):
        gx.sum().backward()


# ----------------------------------------------------------------------------- second order
def _second_order(enc, x, g, v, w):
    y = enc(x, freq_weights=w)
    (gx,) = torch.autograd.grad(y, x, g, create_graph=True)
    return torch.autograd.grad((gx * v).sum(), (x, g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", SECOND_ORDER)
def test_second_order(dev, cfg, dtype):
    D, lo, hi, ident = cfg
    L = hi - lo
    enc = _enc(cfg, out_dtype=dtype)
    for n in (1, 65, 1000):
        for use_w in (False, True):
            x = R.draw(n, D, _seed(cfg, n))
            g = torch.randn(n, enc.latent_dim, generator=torch.Generator().manual_seed(n + 5)).to(dtype)
            v = torch.randn(n, D, generator=torch.Generator().manual_seed(n + 6))
            if n == 65:
                v = torch.zeros(n, D)   # gg_x with one non-zero component
                v[64, D - 1] = 2.0
            w = _weights(L, dev) if use_w else None
            wc = None if w is None else w.cpu()
            xd, gd = x.to(dev).requires_grad_(True), g.to(dev).requires_grad_(True)
            d_x, d_g = _second_order(enc, xd, gd, v.to(dev), w)
            assert d_x.dtype == torch.float32 and d_g.dtype == dtype
            x64, g64 = x.double().requires_grad_(True), g.double().requires_grad_(True)
            y64 = R.encode(x64, lo, hi, ident, None, wc)
            (gx64,) = torch.autograd.grad(y64, x64, g64, create_graph=True)
            w_x, w_g = torch.autograd.grad((gx64 * v.double()).sum(), (x64, g64))
            b_g, b_x = R.second_order_bounds(x, g, v, lo, hi, ident, wc)
            if dtype != torch.float32:
                b_g = b_g + HALF_EPS[dtype] * w_g.abs()   # the one rounding of the stored half
            R.assert_within(d_x, w_x, b_x, f"{cfg} n={n} w={use_w} towards x")
            R.assert_within(d_g, w_g, b_g, f"{cfg} n={n} w={use_w} towards grad_out")
            if ident:
                assert torch.equal(d_g[:, :D].float().cpu(), v.to(dtype).float())
            if n == 65:
                assert (d_x[:64] == 0).all() and (d_x[64, :D - 1] == 0).all() and (d_g[:64] == 0).all() and (d_g[64] != 0).any()
            again = _second_order(enc, xd, gd, v.to(dev), w)
            assert torch.equal(_bits(again[0]), _bits(d_x)) and torch.equal(_bits(again[1]), _bits(d_g))


# ----------------------------------------------------------------------------- a NeRF-shaped field
class _VanillaNeRF(nn.Module):
    """The layer layout of the reference's VanillaNeRFRadianceField (8 layers with a skip at 4, a sigma head, a bottleneck
    joined by the encoded view direction, one conditioned layer, the rgb head) at a small width."""

    def __init__(self, width=32):
        super().__init__()
        self.posi_encoder, self.view_encoder = _enc((3, 0, 10, True)), _enc((3, 0, 4, True))
        d_in = self.posi_encoder.latent_dim
        self.layers = nn.ModuleList(nn.Linear(d_in if i == 0 else width + (d_in if i == 5 else 0), width) for i in range(8))
        self.sigma = nn.Linear(width, 1)
        self.bottleneck = nn.Linear(width, width)
        self.cond = nn.Linear(width + self.view_encoder.latent_dim, width // 2)
        self.rgb = nn.Linear(width // 2, 3)

    def forward(self, x, dirs):
        e = self.posi_encoder(x)
        h = e
        for i, layer in enumerate(self.layers):
            h = torch.relu(layer(h))
            if i == 4:
                h = torch.cat([h, e], -1)
        sigma = self.sigma(h)
        h = torch.cat([self.bottleneck(h), self.view_encoder(dirs)], -1)
        return torch.sigmoid(self.rgb(torch.relu(self.cond(h)))), sigma


def test_field_shaped_use(dev):
    torch.manual_seed(0)
    field = _VanillaNeRF().to(dev)
    assert field.posi_encoder.latent_dim == 63 and field.view_encoder.latent_dim == 27
    x = R.draw(257, 3, 3).to(dev).requires_grad_(True)
    dirs = torch.nn.functional.normalize(R.draw(257, 3, 4), dim=-1).to(dev).requires_grad_(True)
    rgb, sigma = field(x, dirs)
    assert rgb.shape == (257, 3) and sigma.shape == (257, 1)
    (rgb.square().sum() + sigma.sum()).backward()
    for t in (x, dirs, field.layers[0].weight, field.layers[5].weight, field.cond.weight):
        assert t.grad is not None and torch.isfinite(t.grad).all() and (t.grad != 0).any()
    assert x.grad.shape == (257, 3) and dirs.grad.shape == (257, 3)
