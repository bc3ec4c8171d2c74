"""CPU: FusedMLP with biases and skip connections (the reference's MLP class).  The module's torch restatement against the
float64 reference of tests/mlp_bias_skip_reference.py, bit for bit on integer-valued data, and against float64 torch.autograd
through a plain nn.Linear / torch.cat / ReLU stack that needs none of the formulas; the parameter layout; the refusals of the
constructor, of reference_mlp and of the C entries (decided on the host, nothing reaches a GPU); and the golden fixture made
from the reference's own MLP class (tests/golden/ref_mlp.npz, scripts/gen_mlp_golden.py)."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import mlp_bias_skip_reference as S
from conftest import ROOT
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, image_elems, layer_dims, lds_bias_bytes, mlp_from_tcnn_config, reference_mlp, skip_mask_of

DTYPES = [torch.float16, torch.bfloat16]
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_mlp.npz")


def v_mod_of(case):
    """The mod-3 tangent input cancels on the dense first matrix of the 150-input cases (tests/mlp_grad2_reference.py: configs)."""
    return 7 if case[5][1] == 150 else 3


def make(shape, dtype, ws, bs, skip_layer, out_f32, second_order=True, device="cpu"):
    m = FusedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None, second_order=second_order, bias=bs is not None,
                 skip_layer=skip_layer)
    m.load_linear_weights(ws, bs)
    return m.to(device)


def first_and_second_order(m, x, g, v):
    """(y, dL/dx, dL/dparams, u, ds/dparams, ds/dx) of the module, s = <v, dL/dx>."""
    dev = m.params.device
    x = x.to(dev).requires_grad_(True)
    y = m(x)
    g = g.to(dev).to(y.dtype).requires_grad_(True)
    g_x, g_p = torch.autograd.grad(y, [x, m.params], g, create_graph=True)
    s_p, u, s_x = torch.autograd.grad((g_x * v.to(dev)).sum(), [m.params, g, x], allow_unused=True)
    return y.detach(), g_x.detach(), g_p.detach(), u, s_p, s_x


def stack_float64(x, ws, bs, skip_layer, g, v):
    """float64 torch.autograd through nn.Linear / torch.cat / ReLU, the reference's forward written out: (y, dx, [dW], [db],
    u, [ds/dW], [ds/db], ds/dx)."""
    lin = [nn.Linear(w.shape[1], w.shape[0], bias=bs is not None, dtype=torch.float64) for w in ws]
    with torch.no_grad():
        for l, layer in enumerate(lin):
            layer.weight.copy_(ws[l].double())
            if bs is not None:
                layer.bias.copy_(bs[l].double())
    xd = x.double().clone().requires_grad_(True)
    gd = g.double().clone().requires_grad_(True)
    h = xd
    for i, layer in enumerate(lin[:-1]):
        h = torch.relu(layer(h))
        if skip_layer is not None and i % skip_layer == 0 and i > 0:
            h = torch.cat([h, xd], dim=-1)
    y = lin[-1](h)
    params = [l.weight for l in lin] + ([l.bias for l in lin] if bs is not None else [])
    g_x, *g_p = torch.autograd.grad(y, [xd] + params, gd, create_graph=True)
    s = (g_x * v.double()).sum()
    u, s_x, *s_p = torch.autograd.grad(s, [gd, xd] + params, allow_unused=True)
    n = len(lin)
    return y.detach(), g_x.detach(), [t.detach() for t in g_p[:n]], [t.detach() for t in g_p[n:]], u, s_p[:n], s_p[n:], s_x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: f"{c[0]}-W{c[1]}-L{c[2]}-skip{c[3]}-bias{int(c[4])}-N{c[5][0]}-in{c[5][1]}-out{c[5][2]}")
def test_exact_against_the_reference_and_autograd(case, dtype):
    family, width, n_hidden, skip_layer, bias, cfg = case
    shape, skip_mask, ws, bs, x, g, v, f, b, s = S.exact_case(family, dtype, width, n_hidden, cfg, bias, skip_layer, v_mod_of(case))
    n_bias = sum(w.shape[0] for w in ws) if bias else 0
    if cfg[0] >= 31:   # a pass that writes zeros cannot agree
        assert bool(f["y"].any()) and bool(b["dx"].any()) and bool(s["u"].any()) and bool(S.flat_params(s["dw"]).any())
        # g of mlp_reference.exact_inputs has period 5 in the point index and sums to zero over it: db_L is zero when 5 | N
        assert all(bool(d.any()) for d in b["db"][:-1]) and (bool(b["db"][-1].any()) or cfg[0] % 5 == 0)
    m = make(shape, dtype, ws, bs, skip_layer, cfg[4])
    assert m.skip_mask == skip_mask and [tuple(w.shape) for w in ws] == layer_dims(*shape, skip_mask)
    y, g_x, g_p, u, s_p, s_x = first_and_second_order(m, x, g, v)
    assert y.dtype == (torch.float32 if cfg[4] else dtype) and g_x.dtype == x.dtype and g_p.dtype == torch.float32
    assert torch.equal(y.double(), f["y"])
    assert torch.equal(g_x.double(), b["dx"])
    assert torch.equal(g_p.double(), S.flat_params(b["dw"], b["db"] if bias else None))
    assert torch.equal(u.double(), s["u"])
    assert s_p.shape == g_p.shape and torch.equal(s_p.double(), torch.cat([S.flat_params(s["dw"]), torch.zeros(n_bias, dtype=torch.float64)]))
    assert s_x is None
    # float64 autograd through a plain stack: nothing rounds on this data, so it must give the same numbers
    ay, adx, adw, adb, au, asw, asb, asx = stack_float64(x, ws, bs, skip_layer, g, v)
    assert torch.equal(ay, f["y"]) and torch.equal(adx, b["dx"])
    assert torch.equal(S.flat_params(adw, adb if bias else None), g_p.double())
    assert torch.equal(au, s["u"]) and torch.equal(S.flat_params(asw), S.flat_params(s["dw"]))
    assert all(t is None or not bool(t.any()) for t in asb) and (asx is None or not bool(asx.any()))


def test_biases_change_the_masks():
    """The -40 entries switch neurons off: the masks differ from the bias-free network's."""
    family, width, n_hidden, skip_layer, _, cfg = S.CASES[8]
    with_b = S.exact_case(family, torch.float16, width, n_hidden, cfg, True, skip_layer)[7]["hidden"]
    without = S.exact_case(family, torch.float16, width, n_hidden, cfg, False, skip_layer)[7]["hidden"]
    for a, b_ in zip(with_b, without):
        assert not torch.equal(a > 0, b_ > 0)
        assert not bool((a[:, (torch.arange(width) % 8 == 5)] > 0).all())


def test_defaults_are_the_network_as_before():
    for shape in [(32, 16, 64, 1), (32, 3, 64, 2), (40, 32, 128, 4)]:
        old = FusedMLP(*shape)
        new = FusedMLP(*shape, bias=False, skip_layer=None)
        assert torch.equal(old.params, new.params) and old._offsets == new._offsets and old.skip_mask == 0 and not new.bias_enabled
        assert old.params.numel() == sum(o * i for o, i in layer_dims(*shape))
        x = torch.randn(37, shape[0], generator=torch.Generator().manual_seed(3))
        assert torch.equal(old(x), new(x))
        assert "bias" not in repr(old) and "skip" not in repr(old)
    # with biases the matrices come first, drawn in the same order with the true fan-in, then the biases, zero
    m = FusedMLP(36, 3, 64, 4, bias=True, skip_layer=2, generator=torch.Generator().manual_seed(5))
    dims = layer_dims(36, 3, 64, 4, skip_mask_of(2, 4))
    assert dims == [(64, 36), (64, 64), (64, 64), (64, 100), (3, 64)]
    gen = torch.Generator().manual_seed(5)
    want = [(torch.rand(o * i, generator=gen) * 2.0 - 1.0) * (6.0 / (o + i)) ** 0.5 for o, i in dims]
    n_w = sum(o * i for o, i in dims)
    assert torch.equal(m.params[:n_w], torch.cat(want)) and torch.equal(m.params[n_w:], torch.zeros(4 * 64 + 3))
    assert m.weight(3).shape == (64, 100) and m.bias(4).shape == (3,) and m.bias(0).data_ptr() == m.params.data_ptr() + 4 * n_w
    assert "bias=True" in repr(m) and "skip_layer=2" in repr(m)
    assert [skip_mask_of(s, 4) for s in (None, 1, 2, 3, 4)] == [0, 0b11100, 0b01000, 0b10000, 0]
    assert skip_mask_of(2, 3) == 0b1000 and skip_mask_of(1, 1) == 0
    with pytest.raises(ValueError, match="no biases"):
        FusedMLP(32, 16).bias(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_skip_layer_that_selects_nothing_is_the_plain_chain(dtype):
    gen = lambda: torch.Generator().manual_seed(9)
    a = FusedMLP(36, 3, 64, 4, dtype=dtype, bias=True, skip_layer=4, second_order=True, generator=gen())
    b = FusedMLP(36, 3, 64, 4, dtype=dtype, bias=True, second_order=True, generator=gen())
    c = FusedMLP(36, 3, 64, 4, dtype=dtype, skip_layer=7, generator=gen())
    d = FusedMLP(36, 3, 64, 4, dtype=dtype, generator=gen())
    assert a.skip_mask == 0 and torch.equal(a.params, b.params) and torch.equal(c.params, d.params)
    with torch.no_grad():
        for m in (a, b):
            m.params[m._offsets[-1]:].copy_(torch.linspace(-0.5, 0.5, 4 * 64 + 3))
    g = torch.Generator().manual_seed(1)
    x, gy, v = torch.randn(50, 36, generator=g), torch.randn(50, 3, generator=g), torch.randn(50, 36, generator=g)
    for got, want in zip(first_and_second_order(a, x, gy, v)[:5], first_and_second_order(b, x, gy, v)[:5]):
        assert torch.equal(got, want)
    assert torch.equal(c(x), d(x))


def test_linear_and_reference_state_dict_round_trip():
    m = reference_mlp(36, 3, net_depth=4, net_width=64, skip_layer=2, generator=torch.Generator().manual_seed(2))
    assert isinstance(m, FusedMLP) and m.bias_enabled and m.skip_layer == 2 and (m.n_neurons, m.n_hidden_layers) == (64, 4)
    with torch.no_grad():
        m.params[m._offsets[-1]:].uniform_(-1, 1)
    ws, bs = m.linear_weights(), m.linear_biases()
    assert [tuple(w.shape) for w in ws] == [(64, 36), (64, 64), (64, 64), (64, 100), (3, 64)] and [b.numel() for b in bs] == [64] * 4 + [3]
    sd = {}
    for i in range(4):
        sd[f"hidden_layers.{i}.weight"], sd[f"hidden_layers.{i}.bias"] = ws[i], bs[i]
    sd["output_layer.weight"], sd["output_layer.bias"] = ws[4], bs[4]
    m2 = reference_mlp(36, 3, net_depth=4, net_width=64, skip_layer=2)
    assert not torch.equal(m2.params, m.params)
    m2.load_reference_state_dict(sd)
    assert torch.equal(m2.params, m.params)
    m3 = FusedMLP(36, 3, 64, 4, bias=True, skip_layer=2)
    m3.load_linear_weights(ws, bs)
    assert torch.equal(m3.params, m.params)
    m3.load_linear_weights([w * 2 for w in ws])   # biases stay
    assert torch.equal(m3.params[m3._offsets[-1]:], m.params[m._offsets[-1]:])
    with pytest.raises(ValueError, match="output_layer.bias"):
        m2.load_reference_state_dict({k: t for k, t in sd.items() if k != "output_layer.bias"})
    with pytest.raises(ValueError, match="unexpected keys .*extra"):
        m2.load_reference_state_dict(dict(sd, extra=ws[0]))
    with pytest.raises(ValueError, match="matrix 3"):
        m2.load_reference_state_dict(dict(sd, **{"hidden_layers.3.weight": ws[2]}))
    with pytest.raises(ValueError, match="bias 4"):
        m2.load_linear_weights(ws, bs[:4] + [bs[0]])
    with pytest.raises(ValueError, match="without biases"):
        FusedMLP(36, 3, 64, 4, skip_layer=2).load_linear_weights(ws, bs)
    no_bias = reference_mlp(36, 3, 4, 64, 2, bias_enabled=False)
    no_bias.load_reference_state_dict({k: t for k, t in sd.items() if k.endswith("weight")})
    assert torch.equal(no_bias.params, m.params[:m._offsets[-1]]) and no_bias.linear_biases() == []


def test_refusals():
    # a layer that takes [H, x] holds at most 256 inputs
    with pytest.raises(ValueError, match=r"n_input_dims 200 \+ n_neurons 64 = 264.*at most 256"):
        FusedMLP(200, 3, 64, 4, skip_layer=2)
    FusedMLP(192, 3, 64, 4, skip_layer=2)   # 256: fits
    FusedMLP(200, 3, 64, 4, skip_layer=4)   # no layer selected: no limit
    with pytest.raises(ValueError, match=r"n_input_dims 150 \+ n_neurons 128 = 278"):
        FusedMLP(150, 3, 128, 3, skip_layer=1)
    with pytest.raises(ValueError, match="skip_layer 0"):
        FusedMLP(32, 3, 64, 4, skip_layer=0)
    # the LDS budget counts the longer images and the biases: 128 wide, three layers that take [H, x] never fit
    shape = (36, 32, 128, 4)
    fwd, bwd = image_elems(*shape, skip_mask_of(1, 4))
    assert fwd * 2 == (3 * 4 + 32 + 2 * 4 * 11 + 11) * 1024 and bwd * 2 == (2 * 8 + 32 + 2 * 6 * 8 + 6 * 2) * 1024
    with pytest.raises(ValueError, match=f"forward image {fwd * 2} B, backward image {bwd * 2} B.*163840 B.*skip_layer 1"):
        FusedMLP(*shape, skip_layer=1)
    with pytest.raises(ValueError, match=f"forward image {fwd * 2} B with 2176 B of biases, backward image {bwd * 2} B.*163840 B"):
        FusedMLP(*shape, skip_layer=1, bias=True)
    FusedMLP(*shape)
    FusedMLP(*shape, skip_layer=2, bias=True)   # one such layer fits
    # images come in blocks of 1 KiB and 143.5 KiB are free beside the staging tiles, so the at most 2,176 B of biases never
    # decide alone; they are counted all the same (the message above), and the widest network that fits still fits with them
    assert image_elems(256, 32, 128, 3)[0] * 2 == 136 * 1024 and lds_bias_bytes(128, 3, True) == 1664 and lds_bias_bytes(128, 3, False) == 0
    FusedMLP(256, 32, 128, 3, bias=True)
    # reference_mlp names the argument
    for kw, match in [(dict(net_depth=0), "net_depth"), (dict(net_depth=5), "net_depth"), (dict(net_depth=8), "net_depth"),
                      (dict(net_width=256), "net_width"), (dict(net_width=32), "net_width"), (dict(output_enabled=False), "output_enabled"),
                      (dict(hidden_activation="Softplus"), "hidden_activation"), (dict(output_activation="Sigmoid"), "output_activation")]:
        args = dict(input_dim=36, output_dim=3, net_depth=4, net_width=64, skip_layer=2)
        args.update(kw)
        with pytest.raises(ValueError, match=f"'{match}'"):
            reference_mlp(**args)
    # tcnn has neither feature
    m = mlp_from_tcnn_config(32, 16, {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2})
    assert not m.bias_enabled and m.skip_mask == 0
    with pytest.raises(ValueError, match="bias"):
        mlp_from_tcnn_config(32, 16, {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2, "bias": True})


# ---------------------------------------------------------------- the C entries' checks (nothing reaches a GPU)

P = 0x1000   # a stand-in address that is never dereferenced
F16, BF16, F32 = 1, 2, 0
ENTRIES = ["nfa_mlp_net_pack_weights", "nfa_mlp_net_fwd", "nfa_mlp_net_bwd_data", "nfa_mlp_net_bwd_weights", "nfa_mlp_net_tangent"]


def _calls(elem=F16, n=64, n_in=36, n_out=3, width=64, n_hidden=4, bias=1, skip_mask=8, x=P, img=P, y=P, x_elem=F32, part=10 ** 9,
           bias_ptr=P, desc=True):
    lib = B.load()
    d = B.MLPDesc(n_in, n_out, width, n_hidden, bias, skip_mask) if desc else None
    try:
        fe, be = image_elems(n_in, n_out, width, n_hidden, skip_mask)
    except Exception:
        fe = be = 0
    return {
        "nfa_mlp_net_pack_weights": lambda: lib.nfa_mlp_net_pack_weights(elem, d, x, img, fe, y, be, None),
        "nfa_mlp_net_fwd": lambda: lib.nfa_mlp_net_fwd(elem, d, x, x_elem, img, bias_ptr, n, y, elem, None, 0, None),
        "nfa_mlp_net_bwd_data": lambda: lib.nfa_mlp_net_bwd_data(elem, d, x, x_elem, P, img, n, y, None, None, x_elem, None),
        "nfa_mlp_net_bwd_weights": lambda: lib.nfa_mlp_net_bwd_weights(elem, d, x, x_elem, P, P, P, n, y, part, img, 0, None),
        "nfa_mlp_net_tangent": lambda: lib.nfa_mlp_net_tangent(elem, d, x, x_elem, P, img, n, None, y, elem, None),
    }


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,msg", [
    (dict(desc=False), b"descriptor is null"), (dict(elem=F32), b"elem 0"), (dict(width=96), b"width 96"), (dict(n_hidden=0, skip_mask=0), b"n_hidden 0"),
    (dict(n_hidden=5), b"n_hidden 5"), (dict(n_in=0), b"n_in 0"), (dict(n_in=257), b"n_in 257"), (dict(n_out=33), b"n_out 33"),
    (dict(bias=2), b"bias 2"), (dict(bias=-1), b"bias -1"),
    (dict(skip_mask=1), b"skip_mask 0x1"), (dict(skip_mask=2), b"skip_mask 0x2"), (dict(skip_mask=32), b"skip_mask 0x20"),
    (dict(n_hidden=1, skip_mask=4), b"skip_mask 0x4"), (dict(n_hidden=3, skip_mask=16), b"skip_mask 0x10"),
    (dict(n_in=200), b"n_in 200 + width 64 = 264"), (dict(n_in=150, width=128), b"n_in 150 + width 128 = 278"),
    (dict(n_out=32, width=128, skip_mask=28, bias=0), b"do not fit the LDS: forward image 146432 B with 0 B of biases, backward image 159744 B"),
    (dict(n_out=32, width=128, skip_mask=28), b"do not fit the LDS: forward image 146432 B with 2176 B of biases, backward image 159744 B"),
    (dict(x=None), b"null pointer"), (dict(img=None), b"null pointer"), (dict(y=None), b"null pointer"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    rc = _calls(**kw)[entry]()
    assert rc == -1 and msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()


def test_entry_sizes_and_empty():
    lib = B.load()
    for entry in ENTRIES[1:]:
        assert _calls(n=-1)[entry]() == -1 and b"n_points -1 is negative" in lib.nfa_last_error()
        assert _calls(n=0, x=None, img=None, y=None, bias_ptr=None)[entry]() == 0   # N = 0 returns 0 with every pointer null
    assert _calls(bias_ptr=None)["nfa_mlp_net_fwd"]() == -1 and b"null pointer" in lib.nfa_last_error()
    assert _calls(bias_ptr=P + 2)["nfa_mlp_net_fwd"]() == -1 and b"misaligned" in lib.nfa_last_error()
    # the T-NeRF warp network: 36*64 + 2*64*64 + 100*64 + 64*3 matrices and 4*64 + 3 biases
    n_params = 36 * 64 + 2 * 64 * 64 + 100 * 64 + 64 * 3 + 259
    assert FusedMLP(36, 3, 64, 4, bias=True, skip_layer=2).params.numel() == n_params == 17347
    assert _calls(n=1000, part=4 * n_params - 1)["nfa_mlp_net_bwd_weights"]() == -1
    assert f"4 slices of {n_params} parameters need {4 * n_params}".encode() in lib.nfa_last_error()
    fe, be = image_elems(36, 3, 64, 4, 8)
    assert (fe, be) == ((2 * 3 + 8 + 8 + 2 * 7 + 4) * 512, (2 * 4 + 8 + 8 + 4 * 4 + 2) * 512)
    assert lib.nfa_mlp_net_pack_weights(F16, B.MLPDesc(36, 3, 64, 4, 1, 8), P, P, fe - 512, P, be, None) == -1
    assert f"hold {fe} and {be} elements".encode() in lib.nfa_last_error()


# ---------------------------------------------------------------- the golden fixture: the reference's own MLP class

def golden(name):
    z = np.load(GOLDEN)
    pre = name + "/"
    d = {k[len(pre):]: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith(pre)}
    meta = {k: int(t) for k, t in d.items() if k in ("input_dim", "output_dim", "net_depth", "net_width", "skip_layer")}
    # weights, x and g are stored as integer numerators (scale 1 in the exact cases)
    sd = {k[len("sd/"):]: (t / d["w_scale"] if k.endswith("weight") else t).float() for k, t in d.items() if k.startswith("sd/")}
    d["x"], d["g"] = d["x"] / d["x_scale"], d["g"] / d["x_scale"]
    return meta, sd, d


def golden_module(meta, sd, dtype, out_f32, device="cpu", second_order=False):
    m = reference_mlp(meta["input_dim"], meta["output_dim"], meta["net_depth"], meta["net_width"], meta["skip_layer"] or None, dtype=dtype,
                      out_dtype=torch.float32 if out_f32 else None, second_order=second_order)
    m.load_reference_state_dict(sd)
    return m.to(device)


def golden_grads(m, d, x_dtype):
    dev = m.params.device
    x = d["x"].to(x_dtype).to(dev).requires_grad_(True)
    y = m(x)
    g_x, g_p = torch.autograd.grad(y, [x, m.params], d["g"].to(y.dtype).to(dev))
    names = [f"hidden_layers.{i}" for i in range(m.n_hidden_layers)] + ["output_layer"]
    want_p = torch.cat([d[f"grad/{n}.weight"].reshape(-1) for n in names] + [d[f"grad/{n}.bias"].reshape(-1) for n in names])
    return y.detach().cpu(), g_x.cpu(), g_p.cpu(), want_p


GOLDEN_NETS = ["warp", "wide"]   # T-NeRF's warp network 36 -> 4 x 64 -> 3 with skip_layer 2; 40 -> 128 -> 3 without skip


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", GOLDEN_NETS)
def test_golden_exact(net, dtype):
    """Integer weights: the reference's float64 numbers are exact in the half types, so the module must give them bit for bit.
    This pins the cat order, the skip rule and the key names to the reference itself."""
    meta, sd, d = golden(net + "_exact")
    assert float(d["y"].abs().max()) > 0 and float(d["dx"].abs().max()) > 0
    y, g_x, g_p, want_p = golden_grads(golden_module(meta, sd, dtype, True), d, torch.float32)
    assert torch.equal(y.double(), d["y"]) and torch.equal(g_x.double(), d["dx"]) and torch.equal(g_p.double(), want_p)


def golden_bound(meta, sd, d, dtype, n_hidden, skip_mask):
    """The float64 restatement at the kernels' rounding points and its bound on the distance between half-precision passes
    and the reference's UNROUNDED float64 numbers (mlp_bias_skip_reference: ``free``), plus a float32 ulp: the fixture stores
    the reference's results as float32.  Returns (y bound, dx bound, flat dparams bound)."""
    names = [f"hidden_layers.{i}" for i in range(n_hidden)] + ["output_layer"]
    ws, bs = [sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names]
    x, g = d["x"].float(), d["g"].float()
    for t in ws + [x, g]:   # both half types hold the inputs exactly: no input rounding separates the two sides
        assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)
    f = S.forward(x, ws, bs, skip_mask, dtype, True)
    b = S.backward(x, ws, f["hidden"], g, skip_mask, dtype, free=f)
    stored = lambda t: S.ulp(torch.float32, t.abs())
    e_p = S.flat_params(b["e_dw"], b["e_db"])
    return f["e_y"] + stored(f["y"]), b["e_dx"] + stored(b["dx"]), e_p + stored(S.flat_params(b["dw"], b["db"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", GOLDEN_NETS)
def test_golden_xavier_within_the_bound(net, dtype):
    """Xavier weights: the module against the reference's float64 numbers, within the derived bound."""
    meta, sd, d = golden(net + "_xavier")
    m = golden_module(meta, sd, dtype, True)
    e_y, e_dx, e_p = golden_bound(meta, sd, d, dtype, m.n_hidden_layers, m.skip_mask)
    y, g_x, g_p, want_p = golden_grads(m, d, torch.float32)
    ratios = dict(y=S.worst_ratio(y, d["y"], e_y), dx=S.worst_ratio(g_x, d["dx"], e_dx), dparams=S.worst_ratio(g_p, want_p, e_p))
    print(f"golden {net} {dtype} error/bound ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
