"""CPU: nerfacc_amd.mlp.FusedMLP's torch path against the float64 reference of tests/mlp_reference.py (within the derived
bound on random data, bit for bit on the integer-valued data), the weight exchange with nn.Linear, the state dict, the
initialisation, mlp_from_tcnn_config, the refusals, and the four C entries' argument checks through the loaded library."""
import ctypes as C
import math

import pytest
import torch
from torch import nn

import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, image_elems, mlp_from_tcnn_config, wgrad_slices

DTYPES = [torch.float16, torch.bfloat16]


def make(n_in, n_out, width, n_hidden, dtype, weights, out_dtype=None):
    m = FusedMLP(n_in, n_out, width, n_hidden, dtype=dtype, out_dtype=out_dtype)
    m.load_linear_weights(weights)
    return m


def run_module(m, x, g):
    x = x.clone().requires_grad_(True)
    m.params.grad = None
    y = m(x)
    y.backward(g.to(y.dtype))
    return y.detach(), x.grad, m.params.grad.clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.NGP_SHAPES)
@pytest.mark.parametrize("out_f32", [False, True])
def test_torch_path_within_the_bound(dtype, shape, out_f32):
    n_in, n_out, width, n_hidden = shape
    ws = R.xavier_weights(*shape, seed=3)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(257, n_in, generator=gen)
    g = torch.randn(257, n_out, generator=gen)
    m = make(*shape, dtype, ws, torch.float32 if out_f32 else None)
    y, g_x, g_p = run_module(m, x, g)
    assert y.dtype == (torch.float32 if out_f32 else dtype) and g_x.dtype == torch.float32 and g_p.dtype == torch.float32
    f = R.forward(x, ws, dtype, out_f32)
    assert R.worst_ratio(y, f["y"], f["e_y"]) <= 1.0
    # the backward is compared on the module's own hidden activations: recompute them as the module rounds them
    from nerfacc_amd.mlp import _forward_torch
    hidden = [h.double() for h in _forward_torch(x, ws, dtype, out_f32)[1]]
    b = R.backward(x, ws, hidden, g.to(y.dtype), dtype)
    assert R.worst_ratio(g_x, b["dx"], b["e_dx"]) <= 1.0
    assert R.worst_ratio(g_p, R.flat(b["dw"]), R.flat(b["e_dw"])) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["perm", "dense"])
@pytest.mark.parametrize("width,n_hidden", [(64, 1), (64, 2), (128, 4)])
def test_torch_path_is_exact_on_integer_data(dtype, family, width, n_hidden):
    for N, n_in, n_out, x_f32, out_f32 in [(33, 31, 3, True, False), (129, 32, 16, False, True)]:
        ws = R.exact_weights(family, n_in, n_out, width, n_hidden)
        x, g = R.exact_inputs(N, n_in, n_out, torch.float32 if x_f32 else dtype, torch.float32 if out_f32 else dtype)
        f = R.forward(x, ws, dtype, out_f32, exact=True)
        b = R.backward(x, ws, f["hidden"], g, dtype, exact=True)
        y, g_x, g_p = run_module(make(n_in, n_out, width, n_hidden, dtype, ws, torch.float32 if out_f32 else None), x, g)
        assert torch.equal(y.double(), f["y"]) and torch.equal(g_x.double(), b["dx"]) and g_x.dtype == x.dtype
        assert torch.equal(g_p.double(), R.flat(b["dw"]))


def test_linear_exchange_and_state_dict():
    m = FusedMLP(31, 3, 64, 2, dtype=torch.bfloat16)
    seq = nn.Sequential(nn.Linear(31, 64, bias=False), nn.ReLU(), nn.Linear(64, 64, bias=False), nn.ReLU(), nn.Linear(64, 3, bias=False))
    lin = [l for l in seq if isinstance(l, nn.Linear)]
    m.load_linear_weights([l.weight.detach() for l in lin])
    for k, l in enumerate(lin):
        assert torch.equal(m.weight(k), l.weight) and m.weight(k).shape == l.weight.shape
        assert m.weight(k).data_ptr() == m.params.data_ptr() + 4 * m._offsets[k]   # a view of the flat parameter
    assert m.params.dtype == torch.float32 and m.params.numel() == 31 * 64 + 64 * 64 + 64 * 3
    assert [n for n, _ in m.named_parameters()] == ["params"]
    # ... and back
    m2 = FusedMLP(31, 3, 64, 2, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(9))
    for l, w in zip(lin, m2.linear_weights()):
        with torch.no_grad():
            l.weight.copy_(w)
    x = torch.randn(17, 31)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        want = seq(x)
    got = m2(x)
    assert got.dtype == torch.bfloat16 and torch.allclose(got.float(), want.float(), atol=0.05, rtol=0.05)
    with pytest.raises(ValueError, match="matrix 1"):
        m.load_linear_weights([lin[0].weight, lin[0].weight, lin[2].weight])
    # state dict
    m3 = FusedMLP(31, 3, 64, 2, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(11))
    assert not torch.equal(m3.params, m2.params)
    m3.load_state_dict(m2.state_dict())
    assert torch.equal(m3.params, m2.params) and torch.equal(m3(x), got)


def test_init_statistics_and_generator():
    a = FusedMLP(32, 16, 64, 1, generator=torch.Generator().manual_seed(1))
    b = FusedMLP(32, 16, 64, 1, generator=torch.Generator().manual_seed(1))
    c = FusedMLP(32, 16, 64, 1, generator=torch.Generator().manual_seed(2))
    assert torch.equal(a.params, b.params) and not torch.equal(a.params, c.params)
    assert torch.equal(FusedMLP(32, 16).params, FusedMLP(32, 16).params)   # the default generator is seeded
    m = FusedMLP(128, 32, 128, 3, generator=torch.Generator().manual_seed(4))
    for l in range(m.n_layers):
        w = m.weight(l).detach()
        bound = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))   # Xavier uniform: U(-bound, bound), variance bound^2 / 3
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.98 * bound
        assert abs(float(w.mean())) < 4 * bound / math.sqrt(3 * w.numel())
        assert abs(float(w.var()) / (bound ** 2 / 3) - 1) < 0.1


def test_tcnn_config():
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}
    m = mlp_from_tcnn_config(32, 16, cfg)
    assert isinstance(m, FusedMLP) and (m.n_neurons, m.n_hidden_layers, m.dtype) == (64, 1, torch.float16)
    assert mlp_from_tcnn_config(32, 3, dict(cfg, n_neurons=128, n_hidden_layers=4), dtype=torch.bfloat16).dtype == torch.bfloat16
    for key, value in [("otype", "CutlassMLP"), ("activation", "Sigmoid"), ("output_activation", "ReLU"), ("n_neurons", 256),
                       ("n_neurons", 32), ("n_hidden_layers", 5), ("n_hidden_layers", 0), ("feedback_alignment", True)]:
        with pytest.raises(ValueError, match=key):
            mlp_from_tcnn_config(32, 16, dict(cfg, **{key: value}))
    with pytest.raises(ValueError, match="n_hidden_layers"):   # tcnn's default depth (5) is not supported
        mlp_from_tcnn_config(32, 16, {k: v for k, v in cfg.items() if k != "n_hidden_layers"})


def test_constructor_refusals_and_lds_budget():
    for kw, match in [(dict(n_neurons=256), "n_neurons"), (dict(n_hidden_layers=5), "n_hidden_layers"), (dict(n_input_dims=257), "n_input_dims"),
                      (dict(n_input_dims=0), "n_input_dims"), (dict(n_output_dims=33), "n_output_dims"), (dict(dtype=torch.float32), "dtype"),
                      (dict(out_dtype=torch.float64), "out_dtype")]:
        args = dict(n_input_dims=32, n_output_dims=16)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            FusedMLP(**args)
    # 128 wide, 4 hidden layers, 256 inputs: 64 + 3 * 32 + 8 KiB of weights do not fit 160 KiB beside the staging tiles
    fwd, bwd = image_elems(256, 32, 128, 4)
    assert fwd * 2 == (64 + 96 + 8) * 1024 and bwd * 2 == (64 + 96 + 8) * 1024
    with pytest.raises(ValueError, match=f"{fwd * 2} B.*{bwd * 2} B.*163840 B"):
        FusedMLP(256, 32, 128, 4)
    FusedMLP(256, 32, 128, 3)   # fits
    FusedMLP(150, 32, 128, 3)
    with pytest.raises(ValueError, match="x must be"):
        FusedMLP(32, 16)(torch.zeros(4, 31))
    with pytest.raises(TypeError, match="float32 or the network"):
        FusedMLP(32, 16, dtype=torch.float16)(torch.zeros(4, 32, dtype=torch.bfloat16))


def test_second_order_raises():
    m = FusedMLP(16, 3, 64, 1)
    x = torch.randn(8, 16, requires_grad=True)
    (g_x,) = torch.autograd.grad(m(x).float().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="second order"):
        g_x.sum().backward()


def test_empty_batch_and_autocast_cpu():
    m = FusedMLP(16, 3, 64, 1, dtype=torch.bfloat16)
    x = torch.zeros(0, 16, requires_grad=True)
    y = m(x)
    assert y.shape == (0, 3) and y.dtype == torch.bfloat16
    y.sum().backward()
    assert x.grad.shape == (0, 16) and torch.equal(m.params.grad, torch.zeros_like(m.params))
    x = torch.randn(9, 16)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        a = m(x)
    assert torch.equal(a, m(x))


def test_wgrad_slices():
    assert [wgrad_slices(n) for n in (1, 64, 129, 300, 1000, 2 ** 20)] == [1, 1, 1, 2, 4, 256]


# ---------------------------------------------------------------- the C entries' checks (nothing reaches a GPU)

P = 0x1000   # a stand-in address that is never dereferenced
F16, BF16, F32 = 1, 2, 0


def _calls(elem=F16, n=64, n_in=32, n_out=16, width=64, n_hidden=2, x=P, img=P, y=P, x_elem=F32, y_elem=None, part=10 ** 9):
    y_elem = elem if y_elem is None else y_elem
    fe, be = image_elems(n_in, n_out, width, n_hidden) if (width in (64, 128) and 1 <= n_hidden <= 4 and n_in > 0 and n_out > 0) else (0, 0)
    lib = B.load()
    return {
        "nfa_mlp_pack_weights": lambda: lib.nfa_mlp_pack_weights(elem, x, n_in, n_out, width, n_hidden, img, fe, y, be, None),
        "nfa_mlp_fwd": lambda: lib.nfa_mlp_fwd(elem, x, x_elem, img, n, n_in, n_out, width, n_hidden, y, y_elem, None, 0, None),
        "nfa_mlp_bwd_data": lambda: lib.nfa_mlp_bwd_data(elem, x, x_elem, P, img, n, n_in, n_out, width, n_hidden, y, None, None, x_elem, None),
        "nfa_mlp_bwd_weights": lambda: lib.nfa_mlp_bwd_weights(elem, x, x_elem, P, P, P, n, n_in, n_out, width, n_hidden, y, part, img, None),
    }


ENTRIES = ["nfa_mlp_pack_weights", "nfa_mlp_fwd", "nfa_mlp_bwd_data", "nfa_mlp_bwd_weights"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,msg", [
    (dict(elem=F32), b"elem 0"), (dict(elem=7), b"elem 7"), (dict(width=96), b"width 96"), (dict(width=256), b"width 256"),
    (dict(n_hidden=0), b"n_hidden 0"), (dict(n_hidden=5), b"n_hidden 5"), (dict(n_in=0), b"n_in 0"), (dict(n_in=257), b"n_in 257"),
    (dict(n_out=0), b"n_out 0"), (dict(n_out=33), b"n_out 33"), (dict(n_in=-3), b"n_in -3"),
    (dict(width=128, n_hidden=4, n_in=256), b"do not fit the LDS"),
    (dict(x=None), b"null pointer"), (dict(img=None), b"null pointer"), (dict(y=None), b"null pointer"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    rc = _calls(**kw)[entry]()
    assert rc == -1 and msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_entry_negative_size_other_dtypes_and_empty(entry):
    lib = B.load()
    assert _calls(n=-1)[entry]() == -1 and b"n_points -1 is negative" in lib.nfa_last_error()
    assert _calls(elem=F16, x_elem=BF16)[entry]() == -1 and b"_elem 2" in lib.nfa_last_error()
    assert _calls(elem=F16, x_elem=5)[entry]() == -1 and b"_elem 5" in lib.nfa_last_error()
    # N = 0 returns 0 with every pointer null
    assert _calls(n=0, x=None, img=None, y=None)[entry]() == 0
    if entry == "nfa_mlp_fwd":
        assert _calls(y_elem=BF16)[entry]() == -1 and b"y_elem 2" in lib.nfa_last_error()
        assert lib.nfa_mlp_fwd(F16, P, F32, P, 64, 32, 16, 64, 2, P, F16, None, 1, None) == -1 and b"null pointer" in lib.nfa_last_error()
        assert lib.nfa_mlp_fwd(F16, P, F32, P + 8, 64, 32, 16, 64, 2, P, F16, None, 0, None) == -1 and b"misaligned" in lib.nfa_last_error()
    if entry == "nfa_mlp_bwd_weights":
        assert _calls(part=-1)[entry]() == -1 and b"partial_floats -1" in lib.nfa_last_error()
        assert _calls(n=1000, part=4 * 7168 - 1)[entry]() == -1 and b"4 slices of 7168 parameters need 28672" in lib.nfa_last_error()


def test_pack_checks_the_image_sizes():
    lib = B.load()
    fe, be = image_elems(32, 16, 64, 2)
    assert (fe, be) == ((4 + 8 + 4) * 512, (4 + 8 + 2) * 512)
    assert lib.nfa_mlp_pack_weights(F16, P, 32, 16, 64, 2, P, fe - 512, P, be, None) == -1
    assert f"hold {fe} and {be} elements".encode() in lib.nfa_last_error()
    assert lib.nfa_mlp_pack_weights(F16, P, 32, 16, 64, 2, P + 4, fe, P, be, None) == -1 and b"16-byte aligned" in lib.nfa_last_error()
