"""CPU: the streamed-weight fused MLP.  The torch restatement behind StreamedMLP against the float64 reference on the
integer-valued cases (bit for bit); the condition that makes those cases worth comparing (they are alive at depth 8); the
limits, in Python and in every nfa_mlp_stream_* entry, by message; the slice rule; the module's contract; NerfMLP against the
golden fixture made from the reference's own class, with and without a condition.  Nothing here reaches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import mlp_bias_skip_reference as S
import mlp_stream_reference as Q
from nerfacc_amd import _backend as B
from nerfacc_amd import mlp as M
from nerfacc_amd.mlp import FusedMLP, NerfMLP, StreamedMLP, image_elems, stream_limits_error, stream_wgrad_slices

DTYPES = [torch.float16, torch.bfloat16]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_nerf_mlp.npz")


def make_stream(shape, dtype, ws, bs, skip_layer, out_f32, device="cpu"):
    m = StreamedMLP(*shape, dtype=dtype, out_dtype=torch.float32 if out_f32 else None, bias=bs is not None, skip_layer=skip_layer)
    m.load_linear_weights(ws, bs)
    return m.to(device)


def grads(m, x, g):
    """(y, dL/dx, dL/dparams) of a real backward."""
    dev = m.params.device
    x = x.to(dev).requires_grad_(True)
    y = m(x)
    g_x, g_p = torch.autograd.grad(y, [x, m.params], g.to(y.dtype).to(dev))
    return y.detach(), g_x, g_p


# ---------------------------------------------------------------- the integer-valued cases

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", Q.CASES + [Q.SWEEP_CASE], ids=Q.case_id)
def test_exact_cpu(case, dtype):
    """Every case the GPU tests run is exactly representable (the reference asserts that every rounding is a no-op), and the
    torch restatement behind a CPU StreamedMLP gives the reference's numbers bit for bit."""
    shape, skip_mask, ws, bs, x, g, f, b = Q.exact_case(case, dtype)
    y, g_x, g_p = grads(make_stream(shape, dtype, ws, bs, case[3], case[5][4]), x, g)
    assert torch.equal(y.double(), f["y"]) and torch.equal(g_x.double(), b["dx"])
    assert torch.equal(g_p.double(), S.flat_params(b["dw"], b["db"] if bs is not None else None))
    assert bool(f["y"].any()) and bool(b["dw"][0].any())


def test_the_covering_set_covers():
    ns = {c[5][0] for c in Q.CASES}
    assert {1, 31, 33, Q.T - 1, Q.T, Q.T + 1, 300} <= ns and Q.SWEEP_CASE[5][0] == Q.GROUPS * Q.T + 2 * 32 + 7
    assert {c[2] for c in Q.CASES} >= {1, 2, Q.SLOTS + 1, 8} and {c[1] for c in Q.CASES} == {128, 256}
    assert {c[5][1] for c in Q.CASES} >= {5, 36, 63, 283, 320} and {c[5][2] for c in Q.CASES} >= {1, 3, 32, 33, 257, 288}
    assert all(c[5][0] <= 300 for c in Q.CASES if c[2] == 8) and Q.SWEEP_CASE[1:3] == (256, 2)
    masks = [(S.skip_mask_of(c[3], c[2]), c[4], c[2]) for c in Q.CASES]
    assert any(m == 0 and b for m, b, _ in masks) and any(m and not b for m, b, _ in masks) and any(m and b for m, b, _ in masks)
    assert any((m >> d) & 1 for m, _, d in masks), "a cat output layer"
    assert any(c[3] is not None and S.skip_mask_of(c[3], c[2]) == 0 for c in Q.CASES), "a skip_layer that selects nothing"
    assert {c[5][3] for c in Q.CASES} == {c[5][4] for c in Q.CASES} == {True, False}
    assert (Q.T, Q.GROUPS, Q.SLOTS) == (M.STREAM_POINTS, M.STREAM_GROUPS, M.STREAM_SLOTS)


def test_the_trunk_cases_are_alive():
    """A comparison of zeros shows nothing.  On the reference alone, for the trunk-shape cases taken together: dL/dx and every
    dZ_l are at least 10 % non-zero in at least one case; every one of the 256 columns of every dZ_l and every 32 x 32 tile
    of every dW_l is non-zero in at least one case."""
    best_dx, best_dz, cols, tiles = 0.0, [0.0] * 8, [torch.zeros(256, dtype=torch.bool) for _ in range(8)], None
    for case in Q.TRUNK_CASES:
        assert case[1:4] == (256, 8, 4) and case[5][1:3] == (63, 257)
        shape, skip_mask, ws, bs, x, g, f, b = Q.exact_case(case, torch.bfloat16)
        best_dx = max(best_dx, float((b["dx"] != 0).double().mean()))
        for l in range(8):
            best_dz[l] = max(best_dz[l], float((b["dz"][l] != 0).double().mean()))
            cols[l] |= (b["dz"][l] != 0).any(0)
        live = []
        for dw in b["dw"]:
            o, i = dw.shape
            padded = torch.zeros(-(-o // 32) * 32, -(-i // 32) * 32, dtype=torch.float64)
            padded[:o, :i] = dw
            live.append((padded.view(padded.shape[0] // 32, 32, padded.shape[1] // 32, 32) != 0).any(3).any(1))
        tiles = live if tiles is None else [a | c for a, c in zip(tiles, live)]
    assert best_dx >= 0.10 and all(v >= 0.10 for v in best_dz), (best_dx, best_dz)
    assert all(bool(c.all()) for c in cols), [int(c.sum()) for c in cols]
    assert all(bool(t.all()) for t in tiles), [int((~t).sum()) for t in tiles]
    assert [tuple(t.shape) for t in tiles] == [(8, 2)] + [(8, 8)] * 4 + [(8, 10)] + [(8, 8)] * 2 + [(9, 8)]


# ---------------------------------------------------------------- limits, slices, constants

def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nerfacc_hip.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("NFA_MLP_STREAM_POINTS") == M.STREAM_POINTS and define("NFA_MLP_STREAM_GROUPS") == M.STREAM_GROUPS
    assert define("NFA_MLP_STREAM_WGRAD_MIN_SLICE") == M.STREAM_WGRAD_MIN_SLICE
    assert define("NFA_MLP_STREAM_WGRAD_MAX_SLICES") == M.STREAM_WGRAD_MAX_SLICES


def test_slice_rule():
    """A function of N alone, at most 16 slices: the trunk's partials stay within a few tens of MB."""
    assert [stream_wgrad_slices(n) for n in (1, 64, 256, 257, 300, 512, 513, 4095, 4096, 4097, 2 ** 18, 2 ** 20)] == \
        [1, 1, 1, 2, 2, 2, 3, 16, 16, 13, 16, 16]   # 4097: 16 slices of 320 points would leave three empty
    assert stream_wgrad_slices(Q.GROUPS * Q.T + 71) == 16
    trunk = StreamedMLP(63, 257)
    assert trunk.params.numel() == 63 * 256 + 4 * 256 * 256 + 319 * 256 + 2 * 256 * 256 + 256 * 257 + 8 * 256 + 257 == 559105
    assert 16 * trunk.params.numel() * 4 < 40e6


def test_constructor_refusals_and_limits():
    for kw, msg in [(dict(n_neurons=64), "width 64: 128 or 256"), (dict(n_neurons=512), "width 512"), (dict(n_hidden_layers=0), "n_hidden 0: 1 to 8"),
                    (dict(n_hidden_layers=9), "n_hidden 9"), (dict(n_input_dims=0), "n_in 0: 1 to 320"), (dict(n_input_dims=321), "n_in 321"),
                    (dict(n_output_dims=0), "n_out 0: 1 to 288"), (dict(n_output_dims=289), "n_out 289"), (dict(skip_layer=0), "skip_layer 0"),
                    (dict(dtype=torch.float32), "dtype torch.float32"), (dict(out_dtype=torch.float64), "out_dtype torch.float64"),
                    (dict(n_neurons=256.0), "n_neurons 256.0: an integer")]:
        args = dict(n_input_dims=63, n_output_dims=257)
        args.update(kw)
        with pytest.raises(ValueError, match="StreamedMLP: .*" + re.escape(msg)):
            StreamedMLP(**args)
    # the corners of what is held; the ring fits for every one of them
    for shape, skip in [((320, 288, 256, 8), 1), ((1, 1, 128, 1), None), ((320, 288, 128, 8), 1), ((63, 257, 256, 8), 4)]:
        m = StreamedMLP(*shape, skip_layer=skip)
        assert stream_limits_error(*shape, 1, m.skip_mask) is None
        assert M.stream_lds_bytes(*shape, 1, m.skip_mask) <= M.LDS_BUDGET
    assert M.stream_piece_bytes(320, 288, 256, 8, S.skip_mask_of(1, 8)) == 36 * 1024
    assert M.stream_lds_bytes(320, 288, 256, 8, 1, S.skip_mask_of(1, 8)) == 2 * 36864 + 16896 + 1280 + (8 * 256 + 288) * 4 == 101248
    assert M.stream_piece_bytes(63, 257, 256, 8, S.skip_mask_of(4, 8)) == 20 * 1024    # the trunk's cat layer
    assert M.stream_piece_bytes(63, 257, 256, 8, 0) == 17 * 1024                       # the backward's first product: 257 outputs
    # the existing classes keep their refusals
    with pytest.raises(ValueError, match="FusedMLP: n_neurons 256"):
        FusedMLP(32, 3, 256, 2)
    with pytest.raises(ValueError, match="FusedMLP: n_hidden_layers 5"):
        FusedMLP(32, 3, 64, 5)


P = 0x1000   # a stand-in address that is never dereferenced
F16, BF16, F32 = 1, 2, 0
ENTRIES = ["nfa_mlp_stream_pack_weights", "nfa_mlp_stream_fwd", "nfa_mlp_stream_bwd_data", "nfa_mlp_stream_bwd_weights"]


def _calls(elem=F16, n=64, n_in=63, n_out=257, width=256, n_hidden=8, bias=1, skip_mask=32, x=P, img=P, y=P, x_elem=F32, part=10 ** 9,
           bias_ptr=P, desc=True):
    lib = B.load()
    d = B.MLPDesc(n_in, n_out, width, n_hidden, bias, skip_mask) if desc else None
    try:
        fe, be = image_elems(n_in, n_out, width, n_hidden, skip_mask)
    except Exception:
        fe = be = 0
    return {
        "nfa_mlp_stream_pack_weights": lambda: lib.nfa_mlp_stream_pack_weights(elem, d, x, img, fe, y, be, None),
        "nfa_mlp_stream_fwd": lambda: lib.nfa_mlp_stream_fwd(elem, d, x, x_elem, img, bias_ptr, n, y, elem, None, 0, None),
        "nfa_mlp_stream_bwd_data": lambda: lib.nfa_mlp_stream_bwd_data(elem, d, x, x_elem, P, img, n, y, None, None, x_elem, None),
        "nfa_mlp_stream_bwd_weights": lambda: lib.nfa_mlp_stream_bwd_weights(elem, d, x, x_elem, P, P, P, n, y, part, img, 0, None),
    }


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,msg", [
    (dict(desc=False), b"descriptor is null"), (dict(elem=F32), b"elem 0"), (dict(width=64), b"width 64: 128 or 256 neurons are supported"),
    (dict(width=192), b"width 192"), (dict(n_hidden=0, skip_mask=0), b"n_hidden 0: 1 to 8 hidden layers"), (dict(n_hidden=9), b"n_hidden 9"),
    (dict(n_in=0), b"n_in 0: 1 to 320 input features"), (dict(n_in=321), b"n_in 321"), (dict(n_out=0), b"n_out 0: 1 to 288 outputs"),
    (dict(n_out=289), b"n_out 289"), (dict(bias=2), b"bias 2: 0 or 1"), (dict(bias=-1), b"bias -1"),
    (dict(skip_mask=1), b"skip_mask 0x1"), (dict(skip_mask=2), b"skip_mask 0x2"), (dict(skip_mask=512), b"skip_mask 0x200"),
    (dict(n_hidden=1, skip_mask=4), b"skip_mask 0x4"), (dict(n_hidden=3, skip_mask=16), b"skip_mask 0x10"),
    (dict(x=None), b"null pointer"), (dict(img=None), b"null pointer"), (dict(y=None), b"null pointer"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    rc = _calls(**kw)[entry]()
    assert rc == -1 and msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()


@pytest.mark.parametrize("kw", [dict(width=64), dict(n_hidden=9), dict(n_in=321), dict(n_out=289), dict(bias=2), dict(skip_mask=3),
                                dict(n_hidden=2, skip_mask=8)])
def test_python_and_the_entries_refuse_in_the_same_words(kw):
    args = dict(n_in=63, n_out=257, width=256, n_hidden=8, bias=1, skip_mask=32)
    args.update(kw)
    want = stream_limits_error(**args)
    lib = B.load()
    assert want and _calls(**kw)["nfa_mlp_stream_fwd"]() == -1
    assert lib.nfa_last_error().decode() == "nfa_mlp_stream_fwd: " + want


def test_entry_sizes_and_empty():
    lib = B.load()
    for entry in ENTRIES[1:]:
        assert _calls(n=-1)[entry]() == -1 and b"n_points -1 is negative" in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error()
        assert _calls(n=0, x=None, img=None, y=None, bias_ptr=None)[entry]() == 0   # N = 0 returns 0 with every pointer null
    assert _calls(bias_ptr=None)["nfa_mlp_stream_fwd"]() == -1 and b"null pointer" in lib.nfa_last_error()
    assert _calls(bias_ptr=P + 2)["nfa_mlp_stream_fwd"]() == -1 and b"misaligned" in lib.nfa_last_error()
    assert _calls(img=P + 8)["nfa_mlp_stream_bwd_data"]() == -1 and b"misaligned" in lib.nfa_last_error()
    assert _calls(x_elem=BF16)["nfa_mlp_stream_fwd"]() == -1 and b"x_elem 2" in lib.nfa_last_error()
    n_params = 559105   # the trunk
    assert _calls(n=1000, part=4 * n_params - 1)["nfa_mlp_stream_bwd_weights"]() == -1
    assert f"4 slices of {n_params} parameters need {4 * n_params}".encode() in lib.nfa_last_error()
    assert _calls(n=2 ** 20, part=16 * n_params - 1)["nfa_mlp_stream_bwd_weights"]() == -1
    assert f"16 slices of {n_params} parameters need {16 * n_params}".encode() in lib.nfa_last_error()
    assert _calls(n=1000, part=-1)["nfa_mlp_stream_bwd_weights"]() == -1 and b"partial_floats -1 is negative" in lib.nfa_last_error()
    fe, be = image_elems(63, 257, 256, 8, 32)
    # layer 0: 8 x 4 blocks; six plain layers 8 x 16; the cat layer 8 x 20; the output layer 9 x 16
    assert fe == (8 * 4 + 6 * 8 * 16 + 8 * 20 + 9 * 16) * 512 and be == (2 * 16 + 6 * 8 * 16 + 10 * 16 + 8 * 17) * 512
    assert lib.nfa_mlp_stream_pack_weights(F16, B.MLPDesc(63, 257, 256, 8, 1, 32), P, P, fe - 512, P, be, None) == -1
    assert f"nfa_mlp_stream_pack_weights: the images hold {fe} and {be} elements".encode() in lib.nfa_last_error()


# ---------------------------------------------------------------- the module's contract

def test_module_contract_cpu():
    gen = torch.Generator().manual_seed(3)
    m = StreamedMLP(63, 257, generator=gen)
    dims = [(256, 63)] + [(256, 256)] * 4 + [(256, 319)] + [(256, 256)] * 2 + [(257, 256)]
    assert [tuple(m.weight(l).shape) for l in range(9)] == dims and m.skip_mask == 32 and m.bias_enabled
    assert m.params.dtype == torch.float32 and m.params.numel() == sum(o * i + o for o, i in dims)
    for l, (o, i) in enumerate(dims):   # Xavier with the true fan-in, biases zero
        bound = (6.0 / (o + i)) ** 0.5
        assert 0.9 * bound < float(m.weight(l).detach().abs().max()) <= bound and not bool(m.bias(l).any())
    assert m.weight(8).data_ptr() == m.params.data_ptr() + 4 * sum(o * i for o, i in dims[:8])
    assert m.bias(0).data_ptr() == m.params.data_ptr() + 4 * sum(o * i for o, i in dims)
    ws, bs = m.linear_weights(), [torch.full((o,), 0.25 * l) for l, (o, _) in enumerate(dims)]
    other = StreamedMLP(63, 257, dtype=torch.bfloat16, out_dtype=torch.float32)
    other.load_linear_weights(ws, bs)
    assert all(torch.equal(a, b) for a, b in zip(other.linear_weights(), ws)) and all(torch.equal(a, b) for a, b in zip(other.linear_biases(), bs))
    names = [f"hidden_layers.{i}" for i in range(8)] + ["output_layer"]
    sd = {n + ".weight": w for n, w in zip(names, ws)} | {n + ".bias": b for n, b in zip(names, bs)}
    third = StreamedMLP(63, 257)
    third.load_reference_state_dict(sd)
    assert torch.equal(third.params, other.params)
    with pytest.raises(ValueError, match="StreamedMLP: load_reference_state_dict: missing keys .*output_layer.bias"):
        third.load_reference_state_dict({k: v for k, v in sd.items() if k != "output_layer.bias"})
    with pytest.raises(ValueError, match="StreamedMLP: matrix 5 is"):
        third.load_linear_weights(ws[:5] + [ws[4]] + ws[6:], bs)
    x = torch.randn(7, 63, generator=gen)
    y = other(x)
    assert y.dtype == torch.float32 and y.shape == (7, 257)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert torch.equal(other(x), y)
    with pytest.raises(ValueError, match=r"StreamedMLP: x must be \[N, 63\]"):
        other(x[:, :5])
    with pytest.raises(TypeError, match="StreamedMLP: x is torch.float16"):
        other(x.half())
    # N = 0
    x0 = torch.zeros(0, 63, requires_grad=True)
    y0 = other(x0)
    y0.sum().backward()
    assert y0.shape == (0, 257) and x0.grad.shape == (0, 63) and not bool(other.params.grad.any())
    # the gradients are not differentiable again, and the message names the class
    xg = x.clone().requires_grad_(True)
    (g_x,) = torch.autograd.grad(other(xg).sum(), xg, create_graph=True)
    with pytest.raises(NotImplementedError, match="StreamedMLP: the second order"):
        g_x.sum().backward()
    assert "StreamedMLP" not in M.__all__ if hasattr(M, "__all__") else True
    import nerfacc_amd
    assert "StreamedMLP" not in nerfacc_amd.__all__ and "NerfMLP" not in nerfacc_amd.__all__


# ---------------------------------------------------------------- NerfMLP

def nerf_golden(name):
    z = np.load(GOLDEN)
    pre = name + "/"
    d = {k[len(pre):]: torch.from_numpy(np.asarray(z[k]).astype(np.float64)) for k in z.files if k.startswith(pre)}
    for k in ("x", "condition", "g_rgb", "g_sigma"):
        d[k] = d[k] / d["x_scale"]
    return d


def nerf_param_grads(m, g_trunk, g_head):
    """The flat gradients of the two networks under the reference's parameter names."""
    D, W = m.trunk.n_hidden_layers, m.net_width
    cond = m.head is not None
    tw, tb = m.trunk._views(g_trunk), m.trunk._bias_views(g_trunk)
    out = {}
    for i in range(D):
        out[f"base.hidden_layers.{i}.weight"], out[f"base.hidden_layers.{i}.bias"] = tw[i], tb[i]
    first, r = ("bottleneck_layer.output_layer", W) if cond else ("rgb_layer.output_layer", 3)
    out[first + ".weight"], out[first + ".bias"] = tw[D][:r], tb[D][:r]
    out["sigma_layer.output_layer.weight"], out["sigma_layer.output_layer.bias"] = tw[D][r:], tb[D][r:]
    if cond:
        hw, hb = m.head._views(g_head), m.head._bias_views(g_head)
        for i in range(m.head.n_hidden_layers):
            out[f"rgb_layer.hidden_layers.{i}.weight"], out[f"rgb_layer.hidden_layers.{i}.bias"] = hw[i], hb[i]
        out["rgb_layer.output_layer.weight"], out["rgb_layer.output_layer.bias"] = hw[-1], hb[-1]
    return out


def nerf_bounds(sd, d, dtype, cond):
    """The bound on the distance between the half-precision passes and the reference's unrounded float64 numbers, by the rule
    of mlp_bias_skip_reference carried through both networks (mlp_stream_reference: *_with_error): the colour head's input
    carries the trunk's output error, the trunk's incoming gradient carries the head's dL/dx error.  Returns dicts of bounds
    for the outputs and for the parameter gradients by reference key, plus a float32 ulp for how the fixture stores them."""
    D, W, mask = 8, 256, S.skip_mask_of(4, 8)
    first = "bottleneck_layer.output_layer" if cond else "rgb_layer.output_layer"
    ws = [sd[f"base.hidden_layers.{i}.weight"] for i in range(D)] + [torch.cat([sd[first + ".weight"], sd["sigma_layer.output_layer.weight"]])]
    bs = [sd[f"base.hidden_layers.{i}.bias"] for i in range(D)] + [torch.cat([sd[first + ".bias"], sd["sigma_layer.output_layer.bias"]])]
    x, c, g_rgb, g_sigma = d["x"], d["condition"], d["g_rgb"], d["g_sigma"]
    for t in ws + [x, c, g_rgb, g_sigma]:   # both half types hold the inputs exactly
        assert torch.equal(t.to(torch.float16).double(), t.double()) and torch.equal(t.to(torch.bfloat16).double(), t.double())
    f_t = S.forward(x.float(), ws, bs, mask, dtype, False)
    zero = lambda t: torch.zeros_like(t)
    e = {}
    if cond:
        ws_c = [sd["rgb_layer.hidden_layers.0.weight"], sd["rgb_layer.output_layer.weight"]]
        bs_c = [sd["rgb_layer.hidden_layers.0.bias"], sd["rgb_layer.output_layer.bias"]]
        h0, e_h0 = torch.cat([f_t["y"][:, :W], c], 1), torch.cat([f_t["e_y"][:, :W], zero(c)], 1)
        f_c = Q.forward_with_error(h0, e_h0, ws_c, bs_c, 0, dtype)
        b_c = Q.backward_with_error(h0, e_h0, ws_c, g_rgb, zero(g_rgb), 0, dtype, f_c, torch.float32)
        e["raw_rgb"], e["raw_sigma"], e["dcondition"] = f_c["e_y"], f_t["e_y"][:, W:], b_c["e_dx"][:, W:]
        g_t, e_g = torch.cat([b_c["dx"][:, :W], g_sigma], 1), torch.cat([b_c["e_dx"][:, :W], zero(g_sigma)], 1)
        vals = {"raw_rgb": f_c["y"], "raw_sigma": f_t["y"][:, W:], "dcondition": b_c["dx"][:, W:]}
    else:
        e["raw_rgb"], e["raw_sigma"] = f_t["e_y"][:, :3], f_t["e_y"][:, 3:]
        g_t, e_g = torch.cat([g_rgb, g_sigma], 1), torch.cat([zero(g_rgb), zero(g_sigma)], 1)
        vals = {"raw_rgb": f_t["y"][:, :3], "raw_sigma": f_t["y"][:, 3:]}
    b_t = Q.backward_with_error(x, zero(x), ws, g_t, e_g, mask, dtype, f_t, torch.float32)
    e["dx"], vals["dx"] = b_t["e_dx"], b_t["dx"]
    stored = lambda t: S.ulp(torch.float32, t.abs())
    e = {k: v + stored(vals[k]) for k, v in e.items()}
    pw, pe = {}, {}
    r = W if cond else 3
    for i in range(D):
        pw[f"base.hidden_layers.{i}"] = (b_t["dw"][i], b_t["e_dw"][i], b_t["db"][i], b_t["e_db"][i])
    pw[first] = (b_t["dw"][D][:r], b_t["e_dw"][D][:r], b_t["db"][D][:r], b_t["e_db"][D][:r])
    pw["sigma_layer.output_layer"] = (b_t["dw"][D][r:], b_t["e_dw"][D][r:], b_t["db"][D][r:], b_t["e_db"][D][r:])
    if cond:
        pw["rgb_layer.hidden_layers.0"] = (b_c["dw"][0], b_c["e_dw"][0], b_c["db"][0], b_c["e_db"][0])
        pw["rgb_layer.output_layer"] = (b_c["dw"][1], b_c["e_dw"][1], b_c["db"][1], b_c["e_db"][1])
    for n, (dw, e_dw, db, e_db) in pw.items():
        pe["rsum/" + n + ".weight"] = e_dw.sum(1) + stored(dw.abs().sum(1)) * 2
        pe["csum/" + n + ".weight"] = e_dw.sum(0) + stored(dw.abs().sum(0)) * 2
        pe["rsum/" + n + ".bias"] = e_db + stored(db)
    return e, pe


def nerf_golden_check(kind, condition, dtype, device):
    """NerfMLP with the fixture's weights against the reference's float64 numbers: bit for bit (exact) or within the bound
    (xavier; returns the worst error/bound ratios)."""
    d = nerf_golden(("cond" if condition else "nocond") + "_" + kind)
    cd = d["condition"].shape[1]
    assert cd == (27 if condition else 0) and d["x"].shape == (33, 63)
    sd = Q.nerf_state_dict(kind, 63, cd)
    assert Q.checksum(sd) == float(d["checksum"]), "the weights are not the ones the fixture was made with"
    m = NerfMLP(63, cd, dtype=dtype)
    m.load_reference_state_dict(sd)
    m = m.to(device)
    x = d["x"].float().to(device).requires_grad_(True)
    c = d["condition"].float().to(device).requires_grad_(True)
    rgb, sigma = m(x, c) if condition else m(x)
    assert rgb.shape == (33, 3) and sigma.shape == (33, 1) and rgb.dtype == sigma.dtype == dtype
    ins = [x] + ([c, m.head.params] if condition else []) + [m.trunk.params]
    gr = torch.autograd.grad([rgb, sigma], ins, [d["g_rgb"].to(dtype).to(device), d["g_sigma"].to(dtype).to(device)])
    got = {"raw_rgb": rgb.detach(), "raw_sigma": sigma.detach(), "dx": gr[0]}
    if condition:
        got["dcondition"] = gr[1]
    got = {k: v.cpu().double() for k, v in got.items()}
    pg = nerf_param_grads(m, gr[-1].cpu().double(), gr[2].cpu().double() if condition else None)
    assert set(pg) == set(sd) == set(m.reference_keys())
    sums = {}
    for k, v in pg.items():
        if v.dim() == 2:
            sums["rsum/" + k], sums["csum/" + k] = v.sum(1), v.sum(0)
        else:
            sums["rsum/" + k] = v
    assert set(sums) == {k for k in d if k.startswith(("rsum/", "csum/"))}
    assert torch.equal(m.query_density(x).detach().cpu().double(), got["raw_sigma"])
    if kind == "exact":
        for k, v in {**got, **sums}.items():
            assert float(d[k].abs().max()) > 0 or k.endswith("sigma_layer.output_layer.bias") or d[k].numel() <= 1, f"{k}: a comparison of zeros"
            assert torch.equal(v, d[k]), k
        return None
    e, pe = nerf_bounds(sd, d, dtype, condition)
    ratios = {k: S.worst_ratio(v, d[k], e[k]) for k, v in got.items()}
    ratios["dparams"] = max(S.worst_ratio(v, d[k], pe[k]) for k, v in sums.items())
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)
    return ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("condition", [True, False])
@pytest.mark.parametrize("kind", ["exact", "xavier"])
def test_nerf_mlp_golden_cpu(kind, condition, dtype):
    ratios = nerf_golden_check(kind, condition, dtype, "cpu")
    if ratios:
        print(f"NerfMLP golden (cpu) {kind} condition={condition} {dtype} error/bound ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_nerf_mlp_structure_and_refusals():
    gen = torch.Generator().manual_seed(1)
    m = NerfMLP(63, 27, generator=gen)
    assert (m.trunk.n_input_dims, m.trunk.n_output_dims, m.trunk.n_neurons, m.trunk.n_hidden_layers, m.trunk.skip_mask) == (63, 257, 256, 8, 32)
    assert (m.head.n_input_dims, m.head.n_output_dims, m.head.n_neurons, m.head.n_hidden_layers, m.head.skip_mask) == (283, 3, 128, 1, 0)
    # each block of rows of the merged output matrix with the fan of the layer it is: bottleneck 256 -> 256, sigma 256 -> 1
    w = m.trunk.weight(8)
    for rows, fan_out in ((w[:256], 256), (w[256:], 1)):
        bound = (6.0 / (256 + fan_out)) ** 0.5
        assert 0.9 * bound < float(rows.detach().abs().max()) <= bound
    assert float(w[256:].detach().abs().max()) > (6.0 / 512) ** 0.5
    n = NerfMLP(63, 0)
    assert n.head is None and n.trunk.n_output_dims == 4 and float(n.trunk.weight(8)[:3].detach().abs().max()) <= (6.0 / 259) ** 0.5
    # a base that ends in cat([H, x]): the merged layer is a cat output layer
    deep = NerfMLP(20, 3, net_depth=5, net_width=128, skip_layer=4)
    assert deep.trunk.skip_mask == 1 << 5 and tuple(deep.trunk.weight(5).shape) == (129, 148)
    sd = Q.nerf_state_dict("xavier", 63, 27)
    m.load_reference_state_dict(sd)
    assert torch.equal(m.trunk.weight(8), torch.cat([sd["bottleneck_layer.output_layer.weight"], sd["sigma_layer.output_layer.weight"]]))
    assert torch.equal(m.head.bias(1), sd["rgb_layer.output_layer.bias"])
    with pytest.raises(ValueError, match="NerfMLP: load_reference_state_dict: missing keys .*sigma_layer.output_layer.bias"):
        m.load_reference_state_dict({k: v for k, v in sd.items() if k != "sigma_layer.output_layer.bias"})
    with pytest.raises(ValueError, match="unexpected keys .*extra"):
        m.load_reference_state_dict({**sd, "extra": torch.zeros(1)})
    with pytest.raises(ValueError, match="unexpected keys .*bottleneck_layer"):
        n.load_reference_state_dict(sd)
    with pytest.raises(ValueError, match="matrix 3"):
        m.load_reference_state_dict({**sd, "base.hidden_layers.3.weight": torch.zeros(256, 255)})
    with pytest.raises(ValueError, match="sigma_layer.output_layer.weight"):
        m.load_reference_state_dict({**sd, "sigma_layer.output_layer.weight": torch.zeros(1, 255)})
    x = torch.randn(4, 63, generator=gen)
    with pytest.raises(ValueError, match="a condition is required"):
        m(x)
    with pytest.raises(ValueError, match="cannot be taken"):
        n(x, torch.zeros(4, 27))
    with pytest.raises(ValueError, match=r"x must be \[..., 63\]"):
        m(x[:, :5], torch.zeros(4, 27))
    with pytest.raises(ValueError, match="NerfMLP: condition_dim -1"):
        NerfMLP(63, -1)


def test_nerf_mlp_broadcasts_a_condition_per_ray():
    """The reference's rule: a condition [num_rays, C] is spread over x's middle dimensions."""
    gen = torch.Generator().manual_seed(2)
    m = NerfMLP(63, 27, generator=gen)
    x, c = torch.randn(5, 6, 63, generator=gen), torch.randn(5, 27, generator=gen)
    rgb, sigma = m(x, c)
    assert rgb.shape == (5, 6, 3) and sigma.shape == (5, 6, 1) and m.query_density(x).shape == (5, 6, 1)
    full_rgb, full_sigma = m(x.reshape(30, 63), c[:, None, :].expand(5, 6, 27).reshape(30, 27))
    assert torch.equal(rgb.reshape(30, 3), full_rgb) and torch.equal(sigma.reshape(30, 1), full_sigma)
    assert torch.equal(m.query_density(x), sigma)
