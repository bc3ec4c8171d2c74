"""GPU: ``HashGridEncoding(interpolation="Smoothstep")`` on the native `_i` entries -- the forward bit for bit against the
torch path (fp16 / bf16: the float32 output rounded once), the backward and the second order against the float64 restatement
of tests/hashgrid_smoothstep_reference.py, reproducibility, the optional outputs, half gradients, ``deterministic=True`` bit
for bit against the numpy restatement, which native calls are made, the Linear grid untouched, C^1 at cell faces, the pure
second partial, empty input and an Eikonal loss trained end to end.

The bounds are those of the linear grid's tests: per table entry (cnt + 2) * 2^-23 * sum|term| at first order
(tests/test_encodings_gpu.py: test_backward_against_float64); at second order (k + 8) * 2^-23 * sum|term| per element, k the
number of summed terms (tests/test_hashgrid_grad2_gpu.py).  A smoothstep term is a product with at most 9 float32 roundings
after the float32 factors S, 1 - S, S', S'' that the restatement shares with the kernels, and each of the k - 1 additions adds
at most 2^-24 of a running sum that sum|term| bounds: (k - 1 + 9) * 2^-24 * sum|term| at worst, and the bound is at least
twice that.

The second-order table gradient goes through check_against_restatement of tests/test_hashgrid_grad2_gpu.py, which takes
k = hits (one per touching corner: the kernel adds one value a_c * g per touch) and not the restatement's own g2_params_k =
3 * hits (the three summands of a_c counted apart).  That is deliberately the tighter of the two: (hits + 8) <= (3 hits + 8),
and the three summands of a_c are covered by the 8.  g2_params_k is checked by the CPU tier."""
import functools

import numpy as np
import pytest
import torch

import hashgrid_smoothstep_reference as R
import hashgrid_sorted_reference as RL
from hashgrid2_reference import restate_grad2
from nerfacc_amd import _backend as B
from nerfacc_amd import encodings as E
from test_hashgrid_grad2_gpu import CallLog, check_against_restatement, second_order
from test_hashgrid_sorted_gpu import first_order, same_bits

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
KINDS = ["F1_L1", "F1_L32", "F8_L7_edge", "F2_odd_res", "density", "collide", "same_point", "top_digit"]   # R.configs()
WIDTHS = ["F1_L1", "F2_odd_res", "F4_L3", "F8_L7_edge"]                                                      # F = 1, 2, 4, 8
CASES = [pytest.param(kind, n, id=f"{n}-{kind}") for kind in KINDS + ["F4_L3"] for n in R.NS]
SORTED_CASES = [pytest.param(kind, n, id=f"{n}-{kind}") for kind in KINDS for n in R.NS]


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(grid on the CPU, x, g, v): computed once per (config, n), never modified."""
    enc = R.make_grid(kind)
    return (enc,) + R.make_inputs(kind, n, enc)


def pair(kind, dev, out_dtype=None):
    """The sorted and the atomic smoothstep grid on the device, sharing one parameter tensor."""
    det = R.make_grid(kind, out_dtype, deterministic=True).to(dev)
    atomic = R.make_grid(kind, out_dtype)
    atomic.params = det.params
    return det, atomic


def table_within(got, ref, hits, absum, extra):
    F = got.numel() // hits.numel()
    err = (got.detach().cpu().double() - ref).abs()
    bound = (hits.repeat_interleave(F) + extra) * 2.0 ** -23 * absum
    assert bool((err <= bound).all()), (float((err - bound).max()), int((err > bound).sum()))


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("kind,n", CASES)
def test_forward_bit_identical_to_torch_path(dev, kind, n):
    enc, x, _, _ = case(kind, n)
    if n > 8:
        x = x.clone()
        x[0] = torch.tensor([1e6, -1e7, 3e9])
    ref = enc(x)                                   # CPU: the torch path
    lin = R.make_grid(kind, interpolation="Linear")
    assert n == 1 or not torch.equal(ref, lin(x))                 # (n = 1: the point (1, 1, 1), where S(f) = f)
    got = R.make_grid(kind).to(dev)(x.to(dev))
    assert got.shape == ref.shape == (n, enc.n_output_dims)
    assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("kind", WIDTHS)
@pytest.mark.parametrize("d", HALF)
def test_half_output_is_the_float32_output_rounded_once(dev, d, kind):
    enc, x, _, _ = case(kind, 4097)
    y32 = R.make_grid(kind).to(dev)(x.to(dev))
    y = R.make_grid(kind, d).to(dev)(x.to(dev))
    assert y.dtype == d and torch.equal(y, y32.to(d))


# ---------------------------------------------------------------- backward and second order against float64
@pytest.mark.parametrize("kind,n", CASES)
def test_against_float64_restatement(dev, kind, n):
    enc, x, g, v = case(kind, n)
    r = R.restate(x, enc.params.detach(), enc, g, v)             # one reference for both orders
    encd = R.make_grid(kind).to(dev)
    # first order
    g_p, g_x = first_order(encd, x, g)
    g_p, g_x = g_p.clone(), g_x.clone()
    table_within(g_p, r["g_params"], r["hits"], r["g_params_abs"], 2)
    torch.testing.assert_close(g_x.cpu().double(), r["g_x"], rtol=1e-4, atol=1e-3 * float(r["g_x"].abs().mean()))
    assert torch.equal(first_order(encd, x, g)[1], g_x)                       # dL/dx bit for bit, run to run
    # second order
    x2, g2_p, gg_y, g_x2 = second_order(encd, x, g, v)
    x2, g2_p, gg_y = x2.clone(), g2_p.clone(), gg_y.clone()
    assert x2.shape == (n, 3) and gg_y.shape == g.shape and g2_p.shape == enc.params.shape and torch.equal(g_x2, g_x)
    check_against_restatement(r, x2, g2_p, gg_y)
    x2b, g2_pb, gg_yb, _ = second_order(encd, x, g, v)
    assert torch.equal(x2b, x2) and torch.equal(gg_yb, gg_y)                  # gg_y and x2 bit for bit, run to run
    check_against_restatement(r, None, g2_pb, None)
    if n == 4097 and kind != "same_point":
        assert int((r["hits"] > 0).sum()) > 1000 and int((g2_p != 0).sum()) > 1000


def native_second(enc, x, g, v, want):
    """One nfa_hashgrid_bwd_bwd_i call on device tensors with only the outputs named in ``want``."""
    t, L, F = enc.table, enc.n_levels, enc.n_features_per_level
    out = dict(gg_y=torch.full_like(g, float("nan")) if "gg_y" in want else None,
               g_p=torch.zeros_like(enc.params) if "g_p" in want else None,
               x2=torch.full_like(x, float("nan")) if "x2" in want else None)
    B.call("nfa_hashgrid_bwd_bwd_i", enc.interp, B.ELEM_CODES[g.dtype], B.ptr(x), B.ptr(enc.params), B.ptr(g), B.ptr(v),
           x.shape[0], L, F, t.log2_hashmap_size, t.c_scales, t.c_res, t.c_sizes, enc.params.numel(), B.ptr(out["gg_y"]),
           B.ptr(out["g_p"]), B.ptr(out["x2"]), B.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", WIDTHS + ["F1_L32", "collide"])
def test_each_output_alone(dev, kind):
    n = 4097
    enc, x, g, v = case(kind, n)
    encd = R.make_grid(kind).to(dev)
    xd, gd, vd = x.to(dev), g.to(dev), v.to(dev)
    with torch.cuda.device(dev):
        full = native_second(encd, xd, gd, vd, ("gg_y", "g_p", "x2"))
        x2, _, gg_y, _ = second_order(encd, x, g, v)
        assert torch.equal(full["x2"], x2) and torch.equal(full["gg_y"], gg_y)       # the module makes this call
        assert torch.equal(native_second(encd, xd, gd, vd, ("gg_y",))["gg_y"], full["gg_y"])
        assert torch.equal(native_second(encd, xd, gd, vd, ("x2",))["x2"], full["x2"])
        alone = native_second(encd, xd, gd, vd, ("g_p",))["g_p"]
    r = R.restate(x, enc.params.detach(), enc, g, v)
    check_against_restatement(r, None, alone, None)                # (atomic: the order of the adds varies)
    check_against_restatement(r, None, full["g_p"], None)


@pytest.mark.parametrize("kind", ["F1_L32", "F2_odd_res", "F4_L3", "F8_L7_edge", "collide"])
@pytest.mark.parametrize("d", HALF)
def test_half_gradients(dev, d, kind):
    n = 4097
    enc, x, g, v = case(kind, n)
    gh = g.to(d)
    ref = R.make_grid(kind).to(dev)
    x2_32, _, gg_y32, _ = second_order(ref, x, gh.float(), v)       # the float32 op on the exactly widened gradient
    g_p32, g_x32 = first_order(ref, x, gh.float())
    g_x32 = g_x32.clone()
    half = R.make_grid(kind, d)
    half.params = ref.params
    x2, g2_p, gg_y, g_x = second_order(half, x, gh, v)
    assert gg_y.dtype == d and gg_y.shape == g.shape
    assert torch.equal(gg_y, gg_y32.to(d))
    assert torch.equal(x2, x2_32) and torch.equal(g_x, g_x32)
    r = R.restate(x, enc.params.detach(), enc, gh.float(), v)
    check_against_restatement(r, None, g2_p, None)
    g_p, _ = first_order(half, x, gh)
    table_within(g_p, r["g_params"], r["hits"], r["g_params_abs"], 2)


# ---------------------------------------------------------------- deterministic=True
@pytest.mark.parametrize("kind,n", SORTED_CASES)
def test_sorted_table_gradients_bit_for_bit(dev, kind, n):
    enc, x, g, v = case(kind, n)
    F = enc.n_features_per_level
    det, atomic = pair(kind, dev)
    want, info = R.sorted_table_grad(x.numpy(), enc, g.numpy())
    g_p, g_x = first_order(det, x, g)
    g_p, g_x = g_p.clone(), g_x.clone()
    same_bits(g_p, want)
    R.check_bound(g_p.cpu().numpy(), info, F, 2)                  # also: exact zeros where nothing arrived
    assert torch.equal(first_order(det, x, g)[0], g_p)
    assert torch.equal(first_order(atomic, x, g)[1], g_x)
    want2, info2 = R.sorted_table_grad(x.numpy(), enc, g.numpy(), v.numpy())
    x2, g2_p, gg_y, _ = second_order(det, x, g, v)
    x2, g2_p, gg_y = x2.clone(), g2_p.clone(), gg_y.clone()
    same_bits(g2_p, want2)
    R.check_bound(g2_p.cpu().numpy(), info2, F, 8)
    assert torch.equal(second_order(det, x, g, v)[1], g2_p)
    x2a, _, gg_ya, _ = second_order(atomic, x, g, v)
    assert torch.equal(x2, x2a) and torch.equal(gg_y, gg_ya)
    if n > 1:
        assert not np.array_equal(want, RL.sorted_table_grad(x.numpy(), enc, g.numpy())[0])      # not the linear gradient


@pytest.mark.parametrize("d", HALF)
def test_sorted_half_gradients(dev, d):
    kind, n = "collide", 4097
    enc, x, g, v = case(kind, n)
    det, _ = pair(kind, dev, d)
    gh = g.to(d)
    same_bits(first_order(det, x, gh)[0], R.sorted_table_grad(x.numpy(), enc, gh.float().numpy())[0])
    _, g2_p, gg_y, _ = second_order(det, x, gh, v)
    assert gg_y.dtype == d
    same_bits(g2_p, R.sorted_table_grad(x.numpy(), enc, gh.float().numpy(), v.numpy())[0])


# ---------------------------------------------------------------- which native calls
@pytest.mark.parametrize("d", [torch.float32] + HALF)
def test_native_path_taken(dev, monkeypatch, d):
    out = None if d == torch.float32 else d
    det, atomic = pair("density", dev, out)
    monkeypatch.setattr(E, "_hashgrid_torch", lambda *a, **k: pytest.fail("the torch path ran"))
    _, x, g, v = case("density", 4097)
    log = CallLog(monkeypatch)
    second_order(atomic, x, g.to(d), v)
    torch.cuda.synchronize()
    assert log.names() == ["nfa_hashgrid_fwd_i", "nfa_hashgrid_bwd_i", "nfa_hashgrid_bwd_bwd_i"], log.names()
    assert all(a[0] == 1 and a[1] == B.ELEM_CODES[d] for _, a in log.calls)
    log.calls.clear()
    second_order(det, x, g.to(d), v)
    torch.cuda.synchronize()
    assert log.names() == ["nfa_hashgrid_fwd_i", "nfa_hashgrid_bwd_sorted_i", "nfa_hashgrid_bwd_bwd_sorted_i"], log.names()
    assert all(a[0] == 1 and a[1] == B.ELEM_CODES[d] for _, a in log.calls)
    assert log.calls[1][1][-2] == log.calls[2][1][-2] == RL.scratch_bytes(4097, det.n_levels)


# ---------------------------------------------------------------- Linear is untouched
@pytest.mark.parametrize("kind", ["F1_L32", "F2_odd_res", "F4_L3", "F8_L7_edge"])
def test_linear_keyword_is_the_default_grid(dev, monkeypatch, kind):
    n = 4097
    _, x, g, v = case(kind, n)
    results = []
    log = CallLog(monkeypatch)
    for kw in ({}, {"interpolation": "Linear"}):
        torch.manual_seed(0)
        L, F, log2, base, scale = R.grids()[kind]
        one = []
        for deterministic in (False, True):
            torch.manual_seed(0)
            enc = E.HashGridEncoding(3, L, F, log2, base, scale, deterministic=deterministic, **kw)
            with torch.no_grad():
                enc.params.uniform_(-1, 1)
            enc = enc.to(dev)
            y = enc(x.to(dev))
            g_p, g_x = first_order(enc, x, g)
            g_p = g_p.clone()
            x2, g2_p, gg_y, _ = second_order(enc, x, g, v)
            one += [y, g_x, gg_y, x2] + ([g_p, g2_p.clone()] if deterministic else [])
        results.append(one)
    assert len(results[0]) == len(results[1]) == 10
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert not any(name.endswith("_i") for name in log.names()), log.names()      # the entries it always called


# ---------------------------------------------------------------- C^1, the pure second partial
def one_level(interpolation, dev):
    torch.manual_seed(0)
    enc = E.HashGridEncoding(3, 1, 2, 14, 16, 2.0, interpolation=interpolation)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc.to(dev)


@pytest.mark.parametrize("d", [0, 1, 2])
def test_c1_at_cell_faces(dev, d):
    enc = one_level("Smoothstep", dev)
    x = R.face_points(enc, d, 1000)
    g = torch.randn(x.shape[0], enc.n_output_dims, generator=torch.Generator().manual_seed(9))
    _, g_x = first_order(enc, x, g)
    others = [k for k in range(3) if k != d]
    assert bool((g_x[:, d] == 0).all()) and bool((g_x[:, others] != 0).any())
    _, g_lin = first_order(one_level("Linear", dev), x, g)
    assert bool((g_lin[:, d] != 0).any())


@pytest.mark.parametrize("e", [0, 1, 2])
def test_pure_second_partial(dev, e):
    enc, _, g, _ = case("density", 4097)
    x = R.interior_points(4097, enc, seed=30 + e)
    v = torch.zeros(4097, 3)
    v[:, e] = torch.randn(4097, generator=torch.Generator().manual_seed(e)) + 3.0
    others = [k for k in range(3) if k != e]
    x2, _, _, _ = second_order(R.make_grid("density").to(dev), x, g, v)
    r = R.restate(x, enc.params.detach(), enc, g, v)
    check_against_restatement(r, x2, None, None)
    assert bool((r["x2"][:, e] != 0).all()) and bool((x2[:, e] != 0).all()) and bool((x2[:, others] != 0).any())
    x2_lin, _, _, _ = second_order(R.make_grid("density", interpolation="Linear").to(dev), x, g, v)
    assert bool((x2_lin[:, e] == 0).all()) and bool((x2_lin[:, others] != 0).any())
    assert bool((restate_grad2(x, enc.params.detach(), enc, g, v)["x2"][:, e] == 0).all())


# ---------------------------------------------------------------- empty input
@pytest.mark.parametrize("deterministic", [False, True])
def test_empty_input(dev, monkeypatch, deterministic):
    enc = R.make_grid("density", deterministic=deterministic).to(dev)
    log = CallLog(monkeypatch)
    x = torch.zeros(0, 3, device=dev, requires_grad=True)
    g = torch.zeros(0, enc.n_output_dims, device=dev, requires_grad=True)
    y = enc(x)
    assert y.shape == (0, enc.n_output_dims)
    (g_x,) = torch.autograd.grad(y, x, g, create_graph=True)
    assert g_x.shape == (0, 3)
    g_x.backward(torch.zeros(0, 3, device=dev))
    assert log.names() == []
    assert x.grad.shape == (0, 3) and g.grad.shape == g.shape
    assert enc.params.grad.shape == enc.params.shape and not bool(enc.params.grad.any())
    enc.params.grad = None
    enc(x).sum().backward()                                              # the plain first-order step
    assert enc.params.grad.shape == enc.params.shape and not bool(enc.params.grad.any())


# ---------------------------------------------------------------- an Eikonal loss end to end
def sdf_field():
    """tests/test_hashgrid_grad2_gpu.py's field with a smoothstep grid."""
    torch.manual_seed(0)
    enc = E.HashGridEncoding(3, 4, 2, 14, 16, 1.5, interpolation="Smoothstep")
    with torch.no_grad():
        enc.params.uniform_(-0.1, 0.1)
    return torch.nn.ModuleList([enc, torch.nn.Linear(8, 1)])


def test_eikonal_loss_trains(dev, monkeypatch):
    from test_hashgrid_grad2_gpu import eikonal_loss
    ref = sdf_field().double()
    x = R.interior_points(4096, ref[0], seed=5)          # boundary-free: the float32 and float64 cells coincide
    eikonal_loss(ref, x.double()).backward()
    field = sdf_field().to(dev)
    xd = x.to(dev)
    log = CallLog(monkeypatch)
    loss = eikonal_loss(field, xd)
    loss.backward()
    assert log.names() == ["nfa_hashgrid_fwd_i", "nfa_hashgrid_bwd_i", "nfa_hashgrid_bwd_bwd_i"], log.names()
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
    print("eikonal losses", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
