"""GPU: the fused MLP's activations (csrc/mlp.hip: the ACT instantiations behind nfa_mlp_act_*).  Bit for bit on integer-valued
data for the piecewise linear activations, through the module and through the four entries; the default pair forced through
the act entries against the net entries; the smooth activations within the derived bound of tests/mlp_act_reference.py, every
pass fed the reference's stored values; the second order through the module behind a Smoothstep hash grid; the same bits on
every run; guard rows; non-finite rows; and what the entries refuse on the host."""
import pytest
import torch

import mlp_act_reference as A
import mlp_bias_skip_reference as S
import mlp_grad2_reference as G
import mlp_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.mlp import FusedMLP, image_elems, wgrad_slices
from test_mlp_act_cpu import CURVED, act_id, first_and_second_order, make
from test_mlp_bias_skip_gpu import DEV, SENTINEL, guarded, guards_intact, stacked
import test_mlp_bias_skip_gpu as NET

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
N = 1000   # 31 full tiles and one of 8 points; four weight-gradient slices
assert wgrad_slices(N) == 4


def run_abi(shape, skip_mask, dtype, act, ws, bs, x, g, v, out_f32, hidden_in=None, y_in=None, dz_in=None, r_in=None):
    """The four nfa_mlp_act_* entries and nfa_mlp_net_bwd_weights (three times) called directly, every output between guard
    rows.  Each pass runs on what the passes before it wrote, or on ``hidden_in`` / ``y_in`` / ``dz_in`` / ``r_in`` where given
    (float64 values of stored numbers).  Returns CPU float64 tensors: y, hidden, dz (dZ_0 .. dZ_L), dx, dp, u, t, r (R_0 ..
    R_L), e (E_0 .. E_{L-1}), sx, sp1 (on (v, T, dZ)), sp2 (on (x, H, E))."""
    n_in, n_out, width, n_hidden = shape
    Np, elem = x.shape[0], B.ELEM_CODES[dtype]
    desc = B.MLPDesc(*shape, int(bs is not None), skip_mask)
    a = B.MLPAct(B.ACT_CODES[act[0]], B.ACT_CODES[act[1]], act[2])
    params = S.flat_params(ws, bs).to(DEV)
    P, n_w = params.numel(), sum(w.numel() for w in ws)
    fe, be = image_elems(*shape, skip_mask)
    fwd, bwd = torch.empty(fe, dtype=dtype, device=DEV), torch.empty(be, dtype=dtype, device=DEV)
    B.call("nfa_mlp_net_pack_weights", elem, desc, B.ptr(params), B.ptr(fwd), fe, B.ptr(bwd), be, B.stream())
    xd, gd, vd = x.to(DEV), g.to(DEV), v.to(DEV)
    bias_ptr = params.data_ptr() + 4 * n_w if bs is not None else None
    end = torch.float32 if out_f32 else dtype
    code = lambda t: B.ELEM_CODES[t.dtype]
    y_w, y = guarded(Np, n_out, end)
    hid_w, hid = guarded(n_hidden * Np, width, dtype)
    B.call("nfa_mlp_act_fwd", elem, desc, a, B.ptr(xd), code(xd), B.ptr(fwd), bias_ptr, Np, B.ptr(y), code(y), B.ptr(hid), 1, B.stream())
    hid_u = hid if hidden_in is None else stacked(hidden_in, dtype)
    y_u = y if y_in is None else y_in.to(end).to(DEV).contiguous()
    dz_w, dz = guarded(n_hidden * Np, width, dtype)
    dzo_w, dzo = guarded(Np, n_out, dtype)
    dx_w, dx = guarded(Np, n_in, xd.dtype)
    own_dzo = gd.dtype != dtype or act[1] != "None"
    B.call("nfa_mlp_act_bwd_data", elem, desc, a, B.ptr(gd), code(gd), B.ptr(y_u), code(y_u), B.ptr(hid_u), B.ptr(bwd), Np, B.ptr(dz),
           B.ptr(dzo) if own_dzo else None, B.ptr(dx), code(xd), B.stream())
    dz_out = dzo if own_dzo else gd
    part_w, part = guarded(wgrad_slices(Np) * P, 1, torch.float32)
    gp_w, gp = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_net_bwd_weights", elem, desc, B.ptr(xd), code(xd), B.ptr(hid_u), B.ptr(dz), B.ptr(dz_out), Np, B.ptr(part), part.numel(),
           B.ptr(gp), 0, B.stream())
    dz_u, dzo_u = (dz, dz_out) if dz_in is None else (stacked(dz_in[:-1], dtype), dz_in[-1].to(dtype).to(DEV).contiguous())
    tan_w, tan = guarded(n_hidden * Np, width, dtype)
    r_w, r = guarded(n_hidden * Np, width, dtype)
    ro_w, ro = guarded(Np, n_out, dtype)
    u_w, u = guarded(Np, n_out, end)
    B.call("nfa_mlp_act_tangent", elem, desc, a, B.ptr(vd), code(vd), B.ptr(y_u), code(y_u), B.ptr(hid_u), B.ptr(dz_u), B.ptr(dzo_u),
           B.ptr(fwd), Np, B.ptr(tan), B.ptr(r), B.ptr(ro), B.ptr(u), code(u), B.stream())
    r_u, ro_u = (r, ro) if r_in is None else (stacked(r_in[:-1], dtype), r_in[-1].to(dtype).to(DEV).contiguous())
    e_w, e = guarded(n_hidden * Np, width, dtype)
    sx_w, sx = guarded(Np, n_in, xd.dtype)
    B.call("nfa_mlp_act_curvature", elem, desc, a, B.ptr(ro_u), B.ptr(hid_u), B.ptr(r_u), B.ptr(bwd), Np, B.ptr(e), B.ptr(sx), code(xd),
           B.stream())
    sp1_w, sp1 = guarded(P, 1, torch.float32)
    sp2_w, sp2 = guarded(P, 1, torch.float32)
    B.call("nfa_mlp_net_bwd_weights", elem, desc, B.ptr(vd), code(vd), B.ptr(tan), B.ptr(dz_u), B.ptr(dzo_u), Np, B.ptr(part), part.numel(),
           B.ptr(sp1), 1, B.stream())
    B.call("nfa_mlp_net_bwd_weights", elem, desc, B.ptr(xd), code(xd), B.ptr(hid_u), B.ptr(e), B.ptr(ro_u), Np, B.ptr(part), part.numel(),
           B.ptr(sp2), 0, B.stream())
    torch.cuda.synchronize()
    for name, whole in [("y", y_w), ("hidden", hid_w), ("dz", dz_w), ("dz_out", dzo_w), ("dx", dx_w), ("partials", part_w),
                        ("grad_params", gp_w), ("tangent", tan_w), ("r", r_w), ("r_out", ro_w), ("u", u_w), ("e", e_w), ("ds/dx", sx_w),
                        ("ds/dparams 1", sp1_w), ("ds/dparams 2", sp2_w)]:
        assert guards_intact(whole), f"{name}: guard rows overwritten"
    if not own_dzo:
        assert bool((dzo == SENTINEL).all()), "dz_out written although it was not passed"
    c = lambda t: t.cpu().double()
    rows = lambda t: [c(t[l * Np:(l + 1) * Np]) for l in range(n_hidden)]
    return dict(y=c(y), hidden=rows(hid), dz=rows(dz) + [c(dz_out)], dx=c(dx), dp=c(gp).view(-1), u=c(u), t=rows(tan), r=rows(r) + [c(ro)],
                e=rows(e), sx=c(sx), sp1=c(sp1).view(-1), sp2=c(sp2).view(-1))


def reference(shape, skip_mask, dtype, act, ws, bs, x, g, v, out_f32, exact=False):
    f = A.forward(x, ws, bs, skip_mask, dtype, act, out_f32, exact)
    b = A.backward(x, ws, f["hidden"], f["y"], g, skip_mask, dtype, act, exact=exact)
    t = A.tangent(v, ws, f["hidden"], f["y"], b["dz"], skip_mask, dtype, act, out_f32, exact)
    c = A.backward(x, ws, f["hidden"], None, t["r"][-1], skip_mask, dtype, act, inject=t["r"][:-1])
    sw, e_sw = A.tangent_weight_grad(b["dz"], t, skip_mask)
    return f, b, t, c, sw, e_sw


# ---------------------------------------------------------------- bit for bit: the piecewise linear activations

# (hidden, output, family, width, n_hidden, skip_layer, bias, n_in, n_out).  A LeakyReLU value is rnd(rnd32(0.01f k)), no integer:
# behind it only sums of ONE term are exact whatever their order, so those cases take the 'perm' family with n_in = width (one
# entry per row and at most one per column of every matrix) without bias and skip; and a weight gradient, which sums such
# values over the points, is compared within the bound.
EXACT = [
    ("None", "ReLU", "perm", 64, 3, 2, True, 36, 3),
    ("ReLU", "ReLU", "dense", 128, 2, None, True, 40, 32),
    ("None", "None", "perm", 128, 3, 1, True, 36, 3),
    ("LeakyReLU", "None", "perm", 64, 2, None, False, 64, 3),
    ("ReLU", "LeakyReLU", "perm", 128, 2, None, False, 128, 32),
    ("LeakyReLU", "LeakyReLU", "perm", 64, 3, None, False, 64, 16),
]


def check_exact(case, dtype, Np=N):
    hid, out, family, width, n_hidden, skip_layer, bias, n_in, n_out = case
    act, leaky = (hid, out, 10.0), "LeakyReLU" in (hid, out)
    shape, skip_mask = (n_in, n_out, width, n_hidden), S.skip_mask_of(skip_layer, n_hidden)
    ws = S.exact_weights(family, *shape, skip_mask)
    bs = S.exact_biases(n_out, width, n_hidden) if bias else None
    x, g = R.exact_inputs(Np, n_in, n_out, dtype, dtype)
    v = G.exact_tangent_input(Np, n_in, dtype, 7)
    f, b, t, c, sw, e_sw = reference(shape, skip_mask, dtype, act, ws, bs, x, g, v, False, exact=not leaky)
    assert bool(f["y"].any()) and bool(b["dx"].any()) and bool(t["u"].any()) and not bool(c["dx"].any())
    n_w = sum(w.numel() for w in ws)
    want_p, e_p = S.flat_params(b["dw"], b["db"] if bias else None), S.flat_params(b["e_dw"], b["e_db"] if bias else None)
    want_s, e_s = S.flat_params(sw), S.flat_params(e_sw)
    tag = f"{case} {dtype}"

    def same_params(got, want, bound, name):
        if leaky:
            assert A.worst_ratio(got, want, bound) <= 1.0, f"{name}: {tag}"
        else:
            assert torch.equal(got, want), f"{name}: {tag}"

    y, g_x, g_p, u, s_p, s_x = first_and_second_order(make(shape, dtype, ws, bs, skip_layer, act, device=DEV), x, g, v)
    assert torch.equal(y.cpu().double(), f["y"]) and torch.equal(g_x.cpu().double(), b["dx"]), f"module y, dL/dx: {tag}"
    assert torch.equal(u.cpu().double(), t["u"]) and s_x is None, f"module u, ds/dx: {tag}"
    same_params(g_p.cpu().double(), want_p, e_p, "module dL/dparams")
    same_params(s_p.cpu().double()[:n_w], want_s, e_s, "module ds/dW")
    assert not bool(s_p[n_w:].any()), f"module ds/db: {tag}"
    a = run_abi(shape, skip_mask, dtype, act, ws, bs, x, g, v, False)
    assert torch.equal(a["y"], f["y"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["u"], t["u"]), f"abi y, dx, u: {tag}"
    for l in range(n_hidden):
        assert torch.equal(a["hidden"][l], f["hidden"][l]) and torch.equal(a["t"][l], t["t"][l + 1]), f"hidden, T {l}: {tag}"
        assert not bool(a["e"][l].any()), f"E_{l}: {tag}"
    for l in range(n_hidden + 1):
        assert torch.equal(a["dz"][l], b["dz"][l]) and not bool(a["r"][l].any()), f"dZ_{l}, R_{l}: {tag}"
    same_params(a["dp"], want_p, e_p, "abi dW, db")
    same_params(a["sp1"][:n_w], want_s, e_s, "abi ds/dW")
    assert not bool(a["sp1"][n_w:].any()) and not bool(a["sp2"].any()) and not bool(a["sx"].any()), f"zero curvature: {tag}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EXACT, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-W{c[3]}-L{c[4]}-skip{c[5]}-bias{int(c[6])}")
def test_exact(case, dtype):
    check_exact(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_partial_tile_after_full_sweeps(dtype):
    """128 wide, 4 hidden layers, layer 3 takes [H, x], biases: one workgroup per compute unit.  Two full sweeps of 256 x 4 waves
    x 32 points, five full tiles and a tile of 7 points."""
    check_exact(("ReLU", "ReLU", "perm", 128, 4, 2, True, 36, 3), dtype, Np=2 * 256 * 4 * 32 + 5 * 32 + 7)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net", ["warp", "sdf_head"])
def test_default_pair_through_the_act_entries_is_the_net_entries(net, dtype):
    """activation ReLU, output None forced through nfa_mlp_act_*: the bits of nfa_mlp_net_* on random data, intermediates too."""
    shape, skip_layer, skip_mask, ws, bs, x, g, v = NET.random_case(net, dtype, True)
    old = NET.run_abi(shape, skip_mask, dtype, ws, bs, x, g, v, True)
    new = run_abi(shape, skip_mask, dtype, ("ReLU", "None", 10.0), ws, bs, x, g, v, True)
    for k in ("y", "dx", "dp", "u"):
        assert torch.equal(new[k], old[k]), k
    assert torch.equal(new["sp1"], old["sp"])
    for l in range(shape[3]):
        assert torch.equal(new["hidden"][l], old["hidden"][l]) and torch.equal(new["t"][l], old["t"][l]), l
    for l in range(shape[3] + 1):
        assert torch.equal(new["dz"][l], old["dz"][l]) and not bool(new["r"][l].any()), l
    assert not bool(new["sp2"].any()) and not bool(new["sx"].any())


# ---------------------------------------------------------------- the smooth activations within the derived bound

WIDE = (36, 3, 128, 4)   # biases, skip_layer 2
SHAPES = [(s, None, False) for s in R.NGP_SHAPES] + [(WIDE, 2, True)]
SMOOTH = [(n, "None", b) for n, b in CURVED] + [("ReLU", n, b) for n, b in CURVED]
# each activation once as hidden and once as output activation, the shapes dealt round: the 128-wide network gets Softplus
# (beta 100) hidden and Softplus (beta 10) output, and every NGP shape a hidden and an output case
SMOOTH_CASES = [(act, SHAPES[i % len(SHAPES)]) for i, act in enumerate(SMOOTH)] + [(("Softplus", "Sigmoid", 100.0), SHAPES[1])]


def check_within_the_bound(act, net, dtype, f32_ends, Np=N):
    shape, skip_layer, bias = net
    scale = 0.25 if "Exponential" in act[:2] else 1.0
    skip_mask, ws, bs, x, g, v = A.random_net(shape, skip_layer, N=Np, dtype=dtype, f32_ends=f32_ends, scale=scale)
    bs = bs if bias else None
    n_hidden = shape[3]
    f, b, t, c, sw, e_sw = reference(shape, skip_mask, dtype, act, ws, bs, x, g, v, f32_ends)
    a = run_abi(shape, skip_mask, dtype, act, ws, bs, x, g, v, f32_ends, hidden_in=f["hidden"], y_in=f["y"], dz_in=b["dz"], r_in=t["r"])
    n_w = sum(w.numel() for w in ws)
    ratios = {"y": A.worst_ratio(a["y"], f["y"], f["e_y"]), "dx": A.worst_ratio(a["dx"], b["dx"], b["e_dx"]),
              "u": A.worst_ratio(a["u"], t["u"], t["e_u"]), "sx": A.worst_ratio(a["sx"], c["dx"], c["e_dx"])}
    for l in range(n_hidden):
        ratios[f"h{l}"] = A.worst_ratio(a["hidden"][l], f["hidden"][l], f["e_hidden"][l])
        ratios[f"t{l}"] = A.worst_ratio(a["t"][l], t["t"][l + 1], t["e_t"][l + 1])
        ratios[f"e{l}"] = A.worst_ratio(a["e"][l], c["dz"][l], c["e_dz"][l])
    for l in range(n_hidden + 1):
        ratios[f"dz{l}"] = A.worst_ratio(a["dz"][l], b["dz"][l], b["e_dz"][l])
        ratios[f"r{l}"] = A.worst_ratio(a["r"][l], t["r"][l], t["e_r"][l])
    ratios["dw"] = A.worst_ratio(a["dp"][:n_w], S.flat_params(b["dw"]), S.flat_params(b["e_dw"]))
    ratios["sw"] = A.worst_ratio(a["sp1"][:n_w], S.flat_params(sw), S.flat_params(e_sw))
    ratios["cw"] = A.worst_ratio(a["sp2"][:n_w], S.flat_params(c["dw"]), S.flat_params(c["e_dw"]))
    if bias:
        ratios["db"] = A.worst_ratio(a["dp"][n_w:], S.flat_params(b["db"]), S.flat_params(b["e_db"]))
        ratios["cb"] = A.worst_ratio(a["sp2"][n_w:], S.flat_params(c["db"]), S.flat_params(c["e_db"]))
        assert not bool(a["sp1"][n_w:].any()) and bool(a["sp2"][n_w:].any())
    print(f"mlp act error/bound ratios {act} {shape} {dtype} f32_ends={f32_ends} N={Np}: " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    assert bool(a["sx"].any()) and bool(a["sp2"].any()) and bool(a["u"].any())
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMOOTH_CASES, ids=lambda c: f"{act_id(c[0])}-{'x'.join(map(str, c[1][0]))}")
def test_smooth_within_the_bound(case, dtype):
    check_within_the_bound(case[0], case[1], dtype, f32_ends=dtype == torch.bfloat16)


@pytest.mark.parametrize("Np", [1, 33])
def test_guard_rows_at_one_point_and_one_past_a_tile(Np):
    """run_abi puts every output between guard rows; here N = 1 and N = 33 (a tile of one point behind a full one)."""
    check_within_the_bound(("Softplus", "Sigmoid", 100.0), SHAPES[3], torch.float16, False, Np=Np)
    check_within_the_bound(("Tanh", "Exponential", 10.0), SHAPES[1], torch.bfloat16, True, Np=Np)


# ---------------------------------------------------------------- through the module

def sdf_net(activation, dtype=torch.float16, device=DEV):
    return FusedMLP(32, 1, 64, 2, dtype=dtype, second_order=True, bias=True, activation=activation, activation_beta=100.0).to(device)


def eikonal_step(mlp, monkeypatch):
    from nerfacc_amd.encodings import HashGridEncoding
    torch.manual_seed(0)
    # 16 levels x 2 features = the network's 32 inputs, resolutions 16 .. 67: the cotangent of dL/de that the grid's second order
    # hands to the network is fp16 and grows with the finest resolution (at 16 x 1.5^15 = 7000 it passes 65504)
    enc = HashGridEncoding(3, 16, 2, 14, 16, 1.1, out_dtype=torch.float16, interpolation="Smoothstep").to(DEV)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
        mlp.bias(2).fill_(-0.5)
    x = torch.rand(300, 3, device=DEV, requires_grad=True)
    seen, calls = {}, []
    e = enc(x)

    def on_g_e(g_e):
        if g_e is not None and g_e.requires_grad:
            g_e.register_hook(lambda gg_e: seen.__setitem__("gg_e", gg_e.detach().clone()))

    e.register_hook(on_g_e)
    # what the MLP hands back to the hash grid's second order: the gradient towards e that arrives in the second backward
    e.register_hook(lambda s_e: seen.__setitem__("s_e", None if s_e is None else s_e.detach().clone()))
    sdf = mlp(e)
    sdf.register_hook(lambda g_: seen.__setitem__("g", g_.detach().clone()))
    (n,) = torch.autograd.grad(sdf.float().sum(), x, create_graph=True)
    seen.pop("s_e", None)   # the first backward's dL/de
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    ((n.norm(dim=-1) - 1.0) ** 2).mean().backward()
    monkeypatch.setattr(B, "call", real)
    print(f"eikonal step: max |normal| {float(n.norm(dim=-1).max()):.3e}, max |cotangent of dL/de| {float(seen['gg_e'].float().abs().max()):.3e}")
    return enc, e.detach(), seen, [c for c in calls if c.startswith("nfa_mlp")]


def test_second_order_through_the_module_softplus_sdf(monkeypatch):
    """Softplus (beta 100) 32 -> 2 x 64 -> 1 with biases behind a Smoothstep hash grid, one Eikonal step.  The module's second
    order on the captured tensors against its CPU path.  Both paths round at the same points and differ in the order of the
    float32 sums and in the last ulps of expf / log1pf, which now and then moves a stored fp16 value to its neighbour; one fp16
    ulp (2^-10 relative) of a stored activation moves rho = beta e^(-beta H) by up to beta 2^-10 of itself, and every gradient
    here is a sum of terms with such a factor.  Bound per tensor: beta 2^-10 max |want|, element by element."""
    mlp = sdf_net("Softplus")
    enc, e, seen, calls = eikonal_step(mlp, monkeypatch)
    assert calls == ["nfa_mlp_act_tangent", "nfa_mlp_act_curvature", "nfa_mlp_net_bwd_weights", "nfa_mlp_net_bwd_weights"], calls
    n_w = mlp._offsets[-1]
    for name, t in [("table", enc.params.grad), ("matrices", mlp.params.grad[:n_w]), ("biases", mlp.params.grad[n_w:])]:
        assert bool(torch.isfinite(t).all()) and bool(t.any()), name
    assert seen.get("s_e") is not None and bool(seen["s_e"].any()), "ds/dx of the MLP did not reach the hash grid"
    # the module alone on the captured tensors, device and CPU
    got = {}
    for dev in (DEV, "cpu"):
        alone = sdf_net("Softplus", device=dev)
        alone.load_state_dict(mlp.state_dict())
        ed = e.to(dev).clone().requires_grad_(True)
        gd = seen["g"].to(dev).clone().requires_grad_(True)
        (g_e,) = torch.autograd.grad(alone(ed), ed, gd, create_graph=True)
        got[dev] = [t.cpu().double() for t in torch.autograd.grad(g_e, [alone.params, ed, gd], seen["gg_e"].to(dev))]
    assert torch.equal(got[DEV][0].float(), mlp.params.grad.cpu()) and torch.equal(got[DEV][1], seen["s_e"].cpu().double())
    for name, a, w in zip(["ds/dparams", "ds/dx", "ds/dg"], got[DEV], got["cpu"]):
        bound = 100.0 * 2.0 ** -10 * float(w.abs().max())
        print(f"softplus sdf second order, {name}: max |device - cpu| {float((a - w).abs().max()):.3e}, bound {bound:.3e}, max |cpu| {float(w.abs().max()):.3e}")
        assert float((a - w).abs().max()) <= bound, name


def test_second_order_through_the_module_relu_has_no_curvature(monkeypatch):
    mlp = sdf_net("ReLU")
    enc, e, seen, calls = eikonal_step(mlp, monkeypatch)
    assert calls == ["nfa_mlp_net_tangent", "nfa_mlp_net_bwd_weights"], calls
    n_w = mlp._offsets[-1]
    assert seen.get("s_e") is None and bool(mlp.params.grad[:n_w].any()) and not bool(mlp.params.grad[n_w:].any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_reproducible(dtype):
    act, (shape, skip_layer, _) = ("Softplus", "Sigmoid", 100.0), SHAPES[3]
    skip_mask, ws, bs, x, g, v = A.random_net(shape, skip_layer, N=N, dtype=dtype)
    m = make(shape, dtype, ws, bs, skip_layer, act, device=DEV)
    first = first_and_second_order(m, x, g, v)
    first_and_second_order(m, x[:333], g[:333], v[:333])   # another N in between: other slices, other scratch
    second = first_and_second_order(m, x, g, v)
    for a, b_ in zip(first, second):
        assert a.dtype == b_.dtype and torch.equal(a, b_) and bool(a.any())
    one = run_abi(shape, skip_mask, dtype, act, ws, bs, x, g, v, False)
    two = run_abi(shape, skip_mask, dtype, act, ws, bs, x, g, v, False)
    for k, a in one.items():
        for p, q in zip(a if isinstance(a, list) else [a], two[k] if isinstance(a, list) else [two[k]]):
            assert torch.equal(p, q), k


# ---------------------------------------------------------------- non-finite rows

@pytest.mark.parametrize("act", [("Softplus", "Sigmoid", 100.0), ("Tanh", "Exponential", 10.0), ("LeakyReLU", "None", 10.0)], ids=act_id)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_row_stays_in_its_row(act, bad):
    """NaN or +-inf in one row of x, g and v changes that row of y, dL/dx, u and ds/dx and nothing else in them; the row is the
    last one of the partial tile, whose clamped loads put it into lanes that do not store."""
    shape, skip_layer, _ = SHAPES[1]
    skip_mask, ws, bs, x, g, v = A.random_net(shape, skip_layer, N=N, f32_ends=True, scale=0.25)
    m = make(shape, torch.float16, ws, bs, skip_layer, act, out_f32=True, device=DEV)
    clean = first_and_second_order(m, x, g, v)
    for row in (N - 1, 40):
        for which in range(3):
            dirty = [t.clone() for t in (x, g, v)]
            dirty[which][row, 1] = bad
            got = first_and_second_order(m, *dirty)
            keep = torch.ones(N, dtype=torch.bool, device=DEV)
            keep[row] = False
            for k in (0, 1, 3, 5):   # y, dL/dx, u, ds/dx: one row per point
                if got[k] is None:
                    assert clean[k] is None
                    continue
                assert torch.equal(got[k][keep], clean[k][keep]), (act, bad, row, which, k)
            assert any(not torch.equal(got[k][row], clean[k][row]) for k in (0, 1, 3)), (act, bad, row, which)


def test_exponential_overflows_to_inf_in_fp16():
    """e^12 = 162755 is past fp16's 65504: the stored y is inf, never the saturated 65504; e^11 = 59874 is stored rounded."""
    m = FusedMLP(1, 1, 64, 1, activation="None", output_activation="Exponential")
    w0, w1 = torch.zeros(64, 1), torch.zeros(1, 64)
    w0[0, 0], w1[0, 0] = 1.0, 1.0
    m.load_linear_weights([w0, w1])
    y = m.to(DEV)(torch.tensor([[12.0], [11.0], [-30.0]], device=DEV)).cpu()
    assert y.dtype == torch.float16 and bool(torch.isinf(y[0, 0])) and float(y[0, 0]) > 0
    assert float(y[1, 0]) == float(torch.tensor(59874.1417).half()) and float(y[2, 0]) == 0.0


# ---------------------------------------------------------------- what the entries refuse, on the host

def test_abi_refusals():
    shape, dtype = (32, 3, 64, 2), torch.float16
    elem, desc = B.ELEM_CODES[dtype], B.MLPDesc(32, 3, 64, 2, 0, 0)
    fe, be = image_elems(*shape)
    half = lambda *s: torch.full(s, SENTINEL, dtype=dtype, device=DEV)
    fwd, bwd, x, y, hid, dz, dzo, dx, r = half(fe), half(be), half(64, 32), half(64, 3), half(2 * 64, 64), half(2 * 64, 64), half(64, 3), half(64, 32), half(2 * 64 + 1, 64)
    outs = [y, hid, dz, dzo, dx]

    def fwd_call(a, n=64):
        B.call("nfa_mlp_act_fwd", elem, desc, a, B.ptr(x), elem, B.ptr(fwd), None, n, B.ptr(y), elem, B.ptr(hid), 1, B.stream())

    def bwd_call(a, y_ptr, dzo_ptr):
        B.call("nfa_mlp_act_bwd_data", elem, desc, a, B.ptr(x[:, :3].contiguous()), elem, y_ptr, elem, B.ptr(hid), B.ptr(bwd), 64, B.ptr(dz), dzo_ptr,
               B.ptr(dx), elem, B.stream())

    act = lambda h, o, beta=10.0: B.MLPAct(h, o, beta)
    for a, msg in [(act(7, 0), "hidden activation 7"), (act(-1, 0), "hidden activation -1"), (act(1, 9), "output activation 9"),
                   (act(5, 0, 0.0), "beta 0"), (act(5, 0, -2.0), "beta -2"), (act(5, 0, float("nan")), "beta nan")]:
        with pytest.raises(B.NativeError, match=msg):
            fwd_call(a)
        with pytest.raises(B.NativeError, match=msg):
            fwd_call(a, 0)   # before the n_points = 0 return
    with pytest.raises(B.NativeError, match="activation descriptor is null"):
        fwd_call(None)
    with pytest.raises(B.NativeError, match="n_points -1 is negative"):
        fwd_call(act(5, 3), -1)
    with pytest.raises(B.NativeError, match="an output activation needs y and dz_out"):
        bwd_call(act(1, 3), None, B.ptr(dzo))
    with pytest.raises(B.NativeError, match="an output activation needs y and dz_out"):
        bwd_call(act(1, 3), B.ptr(y), None)
    with pytest.raises(B.NativeError, match="an output activation needs y"):
        B.call("nfa_mlp_act_tangent", elem, desc, act(1, 3), B.ptr(x), elem, None, elem, B.ptr(hid), B.ptr(dz), B.ptr(dzo), B.ptr(fwd), 64,
               B.ptr(dz), None, None, B.ptr(y), elem, B.stream())
    with pytest.raises(B.NativeError, match="r and r_out: both or neither"):
        B.call("nfa_mlp_act_tangent", elem, desc, act(5, 0), B.ptr(x), elem, None, elem, B.ptr(hid), B.ptr(dz), B.ptr(dzo), B.ptr(fwd), 64,
               B.ptr(dz), B.ptr(r), None, B.ptr(y), elem, B.stream())
    for inj, msg in [(r.data_ptr() + 2, r"misaligned pointer \(inject 8\)"), (None, r"null pointer \(inject\)")]:
        with pytest.raises(B.NativeError, match=msg):
            B.call("nfa_mlp_act_curvature", elem, desc, act(5, 0), B.ptr(dzo), B.ptr(hid), inj, B.ptr(bwd), 64, B.ptr(dz), B.ptr(dx), elem,
                   B.stream())
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), "a refused call wrote to its outputs"
