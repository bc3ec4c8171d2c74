"""The float64 restatement of the warp stage of the fused NDR query (csrc/ndr_warp.h): three coupling blocks with the kernel's rounding
points and a running error bound.  The encoders are handed in (the module's own, native on the device), because a float32 sincosf's
bits cannot be restated; an encoded column whose position carries e is off by e (identity) or min(2, 2^k e) plus, per side, T-NeRF's
2^-20 for a float32 sincosf, plus its rounding.  The networks follow tests/mlp_bias_skip_reference.py / mlp_stream_reference.py; a
time layer is a one-layer network rounded to the half type.  dw, theta and the translation are float32 and never rounded; every
float32 sum and product of the coupling tail costs one float32 ulp.  Behind the warped position the query is nerf_field_reference's."""
import torch

import mlp_bias_skip_reference as S
import mlp_stream_reference as M
from mlp_reference import ulp, worst_ratio  # noqa: F401

BLOCKS, NET1, NET2, TIME = 3, (82, 1, 128, 2), (73, 3, 128, 1), (9, 64)
SINCOS, F32 = 2.0 ** -20, torch.float32
# the golden fixture's fields (scripts/gen_ndr_golden.py): net_depth, net_width, skip_layer of the NeRF network, the warp's weights
FIELDS = {"perm": (2, 128, 4, "perm"), "rot": (2, 128, 4, "rot")}


def perm_weights(rot=False):
    """One non-zero term in every sum, powers of two, zero biases, zero rows for theta: cos = 1, sin = 0 and every rounding is a
    no-op.  The dw and translation rows are non-zero and differ per block (another input column, another scale).  ``rot``: the same
    matrices with theta = a hidden neuron / 16 and a bias on every layer, the time layers' included: no longer exact, but an error
    still travels along single terms, so the bound stays at a few roundings while rotation and biases move the result by far more."""
    out = []
    for i in range(BLOCKS):
        blk = {}
        for key, (n_in, n_out, width, depth), roll in (("n1", NET1, 1 + 5 * i), ("n2", NET2, 2 + 3 * i)):
            ws = S.exact_weights("perm", n_in, n_out, width, depth, 0)
            ws[0] = torch.roll(ws[0], roll, 1)
            ws[-1] = ws[-1].abs() * 2.0 ** -(i + 2)
            if key == "n2":
                ws[-1][0] = ws[-1][0] * (0.25 if rot else 0.0)
            blk[key] = (ws, [(torch.arange(w.shape[0]) % 3 + 1) / 16.0 * rot for w in ws])
        for key, shift in (("t1", i), ("t2", i + 4)):
            w = torch.zeros(TIME[1], TIME[0])
            j = torch.arange(TIME[1])
            w[j, (j + shift) % TIME[0]] = 2.0 ** (j % 2).float()   # never below 1: a small sine times 2^-k would leave fp16's grid
            blk[key] = (w, (j % 4) / 8.0 * rot)
        out.append(blk)
    return out


def xavier_weights(seed=29, out_scale=1.0 / 16, theta_scale=3.0):
    """Xavier-uniform matrices in multiples of 2^-8, biases in +-0.5; output layers scaled: dw, translation ~ 0.1, theta ~ 0.3."""
    gen = torch.Generator().manual_seed(seed)
    xav = lambda o, i: torch.round((torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 * 256) / 256
    out = []
    for _ in range(BLOCKS):
        blk = {}
        for key, (n_in, n_out, width, depth) in (("n1", NET1), ("n2", NET2)):
            dims = S.layer_dims(n_in, n_out, width, depth, 0)
            ws, bs = [xav(o, i) for o, i in dims], [torch.rand(o, generator=gen) - 0.5 for o, _ in dims]
            ws[-1], bs[-1] = ws[-1] * out_scale, bs[-1] * out_scale
            if key == "n2":
                ws[-1][0], bs[-1][0] = ws[-1][0] * theta_scale, bs[-1][0] * theta_scale
            blk[key] = (ws, bs)
        for key in ("t1", "t2"):
            blk[key] = (xav(TIME[1], TIME[0]), torch.rand(TIME[1], generator=gen) - 0.5)
        out.append(blk)
    return out


def load(f, blocks):   # the family into a module's warp
    with torch.no_grad():
        for i, blk in enumerate(blocks):
            f.warp_layers_1[i].load_linear_weights(*blk["n1"])
            f.warp_layers_2[i].load_linear_weights(*blk["n2"])
            for lin, (w, b) in ((f.time_layers_1[i], blk["t1"]), (f.time_layers_2[i], blk["t2"])):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
    return f


def reference_state_dict(name):
    """The reference module's state dict (without the encoders' buffers) of a field of FIELDS."""
    depth, width, skip, kind = FIELDS[name]
    sd = {}
    for i, blk in enumerate(perm_weights(kind == "rot")):
        for g, key in (("warp_layers_1", "n1"), ("warp_layers_2", "n2")):
            ws, bs = blk[key]
            names = [f"{g}.{i}.hidden_layers.{l}" for l in range(len(ws) - 1)] + [f"{g}.{i}.output_layer"]
            sd.update({n + ".weight": w for n, w in zip(names, ws)}, **{n + ".bias": b for n, b in zip(names, bs)})
        for g, key in (("time_layers_1", "t1"), ("time_layers_2", "t2")):
            sd[f"{g}.{i}.output_layer.weight"], sd[f"{g}.{i}.output_layer.bias"] = blk[key]
    sd.update({"nerf.mlp." + k: v for k, v in M.nerf_state_dict("xavier", 63, 27, depth, width, skip, 1, 128).items()})
    return sd


def enc_err(enc, e_x, dtype, n_freqs=4, against_exact=False):
    """The error of an encoded row whose position carries e_x [N, D].  Between two sides that run the same native encoder a column
    of an unmoved position is the same bits (zero); ``against_exact``: the other side is the float64 formula (the golden fixture), so
    every sine carries one sincosf error and every column its rounding, as tnerf_field_reference.golden_bound counts them."""
    k = torch.arange(n_freqs, dtype=torch.float64).repeat_interleave(e_x.shape[1])
    moved = torch.ones_like(e_x.repeat(1, n_freqs)) if against_exact else (e_x.repeat(1, n_freqs) > 0).double()
    trig = (e_x.repeat(1, n_freqs) * 2.0 ** k).clamp_max(2.0) + (1 if against_exact else 2) * SINCOS * moved
    e = torch.cat([e_x, trig, trig], 1)
    return e + ulp(dtype, enc.double().abs() + e) * (torch.ones_like(e) if against_exact else (e > 0).double())


def _sum(a, e_a, b, e_b):   # one float32 sum (or difference: hand in -b)
    v = a + b
    e = e_a + e_b
    return v, e + ulp(F32, v.abs() + e)


def _prod(a, e_a, b, e_b):
    v = a * b
    e = a.abs() * e_b + b.abs() * e_a + e_a * e_b
    return v, e + ulp(F32, v.abs() + e)


def warp(x, t_row, blocks, dtype, encoders, exact=False, against_exact=False):
    """x [N, 3] float32, t_row [N, 9] the encoded time (``dtype``), encoders = (enc_uv, enc_w): float32 [N, D] -> rows of ``dtype``.
    Returns dict(warped float64 [N, 3], e_warped, dw, theta, tr: the largest magnitudes).  ``exact``: every rounding is a no-op and
    the float32 sums are rounded as the kernel rounds them; otherwise the values stay float64 and the bound covers the roundings."""
    enc_uv, enc_w = encoders
    p, e = x.double(), torch.zeros(x.shape, dtype=torch.float64)
    e_t = enc_err(t_row, torch.zeros(x.shape[0], 1, dtype=torch.float64), dtype, against_exact=against_exact)
    seen = dict(dw=0.0, theta=0.0, tr=0.0)
    f32 = lambda v: v.float().double() if exact else v

    def net(row, e_row, ws, bs, out_f32):
        if exact:
            r = S.forward(row, ws, bs, 0, dtype, out_f32=out_f32, exact=True)
        else:
            r = M.forward_with_error(row.double(), e_row, ws, bs, 0, dtype, out_f32=out_f32)
        return r["y"], r["e_y"]

    for i, blk in enumerate(blocks):
        (u, v, w), (e_u, e_v, e_w) = p.split(1, 1), e.split(1, 1)
        f1, e_f1 = net(t_row, e_t, [blk["t1"][0]], [blk["t1"][1]], False)
        r1 = enc_uv(torch.cat([u, v], 1).float())
        dw, e_dw = net(torch.cat([r1.cpu(), f1.to(dtype)], 1), torch.cat([enc_err(r1.cpu(), torch.cat([e_u, e_v], 1), dtype, against_exact=against_exact), e_f1], 1), *blk["n1"], True)
        w, e_w = _sum(w, e_w, dw, e_dw)
        f2, e_f2 = net(t_row, e_t, [blk["t2"][0]], [blk["t2"][1]], False)
        r2 = enc_w(w.float())
        rt, e_rt = net(torch.cat([r2.cpu(), f2.to(dtype)], 1), torch.cat([enc_err(r2.cpu(), e_w, dtype, against_exact=against_exact), e_f2], 1), *blk["n2"], True)
        th, e_th = rt[:, :1], rt[:, :1] * 0 + e_rt[:, :1]
        s, c = torch.sin(th), torch.cos(th)
        e_sc = e_th.clamp_max(2.0) + SINCOS * (0 if exact else 1)
        du, e_du = _sum(u, e_u, -rt[:, 1:2], e_rt[:, 1:2])
        dv, e_dv = _sum(v, e_v, -rt[:, 2:3], e_rt[:, 2:3])
        du, dv = f32(du), f32(dv)
        (cu, e_cu), (sv, e_sv), (su, e_su), (cv, e_cv) = _prod(c, e_sc, du, e_du), _prod(s, e_sc, dv, e_dv), _prod(s, e_sc, du, e_du), _prod(c, e_sc, dv, e_dv)
        (u, e_u), (v, e_v) = _sum(cu, e_cu, sv, e_sv), _sum(cv, e_cv, -su, e_su)
        seen = dict(dw=max(seen["dw"], float(dw.abs().max())), theta=max(seen["theta"], float(th.abs().max())), tr=max(seen["tr"], float(rt[:, 1:].abs().max())))
        order = ([1, 2, 0], [2, 0, 1], [0, 1, 2])[i]
        p, e = torch.cat([f32(u), f32(v), f32(w)], 1)[:, order], torch.cat([e_u, e_v, e_w], 1)[:, order]
    return dict(warped=p, e_warped=e, **seen)


def golden_bound(blocks, f, x, t, dtype):
    """warp()'s dict, e_warped the bound on |the composed chain's warp on CPU tensors (torch's encoders) - the reference's in float64|."""
    with torch.no_grad():
        w = warp(x, f.time_encoder(t), blocks, dtype, (f.posi_encoder_1, f.posi_encoder_2), against_exact=True)
    return {**w, "e_warped": w["e_warped"] + ulp(F32, w["warped"].abs())}
