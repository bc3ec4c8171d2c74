"""The float64 restatement of the warp stage of the fused T-NeRF query (csrc/nerf_field.hip, WARP): the 36-wide row [enc(x), enc(t)] as
the native encoders store it, the warp network by the rules of tests/mlp_bias_skip_reference.py with a float32 output that is never
rounded, and x' = x + delta as ONE float32 sum.  Behind x' the query is tests/nerf_field_reference.py's."""
import torch

import mlp_bias_skip_reference as S
import mlp_stream_reference as M
import nerf_field_reference as F
from mlp_reference import ulp, worst_ratio  # noqa: F401

WARP_DIMS, WARP_W = 36, 64
MASK = S.skip_mask_of(2, 4)   # 8: layer 3 takes [H_2, row]
# Columns of the row: 0 .. 2 x, 3 .. 14 sin(2^k x_d), 15 .. 26 the cosines, 27 t, 28 .. 31 sin(2^k t), 32 .. 35 cos.  At the reference's
# shape perm_weights gives delta_0 = relu(column 6), a sine, delta_2 = relu(column 24), a cosine, delta_1 = 2 relu(column (6 + roll) % 36):
ROLL = {"pos_identity": 31, "pos_sine": 0, "time_identity": 21, "time_sine": 23}   # columns 1, 6, 27, 29
# the golden fixture's fields (scripts/gen_tnerf_golden.py): net_depth, net_width, skip_layer of the NeRF network, the warp's weights
FIELDS = {"ref": (8, 256, 4, "xavier"), "small": (2, 128, 4, "xavier"), "perm": (2, 128, 4, "perm")}


def perm_weights(roll, depth=4, mask=MASK):
    """The 'perm' family with ONE term in every sum (nerf_field_reference.perm_weights' rule at a cat layer), zero biases."""
    ws = S.exact_weights("perm", WARP_DIMS, 3, WARP_W, depth, mask)
    for l in range(1, depth + 1):
        if S.is_cat(mask, l):
            odd = (torch.arange(ws[l].shape[0]) % 2 == 1).view(-1, 1)
            ws[l] = torch.cat([ws[l][:, :WARP_W] * ~odd, ws[l][:, WARP_W:] * odd], 1)
    ws[0] = torch.roll(ws[0], roll, 1)
    return ws, [torch.zeros(w.shape[0]) for w in ws]


def xavier_weights(seed=23, out_scale=1.0 / 16):
    """Xavier-uniform matrices in multiples of 2^-8 (the output layer scaled: deformations of order 0.1), biases in +-0.5."""
    gen = torch.Generator().manual_seed(seed)
    dims = S.layer_dims(WARP_DIMS, 3, WARP_W, 4, MASK)
    ws = [torch.round((torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 * 256) / 256 for o, i in dims]
    ws[-1] = ws[-1] * out_scale
    return ws, [torch.rand(o, generator=gen) - 0.5 for o, _ in dims]


def reference_state_dict(name):
    """The reference module's state dict (without the encoders' buffers) of a field of FIELDS."""
    depth, width, skip, kind = FIELDS[name]
    ws, bs = xavier_weights() if kind == "xavier" else perm_weights(ROLL["time_sine"])
    names = [f"warp.hidden_layers.{i}" for i in range(4)] + ["warp.output_layer"]
    sd = {**{n + ".weight": w for n, w in zip(names, ws)}, **{n + ".bias": b for n, b in zip(names, bs)}}
    sd.update({"nerf.mlp." + k: v for k, v in M.nerf_state_dict("xavier", 63, 27, depth, width, skip, 1, 128).items()})
    return sd


def warp(row, e_row, ws, bs, dtype, exact=False, mask=MASK):
    """row [N, 36] of ``dtype`` -> dict(delta, e_delta), float32 side (``exact``: every rounding a no-op; else e_row comes in)."""
    if exact:
        r = S.forward(row, ws, bs, mask, dtype, out_f32=True, exact=True)
    else:
        r = M.forward_with_error(row.double(), e_row, ws, bs, mask, dtype, out_f32=True)
    return dict(delta=r["y"], e_delta=r["e_y"])


def warped(x, delta, e_delta):
    """x' = x + delta, one float32 sum: the value and its bound."""
    v = x.double() + delta
    return v.float(), e_delta + ulp(torch.float32, v.abs() + e_delta)


def golden_bound(f, x, t, d, dtype):
    """The bound on |composed chain on CPU tensors - the reference in float64|: dict(e_warped, e_rgb, e_sigma), outputs ACTIVATED.
    An encoded column whose x carries e_x is off by e_x (identity) or min(2, 2^k e_x) + 2^-20 (a float32 sincosf), plus its
    rounding; the trunk's 2^9 slope makes the outputs' bounds loose ("Fused T-NeRF field")."""
    def enc_err(enc, e_x, n_freqs):
        k = torch.arange(n_freqs, dtype=torch.float64).repeat_interleave(e_x.shape[1])
        trig = (e_x.repeat(1, n_freqs) * 2.0 ** k).clamp_max(2.0) + 2.0 ** -20
        e = torch.cat([e_x, trig, trig], 1)
        return e + ulp(dtype, enc.double().abs() + e)
    lin = lambda m: ([v.detach() for v in m.linear_weights()], [v.detach() for v in m.linear_biases()])
    zero = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    with torch.no_grad():
        row = torch.cat([f.posi_encoder(x), f.time_encoder(t)], -1)
        w = warp(row, torch.cat([enc_err(row[:, :27], zero, 4), enc_err(row[:, 27:], zero[:, :1], 4)], 1), *lin(f.warp), dtype)
        xw, e_xw = warped(x, w["delta"], w["e_delta"])
        enc_x, enc_d = f.nerf.posi_encoder(xw), f.nerf.view_encoder(d)
        tr, hd = f.nerf.mlp.trunk, f.nerf.mlp.head
        W = tr.n_neurons
        z = M.forward_with_error(enc_x.double(), enc_err(enc_x, e_xw, 10), *lin(tr), tr.skip_mask, dtype, out_f32=True)
        bott, e_b = F.rounded(z["y"][:, :W], z["e_y"][:, :W], dtype)
        h = M.forward_with_error(torch.cat([bott, enc_d.double()], 1), torch.cat([e_b, enc_err(enc_d, zero, 4)], 1), *lin(hd), 0, dtype, out_f32=True)
        _, e_rgb = F.rounded(*F.activated(*F.rounded(h["y"], h["e_y"], dtype), dtype, True), dtype)
        _, e_sigma = F.rounded(*F.activated(*F.rounded(z["y"][:, W:], z["e_y"][:, W:], dtype), dtype, False), dtype)
    return dict(e_warped=e_xw, e_rgb=e_rgb, e_sigma=e_sigma)


def make_inputs(N, rays, dev):
    """The launch's inputs and the (positions, times [N, 1], directions) they mean.  Rays: seven, ray 2 without a sample."""
    from nerfacc_amd.samples import sample_positions
    gen = torch.Generator().manual_seed(7 + N)
    rand = lambda *s: torch.rand(*s, generator=gen).to(dev)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).to(dev)
    if not rays:
        x, t, d = rand(N, 3) * 3.0 - 1.5, rand(N, 1), unit(N)
        return dict(positions=x, dirs=d, times=t.view(-1)), x, t, d
    o, stamps, d = rand(7, 3) - 0.5, rand(7, 1), unit(7)
    ri = torch.sort(torch.tensor([0, 1, 3, 4, 5, 6])[torch.randint(0, 6, (N,), generator=gen)]).values.to(dev)
    ts = rand(N) * 2.0
    s = sample_positions(o, d, ts, ts + 0.01, ri, dirs="raw")
    return dict(rays=(o, d, ts, ts + 0.01, ri), times=stamps.view(-1)), s.positions, stamps[ri], s.dirs
