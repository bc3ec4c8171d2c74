"""Helpers of the streamed-weight MLP tests (nerfacc_amd/csrc/mlp_stream.hip, nerfacc_amd.mlp.StreamedMLP and NerfMLP).  The
float64 restatement, its rounding points and its bound rule are those of tests/mlp_bias_skip_reference.py, which is
width-agnostic; this module adds

  * the integer-valued cases at 128 / 256 neurons and up to 8 hidden layers, with the hidden neurons RELABELLED per case
    (``shift``: neuron j becomes neuron (j + shift) mod W, which changes no value and moves every column of every H_l and
    dZ_l), so that the cases taken together drive every column and every 32 x 32 tile of every dW_l;
  * the same recursion with an input that already carries an error (the colour head behind the trunk), and a backward whose
    incoming gradient carries one (the trunk behind the colour head);
  * the deterministic weights of the NerfMLP golden fixture (tests/golden/ref_nerf_mlp.npz, scripts/gen_nerf_mlp_golden.py)
    and their checksum.
"""
import torch

import mlp_bias_skip_reference as S
import mlp_reference as R
from mlp_reference import U32, rnd, ulp, worst_ratio  # noqa: F401

T = 128          # points a workgroup carries through one pass of the image (NFA_MLP_STREAM_POINTS)
GROUPS = 256     # workgroups of the persistent grid at most (NFA_MLP_STREAM_GROUPS)
SLOTS = 2        # slots of the ring


def relabelled(ws, bs, width, shift):
    """Hidden neuron j -> (j + shift) mod width in every layer: rows of W_l, l < L, and the H columns of W_l, l >= 1."""
    L = len(ws) - 1
    out_w = []
    for l, w in enumerate(ws):
        if l >= 1:
            w = torch.cat([torch.roll(w[:, :width], shift, 1), w[:, width:]], 1)
        if l < L:
            w = torch.roll(w, shift, 0)
        out_w.append(w.contiguous())
    out_b = None if bs is None else [torch.roll(b, shift, 0) if l < L else b for l, b in enumerate(bs)]
    return out_w, out_b


def exact_case(case, dtype):
    """case = (family, width, n_hidden, skip_layer, bias, (N, n_in, n_out, x float32?, y and g float32?), shift).  Returns
    (shape, skip_mask, ws, bs, x, g, forward, backward); every rounding is asserted to be a no-op."""
    family, width, n_hidden, skip_layer, bias, cfg, shift = case
    N, n_in, n_out, x_f32, out_f32 = cfg
    shape = (n_in, n_out, width, n_hidden)
    skip_mask = S.skip_mask_of(skip_layer, n_hidden)
    ws = S.exact_weights(family, *shape, skip_mask)
    bs = S.exact_biases(n_out, width, n_hidden) if bias else None
    ws, bs = relabelled(ws, bs, width, shift)
    x, g = R.exact_inputs(N, n_in, n_out, torch.float32 if x_f32 else dtype, torch.float32 if out_f32 else dtype)
    f = S.forward(x, ws, bs, skip_mask, dtype, out_f32, exact=True)
    b = S.backward(x, ws, f["hidden"], g, skip_mask, dtype, exact=True)
    return shape, skip_mask, ws, bs, x, g, f, b


def case_id(c):
    return f"{c[0]}-W{c[1]}-L{c[2]}-skip{c[3]}-bias{int(c[4])}-N{c[5][0]}-in{c[5][1]}-out{c[5][2]}-shift{c[6]}"


# The trunk's own shape, 63 -> 8 x 256 -> 257 with the input appended after hidden layer 4.  Taken together these cases drive
# every column of every dZ_l and every 32 x 32 tile of every dW_l (tests/test_mlp_stream_cpu.py asserts it on the reference).
TRUNK_CASES = [
    ("perm", 256, 8, 4, True, (300, 63, 257, True, False), 0),
    ("perm", 256, 8, 4, True, (257, 63, 257, False, True), 37),
    ("perm", 256, 8, 4, False, (300, 63, 257, True, True), 101),
    ("perm", 256, 8, 4, True, (129, 63, 257, False, False), 170),
]

# The covering set.  N: 1, 31, 33, T - 1, T, T + 1, 300 (two weight-gradient slices, the second short);
# depths 1, 2, SLOTS + 1 = 3 and 8; widths 128 and 256; n_in 5 (element-wise loads), 36 (rows of 72 B), 63, 283, 320 (16-byte
# rows, ten 32-column dx blocks); n_out 1, 3, 32, 33, 257, 288 (nine output row tiles); bias only, skip only, both; a cat OUTPUT
# layer (n_hidden 3 with skip_layer 2, n_hidden 2 with skip_layer 1); cat layers at every layer from 2 on (skip_layer 1); a
# skip_layer that selects nothing; float32 and half ends.
CASES = TRUNK_CASES + [
    # bias only
    ("dense", 128, 1, None, True, (1, 5, 1, True, True), 0),
    ("dense", 256, 2, None, True, (31, 36, 3, False, False), 0),
    ("perm", 256, 3, None, True, (33, 320, 32, False, True), 5),
    ("perm", 128, 8, None, True, (300, 5, 3, False, False), 0),
    # skip only
    ("perm", 128, 3, 2, False, (T - 1, 283, 33, True, False), 0),       # cat output layer of 128 + 283 inputs
    ("perm", 256, 2, 1, False, (T, 36, 288, False, True), 0),           # cat output layer, nine output row tiles
    ("perm", 256, 8, 1, False, (33, 320, 288, False, False), 64),       # seven cat layers, the largest piece (36 KiB)
    # both
    ("perm", 256, 3, 1, True, (T + 1, 63, 257, True, True), 9),         # an inner cat layer and a cat output layer
    ("perm", 128, 8, 3, True, (300, 36, 32, True, False), 3),           # cat layers 4 and 7
    ("dense", 128, 2, 1, True, (300, 283, 3, True, True), 0),           # the colour head's input width, element-wise rows
    ("perm", 256, 1, None, True, (T + 1, 283, 3, False, False), 0),
    ("perm", 256, 3, 4, True, (300, 63, 1, False, True), 0),            # a skip_layer that selects nothing
]

# Just beyond a full sweep of the persistent grid plus a partial tile: GROUPS x T points, two more full tiles and 7 points.
SWEEP_CASE = ("perm", 256, 2, None, True, (GROUPS * T + 2 * 32 + 7, 36, 3, False, False), 0)


# ---------------------------------------------------------------- the bound recursion with errors coming in

def forward_with_error(x0, e_x, weights, biases, skip_mask, dtype, out_f32=False):
    """mlp_bias_skip_reference.forward for an input x0 (float64 values of ``dtype`` numbers, not rounded again) that carries
    the error e_x: the same recursion started from e_x; the x columns of a cat layer carry e_x too.  Returns the same dict."""
    h, e = x0, e_x
    hidden, e_hidden, zs, e_zs = [], [], [], []
    for l, w in enumerate(weights):
        wq = rnd(w.double(), dtype)
        cat = S.is_cat(skip_mask, l)
        hin = torch.cat([h, x0], 1) if cat else h
        ein = torch.cat([e, e_x], 1) if cat else e
        b = biases[l].double() if biases is not None else torch.zeros(wq.shape[0], dtype=torch.float64)
        z = hin @ wq.t() + b
        s_abs = hin.abs() @ wq.abs().t() + b.abs()
        e_pre = ein @ wq.abs().t() + (wq.shape[1] + 2 + (biases is not None)) * U32 * s_abs
        if l < len(weights) - 1:
            h = rnd(torch.relu(z), dtype)
            e = e_pre + ulp(dtype, z.abs() + e_pre)
            hidden.append(h)
            e_hidden.append(e)
            zs.append(z)
            e_zs.append(e_pre)
        elif out_f32:
            y, e_y = z, e_pre
        else:
            y, e_y = rnd(z, dtype), e_pre + ulp(dtype, z.abs() + e_pre)
    return dict(y=y, hidden=hidden, e_y=e_y, e_hidden=e_hidden, z=zs, e_z=e_zs)


def backward_with_error(x0, e_x, weights, g, e_g, skip_mask, dtype, free, x_dtype):
    """mlp_bias_skip_reference.backward(..., free=free) between two sides that share neither the input nor the incoming
    gradient: x0 (float64 values of ``dtype`` numbers) carries e_x, g (float64, rounded here as the kernel rounds it) carries
    e_g, so dZ_L = rnd(g) is off by e_g plus the rounding of a perturbed number, and dW_l gains (|dZ_l| + e_dZ)^T e_in at every
    layer, layer 0 included.  ``free`` is the forward's dict (its hidden are the H_l).  dx is rounded to x_dtype."""
    N, W = x0.shape[0], weights[0].shape[0]
    hidden = free["hidden"]
    dz = rnd(g, dtype)
    e = e_g + torch.where((dz == g) & (e_g == 0), torch.zeros_like(g), ulp(dtype, g.abs() + e_g))
    L = len(weights)
    dzs, e_dzs, dws, e_dws, dbs, e_dbs = [dz], [e], [], [], [], []
    skip_dx, skip_e, skip_abs, skip_K = 0.0, 0.0, 0.0, 0
    for l in range(L - 1, -1, -1):
        h_prev, e_prev = (hidden[l - 1], free["e_hidden"][l - 1]) if l > 0 else (x0, e_x)
        cat = S.is_cat(skip_mask, l)
        hin = torch.cat([h_prev, x0], 1) if cat else h_prev
        e_hin = torch.cat([e_prev, e_x], 1) if cat else e_prev
        dws.append(dz.t() @ hin)
        s_abs = dz.abs().t() @ hin.abs()
        e_dws.append(e.t() @ hin.abs() + (N + 2) * U32 * s_abs + ulp(torch.float32, s_abs) + (dz.abs() + e).t() @ e_hin)
        dbs.append(dz.sum(0))
        b_abs = dz.abs().sum(0)
        e_dbs.append(e.sum(0) + (N + 2) * U32 * b_abs + ulp(torch.float32, b_abs))
        wq = rnd(weights[l].double(), dtype)
        K = wq.shape[0]
        if l > 0:
            wh = wq[:, :W]
            if cat:   # the x columns feed dx only
                wx = wq[:, W:]
                skip_dx = skip_dx + dz @ wx
                skip_e = skip_e + e @ wx.abs()
                skip_abs = skip_abs + dz.abs() @ wx.abs()
                skip_K += K
            dh = dz @ wh
            e_pre = e @ wh.abs() + (K + 2) * U32 * (dz.abs() @ wh.abs())
            mask = (h_prev > 0).double()
            dz = rnd(torch.where(h_prev > 0, dh, torch.zeros_like(dh)), dtype)   # a select
            e = (e_pre + ulp(dtype, dh.abs() + e_pre)) * mask
            unsure = free["z"][l - 1].abs() <= free["e_z"][l - 1]
            e = torch.where(unsure, dh.abs() + e_pre + ulp(dtype, dh.abs() + e_pre), e)
            dzs.append(dz)
            e_dzs.append(e)
        else:
            dh = dz @ wq + skip_dx
            s_abs = dz.abs() @ wq.abs() + skip_abs
            e_pre = e @ wq.abs() + skip_e + (K + skip_K + 2) * U32 * s_abs
            dx = rnd(dh, x_dtype)
            e_dx = e_pre + ulp(x_dtype, dh.abs() + e_pre)
    return dict(dx=dx, e_dx=e_dx, dz=dzs[::-1], e_dz=e_dzs[::-1], dw=dws[::-1], e_dw=e_dws[::-1], db=dbs[::-1], e_db=e_dbs[::-1])


# ---------------------------------------------------------------- the NerfMLP golden fixture's weights

def nerf_reference_keys(depth, depth_c, condition):
    names = [f"base.hidden_layers.{i}" for i in range(depth)] + ["sigma_layer.output_layer"]
    if condition:
        names += ["bottleneck_layer.output_layer"] + [f"rgb_layer.hidden_layers.{i}" for i in range(depth_c)]
    return names + ["rgb_layer.output_layer"]


def nerf_state_dict(kind, input_dim, condition_dim, depth=8, width=256, skip_layer=4, depth_c=1, width_c=128):
    """The state dict of the reference's NerfMLP that the golden fixture was made with, by a deterministic rule (the fixture
    stores only a checksum of it).
      exact   the 'perm' family and the integer biases of mlp_bias_skip_reference for the trunk with its merged output matrix
              (rows 0 .. width-1 bottleneck, row width sigma; without a condition rows 0 .. 2 colour, row 3 sigma) and for the
              colour head: every number of the float64 run is a small integer.
      xavier  Xavier uniform per reference layer from a generator seeded 11, rounded to multiples of 2^-8; biases uniform in
              +-0.5, float32."""
    cond = condition_dim > 0
    mask = S.skip_mask_of(skip_layer, depth)
    n_out = width + 1 if cond else 4
    dims = S.layer_dims(input_dim, n_out, width, depth, mask)
    dims_c = S.layer_dims(width + condition_dim, 3, width_c, depth_c, 0) if cond else []
    if kind == "exact":
        ws, bs = S.exact_weights("perm", input_dim, n_out, width, depth, mask), S.exact_biases(n_out, width, depth)
        ws_c, bs_c = (S.exact_weights("dense", width + condition_dim, 3, width_c, depth_c, 0), S.exact_biases(3, width_c, depth_c)) if cond else ([], [])
    else:
        gen = torch.Generator().manual_seed(11)
        split = (width,) if cond else (3,)
        def xavier(o, i):
            return torch.round((torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (o + i)) ** 0.5 * 256) / 256
        ws = [xavier(o, i) for o, i in dims[:-1]]
        ws.append(torch.cat([xavier(split[0], dims[-1][1]), xavier(1, dims[-1][1])]))   # each block with its own fan
        ws_c = [xavier(o, i) for o, i in dims_c]
        bs = [torch.rand(o, generator=gen) - 0.5 for o, _ in dims]
        bs_c = [torch.rand(o, generator=gen) - 0.5 for o, _ in dims_c]
    sd = {}
    for i in range(depth):
        sd[f"base.hidden_layers.{i}.weight"], sd[f"base.hidden_layers.{i}.bias"] = ws[i], bs[i]
    first = "bottleneck_layer.output_layer" if cond else "rgb_layer.output_layer"
    r = width if cond else 3
    sd[first + ".weight"], sd[first + ".bias"] = ws[depth][:r].clone(), bs[depth][:r].clone()
    sd["sigma_layer.output_layer.weight"], sd["sigma_layer.output_layer.bias"] = ws[depth][r:].clone(), bs[depth][r:].clone()
    if cond:
        for i in range(depth_c):
            sd[f"rgb_layer.hidden_layers.{i}.weight"], sd[f"rgb_layer.hidden_layers.{i}.bias"] = ws_c[i], bs_c[i]
        sd["rgb_layer.output_layer.weight"], sd["rgb_layer.output_layer.bias"] = ws_c[depth_c], bs_c[depth_c]
    return sd


def checksum(sd):
    """A float64 number that moves when any entry of the state dict moves: sum over the sorted keys of <v, weights>, the
    weights 1 + (index mod 251) / 251."""
    total = 0.0
    for k in sorted(sd):
        v = sd[k].double().reshape(-1)
        total += float((v * (1.0 + (torch.arange(v.numel(), dtype=torch.float64) % 251) / 251)).sum())
    return total
