"""Case tables and helpers of the number-format edge tests of the fused MLPs (tests/test_mlp_edges_cpu.py and
tests/test_mlp_edges_gpu.py): the same tables drive the modules' torch path and the kernels.  No GPU here.

The float64 restatements (mlp_reference, mlp_grad2_reference, mlp_bias_skip_reference) are the oracle, as they are for the
exact tests; what is new is the data.  The contract (csrc/mlp.hip, "Number-format edges"):

  1. every rounding point is one round-to-nearest-even of the exact float32 value over the whole range: fp16 subnormals are
     kept (gradual underflow, ties to even), a value at or above MAX + ulp/2 becomes +-inf, one float32 step below it MAX;
  2. fp16 subnormals reach the MFMA un-flushed, as packed weights (A) and as x, H_l, dZ_l fragments (B);
  3. relu(NaN) = NaN, relu(-inf) = 0, relu(+inf) = +inf; the backward's and the tangent's mask is a select on H > 0
     (the sign of a zero is not compared: a value that underflows to -0 is as good as the restatement's +0);
  4. a non-finite value in row p of x, g or v changes row p of the per-point arrays and nothing else in them;
  5. dL/dparams is NaN / +inf / -inf / finite exactly where the restatement is, finite elements bit for bit;
  6. an overflow born inside the backward kernel reaches dL/dparams as inf or NaN, so DeviceGradScaler skips the step.

SCALED cases.  An exact case (integer-valued x, g, v, W_l, b_l; every rounding a no-op) with x, g, v and each W_l multiplied
by a power of two (the x columns of a cat layer and the biases by the powers that keep every term of a sum on one grid).
Every operand of every product is then an integer times a power of two, and :func:`product` asserts for every sum that its
terms are multiples of one quantum q with sum |terms| < 2^24 q: the float32 accumulator holds every partial sum exactly,
whatever the order, and each stored half is ONE rounding of a known value -- the comparison stays bit for bit although the
roundings no longer are no-ops.  Infinite and NaN terms are order-free too (inf + finite = inf, inf - inf = NaN in any order)
as long as the finite terms cannot overflow float32 on their way, which :func:`product` asserts as well.

  underflow (fp16): x * 2^-25, g * 2^-24 and weights * 2^-1: everything the passes store is an fp16 subnormal, with ties.
  overflow:         products that pass MAX of the half type, one sub-case per rounding point (an infinity in H_l floods the
                    rows behind it with NaN).  In bf16 MAX is within a factor 1.002 of float32's, so a sum that rounds to inf
                    in bf16 and is finite in float32 needs the integer 511 or 1023 in the accumulator, which the exact
                    families do not produce (the BOUNDARY rows do).  The bf16 overflow cases therefore use the 'perm' family,
                    where a sum has ONE product (and, lower by 2^-8, a bias and the x share of a cat layer): a product at or
                    above 2^129 is inf in float32 whatever it is added to first, and so in bf16.  What a pass stores as
                    float32 is that accumulator (:func:`restate` rounds the restatement's float64 once to float32).

:func:`audit` recomputes the value before each rounding from the restatement's own tensors and counts, per rounding point,
the subnormal results, the subnormal ties by direction and the infinities born there (finite before, infinite after).
"""
from types import SimpleNamespace

import torch

import mlp_bias_skip_reference as S
import mlp_grad2_reference as G
import mlp_reference as R
import mlp_stream_reference as Q

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16]
HALF_MAX = {F16: 65504.0, BF16: 255.0 * 2.0 ** 120}
HALF_TOP_ULP = {F16: 32.0, BF16: 2.0 ** 120}          # spacing of the half type just below MAX
F32_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127
F16_MIN_NORMAL, F16_QUANTUM = 2.0 ** -14, 2.0 ** -24
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- comparison

def classes(t):
    return torch.isnan(t), torch.isposinf(t), torch.isneginf(t)


def same_class_and_bits(got, want):
    """The NaN, +inf and -inf sets are equal, and every other element has the same value (NaN sign and payload are not
    compared; -0 equals +0, as in the exact tests).  Nothing is left out: an element is in one of the three sets or compared."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if got.shape != want.shape:
        return False
    special = torch.zeros_like(want, dtype=torch.bool)
    for a, b in zip(classes(got), classes(want)):
        if not torch.equal(a, b):
            return False
        special |= b
    return torch.equal(got[~special], want[~special])


def explain(got, want):
    """What differs, for an assertion message."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    for name, a, b in zip(("nan", "+inf", "-inf"), classes(got), classes(want)):
        if not torch.equal(a, b):
            i = tuple(int(k) for k in (a != b).nonzero()[0])
            return f"{name} sets differ at {int((a != b).sum())} elements, first {i}: got {float(got[i])}, want {float(want[i])}"
    ne = (got != want) & ~torch.isnan(want)
    if bool(ne.any()):
        i = tuple(int(k) for k in ne.nonzero()[0])
        return f"{int(ne.sum())} finite elements differ, first {i}: got {float(got[i])!r}, want {float(want[i])!r}"
    return "equal"


def matmul_is_ieee():
    """The restatements' float64 matmul must not skip zeros: inf * 0 = NaN.  [40, 64] with one inf times a one-hot matrix."""
    a = torch.ones(40, 64, dtype=torch.float64)
    a[17, 5] = INF
    w = torch.zeros(64, 64, dtype=torch.float64)
    w[9, 5] = 1.0                       # output 9 reads input 5
    row = (a @ w.t())[17]
    clean = torch.cat([(a @ w.t())[:17], (a @ w.t())[18:]])
    return int(torch.isnan(row).sum()) == 63 and bool(torch.isposinf(row[9])) and bool(torch.isfinite(clean).all())


# ---------------------------------------------------------------- networks and base cases

# name: (kind, width, n_hidden, skip_layer, bias, (N, n_in, n_out)).  kind: "plain" = the nfa_mlp_* entries (FusedMLP without
# bias and skip; the one with the second order here), "net" = nfa_mlp_net_* (bias and skip), "stream" = nfa_mlp_stream_*.
# N: 33 (a partial tile behind a full one), 129 (a partial tile behind a streamed workgroup's 128 points), 300 (two
# weight-gradient slices).  n_in 32 (16-byte rows), 31 and 283 (element-wise loads), 36 (rows of 72 B); 283 >= 256 also gives
# every column of the 'perm' W_0 one entry, so that a dL/dx sum has one term per layer that feeds it.
NETS = {
    "plain-64x2": ("plain", 64, 2, None, False, (33, 32, 16)),
    "plain-128x1": ("plain", 128, 1, None, False, (129, 31, 3)),
    "net-64x3-bias-skip2": ("net", 64, 3, 2, True, (300, 36, 3)),
    "stream-256x2": ("stream", 256, 2, None, False, (129, 36, 3)),
    "stream-256x3-bias-skip2": ("stream", 256, 3, 2, True, (300, 283, 33)),
}


def has_second_order(net):
    return NETS[net][0] == "plain" and NETS[net][2] == 2


def base_case(net, dtype, family, f32_ends, N=None):
    """An existing exact case, asserted exact by its own module (exact=True: every rounding is a no-op), as a namespace:
    net, kind, dtype, shape, skip_layer, skip_mask, ws, bs, x, g, v, out_f32."""
    kind, width, n_hidden, skip_layer, bias, (n_pts, n_in, n_out) = NETS[net]
    cfg = (N or n_pts, n_in, n_out, f32_ends, f32_ends)
    if kind == "plain":
        shape, ws, x, g, v, *_ = G.exact_case(family, dtype, width, n_hidden, cfg)
        bs, skip_mask = None, 0
    elif kind == "net":
        shape, skip_mask, ws, bs, x, g, v, *_ = S.exact_case(family, dtype, width, n_hidden, cfg, bias, skip_layer)
    else:
        shape, skip_mask, ws, bs, x, g, *_ = Q.exact_case((family, width, n_hidden, skip_layer, bias, cfg, 0), dtype)
        v = G.exact_tangent_input(cfg[0], n_in, x.dtype)
    return SimpleNamespace(net=net, kind=kind, dtype=dtype, shape=shape, skip_layer=skip_layer, skip_mask=skip_mask, ws=ws, bs=bs,
                           x=x, g=g, v=v, out_f32=f32_ends, second=has_second_order(net))


def custom_case(net, kind, dtype, shape, ws, x, g, v, out_f32, second):
    return SimpleNamespace(net=net, kind=kind, dtype=dtype, shape=shape, skip_layer=None, skip_mask=0, ws=ws, bs=None, x=x, g=g, v=v,
                           out_f32=out_f32, second=second)


def restate(c, x=None, g=None, v=None):
    """The float64 restatement of case ``c`` (optionally on other x, g, v): namespace f, b, s (None without a second order), dp
    and d2p (the flat gradients in the module's layout: matrices, then biases; the second order's bias segment is zero)."""
    x, g, v = (c.x if x is None else x), (c.g if g is None else g), (c.v if v is None else v)
    s = None
    if c.kind == "plain":
        f = R.forward(x, c.ws, c.dtype, c.out_f32)
        b = R.backward(x, c.ws, f["hidden"], g, c.dtype)
        if c.second:
            s = G.second_order(v, c.ws, f["hidden"], b["dz"], c.dtype, c.out_f32)
    else:
        f = S.forward(x, c.ws, c.bs, c.skip_mask, c.dtype, c.out_f32)
        b = S.backward(x, c.ws, f["hidden"], g, c.skip_mask, c.dtype)
        if c.second:
            s = S.second_order(v, c.ws, f["hidden"], b["dz"], c.skip_mask, c.dtype, c.out_f32)
    # What is stored as float32 is the float32 accumulator: a no-op, except that a single product at or above 2^128 (the bf16
    # overflow cases) is inf there.  audit() asserts that no float32 sum overflows in any other way.
    f32 = lambda t: t.float().double()
    if c.out_f32:
        f["y"] = f32(f["y"])
        if s is not None:
            s["u"] = f32(s["u"])
    if x.dtype == F32:
        b["dx"] = f32(b["dx"])
    n_bias = sum(w.shape[0] for w in c.ws) if c.bs is not None else 0
    dp = f32(S.flat_params(b["dw"], b["db"] if c.bs is not None else None))
    d2p = f32(torch.cat([R.flat(s["dw"]), torch.zeros(n_bias, dtype=torch.float64)])) if s is not None else None
    return SimpleNamespace(f=f, b=b, s=s, dp=dp, d2p=d2p)


# ---------------------------------------------------------------- scaling

def scaled(c, ex, eg, ev, ew, eb=0):
    """``c`` with x * 2^ex, g * 2^eg, v * 2^ev, W_l * 2^ew[l]; the x columns of a cat layer l by 2^(ew_0 + .. + ew_{l-1}) more
    and b_l by 2^(ex + ew_0 + .. + ew_l), so that all terms of every sum keep one power of two.  ``eb`` < 0 puts the biases and
    the x columns of the cat layers 2^eb lower, on a finer grid of the same sums: where the products of a layer are to pass
    2^128, -40 times their power would leave float32, and two terms of that size would make the sum depend on its order.  The
    masters stay exact."""
    W = c.shape[2]
    cum = [sum(ew[:l]) for l in range(len(c.ws) + 1)]
    ws = []
    for l, w in enumerate(c.ws):
        w2 = w.double() * 2.0 ** ew[l]
        if S.is_cat(c.skip_mask, l):
            w2[:, W:] *= 2.0 ** (cum[l] + eb)
        assert torch.equal(w2.float().double(), w2) and torch.equal(R.rnd(w2, c.dtype), w2 + 0.0), "a scaled master must stay exact"
        ws.append(w2.float())
    bs = None
    if c.bs is not None:
        bs = [(b.double() * 2.0 ** (ex + cum[l + 1] + eb)).float() for l, b in enumerate(c.bs)]
        assert all(torch.equal(b2.double(), b.double() * 2.0 ** (ex + cum[l + 1] + eb)) for l, (b, b2) in enumerate(zip(c.bs, bs)))
    out = SimpleNamespace(**vars(c))
    out.ws, out.bs = ws, bs
    out.x = (c.x.double() * 2.0 ** ex).to(c.x.dtype)
    out.g = (c.g.double() * 2.0 ** eg).to(c.g.dtype)
    out.v = (c.v.double() * 2.0 ** ev).to(c.v.dtype)
    return out


def quantum(t, dim):
    """Per row (``dim=1``) or column (``dim=0``) of the finite float64 matrix ``t``: the largest power of two that divides every
    non-zero element of it (2^1000 for a row of zeros)."""
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double().clamp_min(1.0)
    exp = torch.where(t != 0, e.double() - 53 + torch.log2(low).round(), torch.full_like(t, 1000.0))
    return torch.exp2(exp.min(dim).values)


def product(a, b, dtype, where, split=None, add=None):
    """a @ b in float64, after asserting that a float32 accumulator gives the same number in any order of summation: for
    every element the finite non-zero terms are multiples of one power of two q with sum |terms| < 2^24 q, q is a normal
    float32 number, and the terms cannot overflow float32 on their way unless there is just one.  q is the row's of ``a`` times
    the column's of ``b``; ``split``: the column(s) of ``a`` where a block with a power of its own starts (the x part of a cat layer's
    input; the cat layers' shares of dL/dx); ``add``: the float32 bias the accumulator starts from, one more term of every sum."""
    fa = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    fb = torch.where(torch.isfinite(b), b, torch.zeros_like(b))
    s_abs, n_terms, q, largest, single = 0.0, 0.0, None, 0.0, True
    cuts = [0] + ([] if split is None else [split] if isinstance(split, int) else list(split)) + [a.shape[1]]
    for k0, k1 in zip(cuts[:-1], cuts[1:]):
        pa, pb = fa[:, k0:k1], fb[k0:k1]
        part = pa.abs() @ pb.abs()
        q_part = torch.where(part > 0, quantum(pa, 1).view(-1, 1) * quantum(pb, 0).view(1, -1), torch.full_like(part, 2.0 ** 1000))
        q = q_part if q is None else torch.minimum(q, q_part)
        n_part = (pa != 0).double() @ (pb != 0).double()
        s_abs, n_terms = s_abs + part, n_terms + n_part
        largest, single = torch.maximum(part, part * 0 + largest), (n_part <= 1) & single   # `part` is one term where n_part <= 1
    if add is not None:
        add = add.view(1, -1).expand_as(s_abs)
        q = torch.minimum(q, quantum(add, 0).view(1, -1).expand_as(s_abs))
        s_abs, largest = s_abs + add.abs(), torch.maximum(largest, add.abs())
    live = s_abs > 0
    assert bool((s_abs < 2.0 ** 24 * q)[live].all()), f"{where}: partial sums need more than 24 bits"
    assert bool((q >= 2.0 ** -126)[live].all()), f"{where}: a term below float32's normal range"
    # float32 overflow: none on the way (sum |terms| <= MAX); or ONE product and nothing else (its own float32 rounding); or one
    # term per block, the largest of which overflows whatever it is added to first (largest - rest >= 2^128)
    rest = s_abs - largest
    ok = (s_abs <= F32_MAX) | ((n_terms <= 1) & (s_abs == largest)) | (single & (largest - rest >= 2.0 ** 128))
    assert bool(ok.all()), f"{where}: finite terms can overflow float32 on their way"
    return a @ b if add is None else a @ b + add


def audit(c, r=None):
    """{rounding point: namespace(pre, post, sub, tie_down, tie_up, born_inf)} for case ``c``.  ``pre`` is the exact value before
    the rounding, recomputed from the restatement's tensors through :func:`product`."""
    r = r or restate(c)
    dtype, W, H = c.dtype, c.shape[2], c.shape[3]
    wq = [R.rnd(w.double(), dtype) for w in c.ws]
    x0 = R.rnd(c.x.double(), dtype)
    cat = lambda h, tail, l: torch.cat([h, tail], 1) if S.is_cat(c.skip_mask, l) else h
    zeros = torch.zeros_like
    pts = {}
    if c.x.dtype == F32:
        pts["x"] = (c.x.double(), x0)
    for l, w in enumerate(c.ws):
        pts[f"W{l}"] = (w.double(), wq[l])
    hid, dz = r.f["hidden"], r.b["dz"]
    for l in range(H + 1):
        z = product(cat(hid[l - 1] if l else x0, x0, l), wq[l].t(), dtype, f"z_{l}", W if S.is_cat(c.skip_mask, l) else None,
                    c.bs[l].double() if c.bs is not None else None)
        if l < H:
            pts[f"H{l}"] = (torch.relu(z), hid[l])
        elif not c.out_f32:
            pts["y"] = (z, r.f["y"])
    if c.g.dtype == F32:
        pts["g"] = (c.g.double(), dz[H])
    for l in range(H, -1, -1):
        product(dz[l].t(), cat(hid[l - 1] if l else x0, x0, l), dtype, f"dW_{l}")
        if l > 0:
            dh = product(dz[l], wq[l][:, :W], dtype, f"dH_{l - 1}")
            pts[f"dZ{l - 1}"] = (torch.where(hid[l - 1] > 0, dh, zeros(dh)), dz[l - 1])
    cats = [l for l in range(1, H + 1) if S.is_cat(c.skip_mask, l)]   # dL/dx: ONE float32 sum over layer 0 and the cat layers
    parts = [dz[0]] + [dz[l] for l in cats]
    dh = product(torch.cat(parts, 1), torch.cat([wq[0]] + [wq[l][:, W:] for l in cats], 0), dtype, "dL/dx",
                 [sum(p.shape[1] for p in parts[:i]) for i in range(1, len(parts))])
    if c.x.dtype != F32:
        pts["dx"] = (dh, r.b["dx"])
    if r.s is not None:
        t = r.s["t"]
        if c.v.dtype == F32:
            pts["v"] = (c.v.double(), t[0])
        for l in range(H + 1):
            product(dz[l].t(), cat(t[l], t[0], l), dtype, f"d2W_{l}")
            z = product(cat(t[l], t[0], l), wq[l].t(), dtype, f"tangent z_{l}", W if S.is_cat(c.skip_mask, l) else None)
            if l < H:
                pts[f"T{l}"] = (torch.where(hid[l] > 0, z, zeros(z)), t[l + 1])
            elif not c.out_f32:
                pts["u"] = (z, r.s["u"])
    out = {}
    for name, (pre, post) in pts.items():
        sub = (post != 0) & (post.abs() < F16_MIN_NORMAL) if dtype == F16 else torch.zeros_like(post, dtype=torch.bool)
        tie = (pre.abs() < F16_MIN_NORMAL) & (torch.remainder(pre.abs() / F16_QUANTUM, 1.0) == 0.5) if dtype == F16 else sub
        born = torch.isinf(post) & torch.isfinite(pre)
        to_max = (post.abs() == HALF_MAX[dtype]) & (pre.abs() > HALF_MAX[dtype])
        out[name] = SimpleNamespace(pre=pre, post=post, sub=int(sub.sum()), tie_down=int((tie & (post.abs() < pre.abs())).sum()),
                                    tie_up=int((tie & (post.abs() > pre.abs())).sum()), born_inf=int(born.sum()),
                                    born_pos=int((born & (post > 0)).sum()), born_neg=int((born & (post < 0)).sum()),
                                    to_max_pos=int((to_max & (post > 0)).sum()), to_max_neg=int((to_max & (post < 0)).sum()))
    return out


def stored_points(c):
    """The rounding points whose result a pass STORES or hands to the next product, for the conditions on a scale set."""
    H = c.shape[3]
    pts = [f"H{l}" for l in range(H)] + [f"dZ{l}" for l in range(H)]
    if not c.out_f32:
        pts.append("y")
    if c.x.dtype != F32:
        pts.append("dx")
    if c.second:
        pts += [f"T{l}" for l in range(H)] + ([] if c.out_f32 else ["u"])
    return pts


# ---------------------------------------------------------------- hand-built boundary rows

# MAX = a * w[0]; ulp/2 = h * w[1]; "one float32 step below MAX + ulp/2" = a * w[0] + lo * w[2].  All factors are numbers of the
# half type and every product is exact in float32: fp16 65504 + 16 -> inf and 65504 + 15.9921875 -> 65504 (the largest sum of
# two fp16 products below 65520); bf16 255 * 2^120 + 2^119 -> inf and 255 * 2^120 + 32767 * 2^104 (= 217 * 151 * 2^104) -> MAX.
# unit: a positive input that keeps a path alive; gs: the scale of a gradient that only accompanies a forward probe; small: a
# weight that brings MAX back into the middle of the range; mid: the live inputs beside a float32 input at the boundary.
# The bf16 values keep every float32 sum of finite terms between 2^-126 and 2^128 (product() asserts it).
BOUNDARY = {
    F16: dict(a=2047.0, h=0.5, lo=2047.0 / 4096.0, w=(32.0, 32.0, 32.0), unit=1.0, gs=1.0, small=2.0 ** -6, mid=1.0),
    BF16: dict(a=255.0 * 2.0 ** 90, h=2.0 ** 89, lo=217.0 * 2.0 ** 84, w=(2.0 ** 30, 2.0 ** 30, 151.0 * 2.0 ** 20), unit=2.0 ** -80,
               gs=2.0 ** -40, small=2.0 ** -60, mid=2.0 ** -20),
}
BOUNDARY_N = 37                                   # the four rows at 0 .. 3 and once more at 33 .. 36, in a partial tile
BOUNDARY_ROWS = [0, 1, 2, 3, 33, 34, 35, 36]      # +hi, +lo, -hi, -lo
BOUNDARY_IN, BOUNDARY_OUT = 12, 4


def boundary_probes(net, f32_ends):
    """The rounding points of a network: x / g / v / W (inputs and masters: x, g, v only when they are float32), every H_l,
    dZ_l and T_l, and y, dx, u when they are stored as halves."""
    H = NETS[net][2]
    second = has_second_order(net)
    probes = ["W"] + [f"H{l}" for l in range(H)] + [f"dZ{l}" for l in range(H)] + ([f"T{l}" for l in range(H)] if second else [])
    if f32_ends:
        return probes + ["x", "g"] + (["v"] if second else [])
    return probes + ["y", "dx"] + (["u"] if second else [])


def boundary_case(net, dtype, f32_ends, probe):
    """A network whose value before the rounding ``probe`` is exactly MAX + ulp/2 (rows 0 and 2, signs + and -) and one float32
    step below it (rows 1 and 3) at one or two neurons; every other layer passes the first neurons through with weight 1.
    The "W" probe of fp16 also holds float32 masters at subnormal ties."""
    kind, W, H, skip_layer, bias, _ = NETS[net]
    K = BOUNDARY[dtype]
    skip_mask = S.skip_mask_of(skip_layer, H)
    n_in, n_out, N = BOUNDARY_IN, BOUNDARY_OUT, BOUNDARY_N
    end = F32 if f32_ends else dtype
    ws = [torch.zeros(o, i, dtype=torch.float64) for o, i in S.layer_dims(n_in, n_out, W, H, skip_mask)]
    for w in ws:
        for k in range(4):
            w[k, k] = 1.0
    sgn = torch.tensor([1.0, 1.0, -1.0, -1.0] * 2, dtype=torch.float64)
    hi = torch.tensor([1.0, 0.0, 1.0, 0.0] * 2, dtype=torch.float64)
    vec = torch.zeros(N, 4, dtype=torch.float64)      # the probing vector: (a, h, 0) or (a, 0, lo), signed
    vec[BOUNDARY_ROWS, 0] = sgn * K["a"]
    vec[BOUNDARY_ROWS, 1] = sgn * hi * K["h"]
    vec[BOUNDARY_ROWS, 2] = sgn * (1 - hi) * K["lo"]
    ones = torch.zeros(N, 4, dtype=torch.float64)     # what the other inputs hold: a live path of small positive numbers
    ones[BOUNDARY_ROWS, :3] = 1.0
    top = HALF_MAX[dtype] + HALF_TOP_ULP[dtype] / 2
    below = float(torch.nextafter(torch.tensor(top, dtype=F32), torch.tensor(0.0)))
    edge = torch.zeros(N, 4, dtype=torch.float64)     # a float32 input at the boundary itself
    edge[BOUNDARY_ROWS, 0] = sgn * (hi * top + (1 - hi) * below)
    wide = lambda t, n: torch.cat([t, torch.zeros(N, n - 4, dtype=torch.float64)], 1)
    x, v = wide(ones, n_in) * K["unit"], wide(ones, n_in) * K["unit"]
    g = ones * K["gs"] * sgn.new_tensor([1.0, -1.0, 1.0, 0.0])
    wrow = torch.tensor(K["w"], dtype=torch.float64)
    if probe == "W":                                   # masters that round when they are packed
        ws[0][:4, :4] = 0.0
        ws[0][:4, 0] = torch.tensor([top, below, -top, -below], dtype=torch.float64)
        x = x * K["small"] / K["unit"]
        v = v * K["small"] / K["unit"]
        if dtype == F16:   # and float32 masters at subnormal ties: 1.5 q -> 2 q (up, to even), 2.5 q -> 2 q (down), q = 2^-24, both signs;
            q = F16_QUANTUM   # input 1 is 2^10, so that H_0[:, 4 .. 5] = 2 q 2^10 shows them, and layer 1 hands them on
            ws[0][4:8, 1] = torch.tensor([1.5 * q, 2.5 * q, -1.5 * q, -2.5 * q], dtype=torch.float64)
            x[:, 1], v[:, 1] = x[:, 1] * 2.0 ** 16, v[:, 1] * 2.0 ** 16
            ws[1][2, 4] = ws[1][3, 5] = 1.0
    elif probe in ("x", "g", "v"):                     # float32 inputs that round on load
        assert f32_ends
        l = H if probe == "g" else 0
        ws[l][:4, :4] = 0.0
        ws[l][0, 0], ws[l][1, 0] = K["small"], -K["small"]
        x, v = x * K["mid"] / K["unit"], v * K["mid"] / K["unit"]
        if probe == "g":
            ws[l][0, 1] = ws[l][0, 2] = K["small"]     # (so that dZ below the output layer is not a column of zeros only)
            g = edge
        elif probe == "x":
            x = wide(edge, n_in)
        else:
            v = wide(edge, n_in)
    elif probe[0] in "HyTu":                           # forward and tangent: z_r[0] = +(a w0 + ..), z_r[1] = -(..)
        r = H if probe in ("y", "u") else int(probe[1:])
        ws[r][:4, :4] = 0.0
        ws[r][0, :3], ws[r][1, :3] = wrow, -wrow
        if probe[0] in "Hy":
            x = wide(vec, n_in)
        else:
            v = wide(vec, n_in)
    else:                                              # backward: dH_{j-1}[0] = +(..), dH_{j-1}[1] = -(..); neuron 2 keeps layer j alive
        j = 0 if probe == "dx" else int(probe[2:]) + 1
        ws[j][:4, :4] = 0.0
        ws[j][:3, 0], ws[j][:3, 1], ws[j][:3, 2] = wrow, -wrow, wrow
        g = vec
    c = custom_case(net, kind, dtype, (n_in, n_out, W, H), [w.float() for w in ws], x.to(end), g.to(end), v.to(end), f32_ends,
                    has_second_order(net))
    c.skip_layer, c.skip_mask = skip_layer, skip_mask
    c.bs = [torch.zeros(w.shape[0]) for w in ws] if bias else None
    for t, t64 in ((c.x, x), (c.g, g), (c.v, v)):
        assert end == F32 or torch.equal(t.double(), t64), "a half input of a boundary case must be exact"
    return c


def boundary_conditions(c, probe, a):
    """On the restatement: the probed rounding gives +inf and MAX (and -inf and -MAX where the sign survives: not behind a
    ReLU) out of values that are finite and above MAX before it."""
    p = a[{"W": "W0"}.get(probe, probe)]
    n = 1 if probe == "W" else 2   # the rows are there twice, a master once
    counts = (p.born_pos, p.to_max_pos, p.born_neg, p.to_max_neg)
    assert p.born_pos >= n and p.to_max_pos >= n, (probe, counts)
    if probe[0] != "H":
        assert p.born_neg >= n and p.to_max_neg >= n, (probe, counts)
    if probe == "W" and c.dtype == F16:   # the masters at subnormal ties, and what they feed
        assert p.tie_up == 2 and p.tie_down == 2 and p.sub == 4, (p.tie_up, p.tie_down, p.sub)
        h0 = a["H0"].post[BOUNDARY_ROWS]
        assert bool((h0[:, 4:6] == 2 * F16_QUANTUM * 2.0 ** 10).all()) and not bool(h0[:, 6:8].any())


# ---------------------------------------------------------------- poison: one non-finite element in row p

POISON_VALUES = (NAN, INF, -INF)


def poison_rows(net):
    """[(N, p, value)]: p = 0, 31, 32, N - 1 for N = 33, 129, 300 (the streamed kernels: 0, 127, 128 for N = 129), the three
    values dealt round so that every kind of row meets each of them."""
    if NETS[net][0] == "stream":
        return [(129, p, POISON_VALUES[i]) for i, p in enumerate((0, 127, 128))]
    return [(N, p, POISON_VALUES[(i + k) % 3]) for k, N in enumerate((33, 129, 300)) for i, p in enumerate((0, 31, 32, N - 1))]


def poisoned(t, p, value):
    out = t.clone()
    out[p, (p + 1) % t.shape[1]] = value
    return out


# ---------------------------------------------------------------- a dead neuron under an infinite gradient

def dead_neuron_case(dtype):
    """4 -> 64 -> 64 -> 2 without biases, 3 points, half ends.  Finite g and v; in row 0
        dZ_1[0] = +inf is BORN at its rounding (g[0, 0] W_2[0, 0] is finite in float32 and above MAX), at a live neuron;
        dH_0 = dZ_1 W_1 is +inf at neuron 0 (H_0 > 0), +inf at neuron 1 (H_0 = 0: dead) and NaN (inf * 0) at the dead neurons 3 ..;
        T_0[0] = +inf is born the same way, and W_1 T_0 is -inf at neuron 1 of layer 1, which is dead.
    A select gives 0 at the dead neurons, a multiplication by the mask NaN.  Rows 1 and 2 have g = v = 0."""
    big, g0 = {F16: (2.0, 60000.0), BF16: (7.0 * 2.0 ** 59, 73.0 * 2.0 ** 60)}[dtype]
    unit = {F16: 1.0, BF16: 2.0 ** -100}[dtype]
    w0, w1, w2 = torch.zeros(64, 4), torch.zeros(64, 64), torch.zeros(2, 64)
    w0[0, 0], w0[1, 0], w0[2, 1] = big, -big, big
    w1[0, :3] = 1.0
    w1[1, 0] = -1.0
    w1[2, 2] = 1.0
    w2[0, 0], w2[0, 1], w2[1, 2] = big, big, big
    x = torch.full((3, 4), unit).to(dtype)
    g = torch.zeros(3, 2)
    g[0, 0] = g0
    v = torch.zeros(3, 4)
    v[0, 0] = g0
    return custom_case("dead", "plain", dtype, (4, 2, 64, 2), [w0, w1, w2], x, g.to(dtype), v.to(dtype), False, True)


def dead_neuron_conditions(c, r, a):
    h0, h1 = r.f["hidden"]
    assert float(h0[0, 0]) > 0 and float(h0[0, 1]) == 0 and float(h1[0, 0]) > 0 and float(h1[0, 1]) == 0
    assert bool(torch.isfinite(c.g.double()).all()) and bool(torch.isfinite(c.v.double()).all())
    assert a["dZ1"].born_inf == 1 and float(a["dZ1"].post[0, 0]) == INF
    pre = product(r.b["dz"][1], R.rnd(c.ws[1].double(), c.dtype), c.dtype, "dH_0")
    assert float(pre[0, 0]) == INF and float(pre[0, 1]) == INF and bool(torch.isnan(pre[0, 3:]).all())
    assert r.b["dz"][0][0].tolist() == [INF, 0.0, INF] + [0.0] * 61
    assert a["T0"].born_inf == 1 and float(a["T0"].post[0, 0]) == INF
    pre = product(r.s["t"][1], R.rnd(c.ws[1].double(), c.dtype).t(), c.dtype, "tangent z_1")
    assert float(pre[0, 0]) == INF and float(pre[0, 1]) == -INF
    assert float(r.s["t"][2][0, 0]) == INF and float(r.s["t"][2][0, 1]) == 0.0
    n01 = c.ws[0].numel() + c.ws[1].numel()
    assert bool(torch.isfinite(r.dp[4:8]).all()), "dW_0[1, :]: the dead neuron's row of the first matrix"
    assert float(r.d2p[n01 + 1]) == 0.0, "d2W_2[0, 1] = g[0, 0] T_1[0, 1] sees T_1[0, 1] = 0"


# ---------------------------------------------------------------- the scaler: an overflow born inside the backward kernel

SCALER_SHAPE = (16, 4, 64, 1)
SCALER_POINTS = 64
SCALER_LOG2_SCALE = 14          # g * 2^14 <= 2 * 2^14 = 32768 is finite in fp16; dZ_0 = g W_1 * 2^14 is not


def scaler_case():
    """(ws, x, coef, scales, skips): the exact 16 -> 64 -> 4 fp16 network with float32 ends on 64 points, the loss
    sum(coef * y) (so dL/dy = coef, integers -2 .. 2), and what the restatement predicts for a scaler that starts at 2^14 and
    halves: ``scales[i]`` is the scale at step i, ``skips`` how many steps in a row have a non-finite dL/dparams before the first
    that is finite.  While steps are skipped the parameters do not move, so the data stay exact."""
    ws = R.exact_weights("dense", *SCALER_SHAPE)
    ws[1] = ws[1] * 4.0          # still integers: |dH_0| reaches 28, so three scales in a row overflow
    x, coef = R.exact_inputs(SCALER_POINTS, SCALER_SHAPE[0], SCALER_SHAPE[1], F32, F32)
    c = custom_case("scaler", "plain", F16, SCALER_SHAPE, ws, x, coef, x, True, False)
    R.backward(x, ws, R.forward(x, ws, F16, True, exact=True)["hidden"], coef, F16, exact=True)
    scales, skips = [], None
    for i in range(SCALER_LOG2_SCALE + 1):
        s = 2.0 ** (SCALER_LOG2_SCALE - i)
        g = coef * s
        assert bool(torch.isfinite(g.to(F16)).all()), "the scaled dL/dy itself must be finite in fp16"
        r = restate(c, g=g)
        a = audit(SimpleNamespace(**{**vars(c), "g": g}), r)
        scales.append(s)
        if bool(torch.isfinite(r.dp).all()):
            skips = i
            break
        assert a["dZ0"].born_inf > 0 and bool(torch.isfinite(r.b["dz"][1]).all()), "the overflow is born at dZ_0"
    return ws, x, coef, scales, skips


# ---------------------------------------------------------------- the scale sets

# (ex, eg, ev, [ew_l]) per network, found by search so that the restatement meets scale_conditions below.  The 'dense' family,
# except for the streamed network with a skip, where it leaves dZ_0 dead (FAMILY).
FAMILY = {"stream-256x3-bias-skip2": "perm"}
UNDERFLOW = {
    "plain-64x2": (-25, -24, -24, [-1, -1, -1]),
    "plain-128x1": (-25, -24, -24, [-2, -1]),
    "net-64x3-bias-skip2": (-25, -24, -24, [0, -1, 0, -1]),
    "stream-256x2": (-25, -23, -24, [-1, -1, -1]),
    "stream-256x3-bias-skip2": (-25, -24, -24, [0, 0, 0, -1]),
}
# Several sub-cases per network: an infinity in H_l floods the rows behind it with NaN, so each rounding point gets a sub-case
# in which the overflow is born THERE.  Forward sub-cases scale x and v, backward sub-cases g.
OVERFLOW = {
    F16: {   # the 'dense' family (FAMILY)
        "plain-64x2": [(11, 0, 11, [4, 0, 0]), (10, 0, 10, [0, 4, 0]), (9, 0, 9, [0, 0, 4]), (0, 9, 0, [0, 4, 0]), (0, 11, 0, [0, 0, 4])],
        "plain-128x1": [(8, 0, 8, [4, 0]), (8, 0, 8, [2, 0]), (0, 10, 0, [0, 4])],
        "net-64x3-bias-skip2": [(8, 0, 8, [4, 0, 0, 0]), (8, 0, 8, [0, 0, 3, 0]), (0, 9, 0, [0, 4, 0, 0]), (0, 11, 0, [0, 0, 4, 0]),
                                (0, 11, 0, [0, 0, 0, 4])],
        "stream-256x2": [(9, 0, 9, [4, 0, 0]), (8, 0, 8, [2, 0, 0]), (0, 8, 0, [4, 0, 0]), (0, 10, 0, [0, 4, 0]), (0, 11, 0, [0, 0, 4])],
        "stream-256x3-bias-skip2": [(8, 0, 8, [6, 0, 0, 0]), (8, 0, 8, [4, 0, 0, 0]), (0, 8, 0, [6, 0, 0, 0]), (0, 8, 0, [0, 6, 0, 0]),
                                    (0, 8, 0, [0, 0, 8, 0]), (0, 8, 0, [0, 0, 0, 8])],
    },
    BF16: {  # the 'perm' family (see the module's docstring); g, or x and v, at 2^-60 keep every weight-gradient sum finite
        "plain-64x2": [(124, -60, 124, [4, 0, 0]), (123, -60, 123, [0, 4, 0]), (123, -60, 123, [0, 0, 4]), (-60, 122, -60, [4, 0, 0]),
                       (-60, 122, -60, [0, 4, 0]), (-60, 123, -60, [0, 0, 4])],
        "plain-128x1": [(122, -60, 122, [4, 0]), (121, -60, 121, [4, 0]), (-60, 126, -60, [1, 0])],
        "net-64x3-bias-skip2": [(121, -60, 121, [8, 0, 0, 0]), (120, -60, 120, [0, 8, 0, 0]), (120, -60, 120, [0, 0, 8, 0]),
                                (120, -60, 120, [0, 0, 0, 8]), (-60, 122, -60, [1, 4, 0, 0]), (-60, 121, -60, [0, 0, 6, 0]),
                                (-60, 121, -60, [0, 0, 0, 6])],
        "stream-256x2": [(122, -60, 122, [4, 0, 0]), (121, -60, 121, [4, 0, 0]), (121, -60, 121, [0, 0, 4]), (-60, 126, -60, [1, 0, 0]),
                         (-60, 124, -60, [0, 0, 4])],
        "stream-256x3-bias-skip2": [(121, -60, 121, [8, 0, 0, 0]), (120, -60, 120, [0, 8, 0, 0]), (120, -60, 120, [0, 0, 8, 0]),
                                    (120, -60, 120, [0, 0, 0, 8]), (-60, 120, -60, [8, 0, 0, 0]), (-60, 120, -60, [0, 6, 0, 0]),
                                    (-60, 120, -60, [0, 0, 8, 0]), (-60, 120, -60, [0, 0, 0, 8])],
    },
}
BF16_BIAS_EXPONENT = -8   # scaled(): eb of the bf16 overflow cases


SUBNORMAL_WEIGHT_EXPONENT = -16   # the masters are integers 1 .. 2 (and the x columns' +-1): 2^-16 and 2^-15 are fp16 subnormals


def scaled_cases(net, dtype, which, f32_ends):
    """The cases of a scale set.  "underflow" (fp16): the case of UNDERFLOW, in which what the passes STORE is subnormal, and
    behind it one sub-case per layer l in which W_l * 2^-16 is subnormal and nothing else is scaled: the packed weights are
    the MFMA's A operand in the forward, data-gradient and tangent passes, so a pack kernel or a layer kernel that flushed
    them would zero H_l, dZ_{l-1} and T_l.  "overflow": one case per sub-case of OVERFLOW."""
    if which == "underflow":
        assert dtype == F16
        base = base_case(net, dtype, FAMILY.get(net, "dense"), f32_ends)
        L = len(base.ws)
        return [scaled(base, *UNDERFLOW[net])] + [scaled(base, 0, 0, 0, [SUBNORMAL_WEIGHT_EXPONENT * (k == l) for k in range(L)])
                                                  for l in range(L)]
    base = base_case(net, dtype, FAMILY.get(net, "dense") if dtype == F16 else "perm", f32_ends)
    return [scaled(base, *s, eb=BF16_BIAS_EXPONENT if dtype == BF16 else 0) for s in OVERFLOW[dtype][net]]


def scale_conditions(c, which, audits, restated):
    """underflow: at least 32 non-zero subnormal results at every stored rounding point, at least one subnormal tie that rounds
    down to even and one that rounds up (the first case); in the sub-case of layer l EVERY non-zero packed weight of W_l
    is subnormal (at least 16: a 3-row output matrix of the 'dense' family keeps 24 entries), and at least 32 non-zero finite results of each product that has them as its A operand (H_l or y, dZ_{l-1} or dL/dx,
    T_l or u).  overflow: at least 8 infinities born at every stored rounding point (finite in float32 before the rounding, or
    the float32 rounding of a single product), in one of the sub-cases."""
    for p in stored_points(c):
        if which == "underflow":
            assert audits[0][p].sub >= 32, (p, audits[0][p].sub)
        else:
            assert max(a[p].born_inf for a in audits) >= 8, (p, [a[p].born_inf for a in audits])
    if which == "underflow":
        assert sum(s.tie_down for s in audits[0].values()) >= 1 and sum(s.tie_up for s in audits[0].values()) >= 1
        H = c.shape[3]
        assert len(audits) == H + 2
        for l, (a, r) in enumerate(zip(audits[1:], restated[1:])):
            assert a[f"W{l}"].sub >= 16 and a[f"W{l}"].sub == int((a[f"W{l}"].post != 0).sum()), (l, a[f"W{l}"].sub)
            through = [r.f["hidden"][l] if l < H else r.f["y"], r.b["dz"][l - 1] if l > 0 else r.b["dx"]]
            if r.s is not None:
                through.append(r.s["t"][l + 1] if l < H else r.s["u"])
            for t in through:
                assert bool(torch.isfinite(t).all()) and int((t != 0).sum()) >= 32, (l, int((t != 0).sum()))
