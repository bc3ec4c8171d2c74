"""Float64 restatements of the rendering passes at the edges of opacity's range, in plain torch (no nerfacc_amd import).

Built on ``seg_reference`` (``Rays``, ``bound``, the scale helpers).  What it adds:

* the backward of the density and alpha chains and of the plain product scans in CLOSED FORM.  ``seg_reference``'s
  gradients come from autograd over ``cumprod``; at ``alpha == 1`` that is not what the kernels (and the reference
  implementation they follow) compute: they divide the suffix sum by ``max(1 - alpha, 1e-10)``.  The two agree wherever
  ``alpha < 1`` and differ at ``alpha == 1`` (tests/test_render_edges_cpu.py keeps both facts on record);
* ``rendering``'s depth normalisation ``depth / opacity.clamp_min(eps)`` and its gradient;
* generators of edge cases -- saturating samples, vanishing opacity, transmittance sums around the early-stop threshold --
  on the ray lengths at which the packed engine changes behaviour.

Every function is dtype-generic: run on float32 tensors it is the float32 torch composition of the same formulas, which
the CPU tests hold against the float64 run to show that the bounds are not what a GPU failure could be blamed on.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import seg_reference as SR

TINY = 2.0 ** -126 * SR.K_ROUND    # results below float32's normal range have no relative precision
EPS_DEPTH = 2.0 ** -23             # torch.finfo(float32).eps: rendering's clamp of the opacity under the depth
CLAMP_1MA = 1e-10                  # the alpha / product backward divides by max(1 - alpha, 1e-10)
DELTA = 2.0 ** -6                  # the generators' sample length: t_ends = t_starts + DELTA exactly (t_starts on a 2^-10 grid)
X_SAT32 = 1.0e4                    # for float32 every sigma * delta above ~104 is the same sample: alpha == 1, T == 0 behind it


# ----------------------------------------------------------------------------- ray lengths
# Rays in a fixed order, so that the named positions below exist: rays of 1-3 samples that share a lane, a ray that ends
# exactly at a 256-element step, one that is the last of a 1024-element tile, one that is the first of the next tile and sits
# next to a run of empty rays, and the 1025-sample ray.
_BLOCKS = [("lane", [1, 2, 3, 1, 2, 3, 2, 1, 1]), ("short", [0, 1, 2, 3, 4, 5]), ("wave", [63, 64, 65]), ("step_end", [33]),
           ("steps", [255, 256, 257]), ("tile_first", [5]), ("empty", [0] * 70), ("long", [1025]), ("tail", [5, 4, 3, 2, 1, 0])]
TILE_ELEMS, STEP_ELEMS = 1024, 256


def edge_counts() -> torch.Tensor:
    c = np.concatenate([np.asarray(b, np.int64) for _, b in _BLOCKS])
    assert c.sum() % 4 != 0
    return torch.from_numpy(c)


def edge_rays() -> dict:
    """Ray numbers of the named positions in ``edge_counts()``."""
    first, r = {}, 0
    for name, b in _BLOCKS:
        first[name] = r
        r += len(b)
    return {"lane": first["lane"] + 4,            # 2 samples, between rays of 1 and 3 samples: three rays in one lane
            "step_end": first["step_end"],        # ends at element 256
            "tile_last": first["steps"] + 2,      # the 257-sample ray: ends at element 1024
            "tile_first": first["tile_first"],    # starts at element 1024; 70 empty rays follow
            "long": first["long"]}


# ----------------------------------------------------------------------------- closed-form backward
def _suffix(rays: SR.Rays, q: torch.Tensor, inclusive: bool = False) -> torch.Tensor:
    return rays.unpad(SR.rev_sum_rows(rays.pad(q), inclusive))


def _z(like, g):
    return torch.zeros_like(like) if g is None else g


def density_forward(rays: SR.Rays, ts, te, sig, prefix=None):
    """(weights, trans, alphas, x = sigma * delta) in the dtype of the inputs."""
    x = sig * (te - ts)
    S = rays.unpad(SR.excl_sum_rows(rays.pad(x)))
    T = torch.exp(-S)
    if prefix is not None:
        T = T * prefix
    a = 1.0 - torch.exp(-x)
    return T * a, T, a, x


def density_backward(rays: SR.Rays, ts, te, T, a, gw=None, gt=None, ga=None):
    """dL/dx and dL/dsigma of L = sum gw w + gt T + ga alpha, x = sigma * delta:
        dL/dx_i = (gw_i T_i + ga_i)(1 - a_i) - sum_{j > i} (gw_j a_j + gt_j) T_j,   dL/dsigma = delta * dL/dx."""
    gw, gt, ga = _z(T, gw), _z(T, gt), _z(T, ga)
    gx = (gw * T + ga) * (1.0 - a) - _suffix(rays, (gw * a + gt) * T)
    return gx, (te - ts) * gx


def alpha_forward(rays: SR.Rays, al, prefix=None):
    T = rays.unpad(SR.excl_prod_rows(rays.pad(1.0 - al, 1.0)))
    if prefix is not None:
        T = T * prefix
    return T * al, T


def alpha_backward(rays: SR.Rays, al, T, gw=None, gt=None):
    """dL/dalpha_i = gw_i T_i - [sum_{j > i} (gw_j a_j + gt_j) T_j] / max(1 - a_i, 1e-10)."""
    gw, gt = _z(T, gw), _z(T, gt)
    return gw * T - _suffix(rays, (gw * al + gt) * T) / (1.0 - al).clamp_min(CLAMP_1MA)


def prod_backward(rays: SR.Rays, x, y, g, kind: str):
    """Gradient of inclusive_prod / exclusive_prod: the suffix sum of g * y (from the element itself / from the next one)
    over max(x, 1e-10)."""
    return _suffix(rays, g * y, kind.startswith("inclusive")) / x.clamp_min(CLAMP_1MA)


def alpha_scales(rays: SR.Rays, al, T, gw=None, gt=None):
    """``seg_reference.alpha_scales`` with the backward's own clamp: at a_i == 1 every T_j behind is exactly 0, so the
    chain's share vanishes and the scale is |gw_i| T_i (seg_reference divides by zero there)."""
    T, a = T.abs(), al.abs()
    gw, gt = _z(T, gw).abs(), _z(T, gt).abs()
    chain = _suffix(rays, (gw * a + gt) * T) / (1.0 - a).clamp_min(CLAMP_1MA)
    return T * a, T, gw * T + chain


def prod_scales(rays: SR.Rays, x, y, g, kind: str):
    """Forward: every factor and product rounds once (relative).  Backward: the g_j y_j and their sum round, over the
    clamped x."""
    return y.abs(), 2.0 * _suffix(rays, (g * y).abs(), kind.startswith("inclusive")) / x.abs().clamp_min(CLAMP_1MA)


def density_scales(rays: SR.Rays, ts, te, sig, T, a, gw=None, gt=None, ga=None):
    """``seg_reference.density_scales`` with +inf densities taken at X_SAT32 / delta: in float32 both are the same sample
    (alpha == 1 exactly, T == 0 exactly behind), and inf would make the scales 0 * inf."""
    big = X_SAT32 / (te - ts).abs().clamp_min(1e-30)
    s = torch.where(torch.isinf(sig), big, sig)
    return SR.density_scales(rays, ts, te, s, T, a, gw, gt, ga)


# ----------------------------------------------------------------------------- depth normalisation
def normalise_depth(opac, depth_raw, eps: float = EPS_DEPTH):
    return depth_raw / opac.clamp_min(eps)


def normalise_depth_backward(opac, depth, g_o, g_d, eps: float = EPS_DEPTH):
    """(G_opacity, G_depth_raw, share): what reaches the accumulated opacity and un-normalised depth from the gradients
    (g_o, g_d) of opacity and normalised depth ``depth``.  ``share`` is the part of G_opacity that came through the
    normalisation: exactly 0 while opacity < eps (the clamp passes no gradient there)."""
    oc = opac.clamp_min(eps)
    live = (opac >= eps).to(opac.dtype)
    share = -live * g_d * depth / oc
    return g_o + share, g_d / oc, share


def rendering_reference(rays: SR.Rays, ts, te, field, rgb, dens: bool, g_c, g_o, g_d, g_ex=(None, None, None),
                        opac_own=None, depth_own=None) -> dict:
    """``rendering`` forward and closed-form backward in the dtype of the inputs, with the tolerances of a float32 pass.

    field: sigmas (dens) or alphas.  (g_c, g_o, g_d): gradients of colours (R, 3), opacity (R, 1), normalised depth (R, 1);
    g_ex: gradients arriving at the per-sample weights / trans / alphas.  The depth normalisation amplifies by up to 2^23,
    so its backward is formed from the outputs the pass under test produced itself (opac_own, depth_own; default: this
    run's), as torch forms it from the product's outputs.  Returns {name: (value, tolerance)}."""
    ri = rays.ray_ids
    if dens:
        w, T, a, _ = density_forward(rays, ts, te, field)
    else:
        w, T = alpha_forward(rays, field)
        a = field
    col, op, draw = SR.render_accumulate(rays, w, rgb, ts, te)
    depth = normalise_depth(op, draw)
    opac_own = op if opac_own is None else opac_own.to(op.dtype)
    depth_own = depth if depth_own is None else depth_own.to(op.dtype)
    G_o, G_d, share = normalise_depth_backward(opac_own, depth_own, g_o, g_d)
    mid = (ts + te) / 2.0
    gw_ex, gt_ex, ga_ex = g_ex
    gw = (g_c[ri] * rgb).sum(-1) + G_o[ri, 0] + G_d[ri, 0] * mid + _z(w, gw_ex)
    if dens:
        _, g_field = density_backward(rays, ts, te, T, a, gw, gt_ex, ga_ex)
    else:
        g_field = alpha_backward(rays, a, T, gw, gt_ex)
    g_rgb = g_c[ri] * w[:, None]
    # scales (as tests/test_kernel_variants_gpu.py: test_rendering_scalar_form)
    gw_abs = (g_c.abs()[ri] * rgb.abs()).sum(-1) + (g_o.abs() + share.abs())[ri, 0] + G_d.abs()[ri, 0] * mid.abs() + _z(w, gw_ex).abs()
    if dens:
        s_w, s_t, s_a, s_gx = density_scales(rays, ts, te, field, T, a, gw_abs, gt_ex, ga_ex)
        s_f = s_gx * (te - ts).abs()
    else:
        s_w, s_t, s_f = alpha_scales(rays, a, T, gw_abs, gt_ex)
        s_a = torch.zeros_like(s_t)
    sw1 = s_w + w.abs()
    s_col = SR.accumulate(rays, sw1, rgb.abs())
    s_op = SR.accumulate(rays, sw1)
    s_dr = SR.accumulate(rays, sw1, mid.abs()[:, None])
    s_dep = (s_dr + depth.abs() * s_op) / op.clamp_min(EPS_DEPTH)
    b = lambda s, **kw: SR.bound(rays, s, **kw)
    return {"colors": (col, b(s_col, per_ray=True)), "opacities": (op, b(s_op, per_ray=True)),
            "depths": (depth, b(s_dep, per_ray=True, extra=4)), "weights": (w, b(s_w)), "trans": (T, b(s_t)),
            "alphas": (a, b(s_a)), "g_field": (g_field, b(s_f)), "g_rgbs": (g_rgb, b(g_c.abs()[ri] * sw1[:, None])),
            "share": (share, None)}


# ----------------------------------------------------------------------------- generators
BACKGROUND = (0.0, 1e-40, 1e-9, 2.0 ** -25, 1e-3, 0.5, 1.0)     # sigma * delta of the samples that do not saturate
SATURATING = (88.0, 104.0, 1.0e4, math.inf)
N_BG = len(BACKGROUND)


def _grid_times(n: int, g: torch.Generator):
    ts = torch.randint(0, 4096, (n,), generator=g).float() / 1024.0
    te = ts + DELTA
    assert bool(((te - ts) == DELTA).all())
    return ts, te


def saturating(counts: torch.Tensor, where: str, seed: int = 0, with_inf: bool = True) -> dict:
    """Packed float32 (t_starts, t_ends, sigmas) with one saturating sample per ray at its first / middle / last position
    and background samples drawn from BACKGROUND.  ``cls``: per sample, the index into BACKGROUND or N_BG + the index into
    SATURATING; ``sat``: the packed index of each ray's saturating sample (-1 for an empty ray)."""
    assert where in ("first", "middle", "last")
    rays = SR.Rays(counts)
    g = torch.Generator().manual_seed(seed)
    n = rays.n
    ts, te = _grid_times(n, g)
    cls = torch.randint(0, N_BG, (n,), generator=g)
    x = torch.tensor(BACKGROUND, dtype=torch.float64)[cls]
    n_sat = len(SATURATING) if with_inf else len(SATURATING) - 1
    live = rays.counts > 0
    off = {"first": torch.zeros_like(rays.counts), "middle": rays.counts // 2, "last": rays.counts - 1}[where]
    sat = torch.where(live, rays.starts + off, torch.full_like(rays.starts, -1))
    kind = torch.arange(int(live.sum())) % n_sat
    x[sat[live]] = torch.tensor(SATURATING, dtype=torch.float64)[kind]
    cls[sat[live]] = N_BG + kind
    sig = (x / DELTA).float()
    return {"rays": rays, "t_starts": ts, "t_ends": te, "sigmas": sig, "cls": cls, "sat": sat, "where": where}


def ordinary(counts: torch.Tensor, seed: int = 0, sig_max: float = 20.0) -> dict:
    """A finite mid-range case on the same grid of times: the base of the containment tests."""
    rays = SR.Rays(counts)
    g = torch.Generator().manual_seed(seed)
    ts, te = _grid_times(rays.n, g)
    sig = torch.rand(rays.n, generator=g) * sig_max
    rgbs = torch.rand(rays.n, 3, generator=g)
    alphas = 1.0 - torch.exp(-sig * (te - ts))
    return {"rays": rays, "t_starts": ts, "t_ends": te, "sigmas": sig, "alphas": alphas, "rgbs": rgbs}


VANISHING = ("zeros", "neg_zeros", "subnormal", "total_0", "total_subnormal", "total_below_eps", "total_eps", "total_above_eps")
_SUB = 1e-42
OPACITY_TARGETS = {"total_0": 0.0, "total_subnormal": 1e-40,
                   "total_below_eps": float(np.nextafter(np.float32(EPS_DEPTH), np.float32(0))),
                   "total_eps": EPS_DEPTH, "total_above_eps": float(np.nextafter(np.float32(EPS_DEPTH), np.float32(1)))}


def vanishing(counts: torch.Tensor, seed: int = 0) -> dict:
    """Rays that are all zeros, all -0.0, all subnormal, and rays whose opacity lands at 0, in the subnormal range, at
    nextafter(2^-23, 0), 2^-23 and nextafter(2^-23, 1).  ``alphas`` hits the five targets exactly (one live sample in the
    middle of the ray, exact zeros around it; for the target 0 every alpha is 0).  ``sigmas`` = alphas / delta is the
    density form: 1 - exp(-x) is x to first order, so those rays land next to the targets -- except "total_0", whose
    sigma * delta is 2^-30 everywhere: non-zero densities whose float32 alphas are all exactly 0.  ``kind``: per ray the
    index into VANISHING (-1: empty), ``cls`` the same per sample."""
    rays = SR.Rays(counts)
    g = torch.Generator().manual_seed(seed)
    n = rays.n
    ts, te = _grid_times(n, g)
    live = rays.counts > 0
    kind = torch.full_like(rays.counts, -1)
    kind[live] = torch.arange(int(live.sum())) % len(VANISHING)
    cls = kind[rays.ray_ids]
    al = torch.zeros(n, dtype=torch.float32)
    sig = torch.zeros(n, dtype=torch.float32)
    al[cls == VANISHING.index("neg_zeros")] = -0.0
    sig[cls == VANISHING.index("neg_zeros")] = -0.0
    al[cls == VANISHING.index("subnormal")] = _SUB
    sig[cls == VANISHING.index("subnormal")] = _SUB
    sig[cls == VANISHING.index("total_0")] = 2.0 ** -30 / DELTA
    mid = rays.starts + rays.counts // 2
    for name, target in OPACITY_TARGETS.items():
        if name == "total_0":
            continue
        rows = mid[kind == VANISHING.index(name)]
        al[rows] = target
        sig[rows] = target / DELTA
    rgbs = torch.rand(n, 3, generator=g)
    return {"rays": rays, "t_starts": ts, "t_ends": te, "sigmas": sig, "alphas": al, "rgbs": rgbs, "kind": kind, "cls": cls}


# ---- the early-stop threshold
EARLY_STOP_EPS = (1e-2, 1e-4, 1e-6, 1e-10, 1e-37, 1e-40, 1e-44, 1.0 - 2.0 ** -24, 1.0, 1.5)
FLT_MIN = 2.0 ** -126
AMBIGUOUS_REL = 8 * 2.0 ** -24
GRID_BELOW_1 = 2.0 ** -26
N_BEYOND = 50


def eps32(eps: float) -> float:
    """The float32 the kernel receives."""
    return float(np.float32(eps))


def band(eps: float):
    """The band [s_lo, s_hi] of sums S inside which the visibility pass evaluates exp(-S) for a normal eps: +-2e-5 relative
    around -ln(eps), as float32 (a restatement of the host code's arithmetic).  For a subnormal eps the pass evaluates
    exp(-S) everywhere; the sweeps still step through this nominal band."""
    L = -math.log(eps32(eps))
    w = 2e-5 * max(L, 1.0)
    return float(np.float32(L - w)), float(np.float32(L + w))


def threshold_sweeps(eps: float) -> torch.Tensor:
    """Float32 sums S >= 0, ascending, that step through the whole band around -ln(eps) and N_BEYOND values beyond each end:
    consecutive float32 values, or a grid of 2^-26 where -ln(eps) < 1."""
    L = -math.log(eps32(eps))
    s_lo, s_hi = band(eps)
    if L < 1.0:
        k_lo = max(0, int(math.floor(s_lo / GRID_BELOW_1)) - N_BEYOND)
        k_hi = max(int(math.ceil(s_hi / GRID_BELOW_1)), 0) + N_BEYOND
        s = np.arange(k_lo, k_hi + 1, dtype=np.float64) * GRID_BELOW_1
        s32 = s.astype(np.float32)
        assert np.array_equal(s32.astype(np.float64), s)
        return torch.from_numpy(s32)
    lo, hi = np.float32(s_lo), np.float32(s_hi)
    for _ in range(N_BEYOND):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    b_lo, b_hi = int(lo.view(np.int32)), int(hi.view(np.int32))     # positive floats: consecutive values, consecutive bits
    return torch.from_numpy(np.arange(b_lo, b_hi + 1, dtype=np.int32).view(np.float32).copy())


def sweep_expectation(S: torch.Tensor, eps: float):
    """(visible, ambiguous) per probe: float64 exp(-S) >= eps, and whether exp(-S) is within 8 * 2^-24 relative of eps (either
    answer is accepted there).  For a subnormal eps a relative ulp is not defined and this expectation is not used."""
    e = eps32(eps)
    T = torch.exp(-S.double())
    return T >= e, (T / e - 1.0).abs() <= AMBIGUOUS_REL


def ambiguous_cap(eps: float) -> int:
    """At most 8 ambiguous probes per sweep.  Where -ln(eps) < 1 the sweep is a grid of 2^-26 and the ambiguous window, 2 * 8 *
    2^-24 wide in S, necessarily holds 64 grid intervals: there the cap is the number of grid points the window can hold."""
    L = -math.log(eps32(eps))
    return 8 if L >= 1.0 else int(2 * AMBIGUOUS_REL / GRID_BELOW_1) + 1


def probe_rays(S: torch.Tensor, lead: int = 0) -> dict:
    """One ray per value of S: ``lead`` zero-density samples, one sample with t_starts = 0, t_ends = 1, sigma = S (so that the
    sum is S exactly), and the probed sample behind it.  ``probe``: packed index of each ray's probed sample."""
    R, m = int(S.numel()), lead + 2
    sig = torch.zeros(R, m, dtype=torch.float32)
    sig[:, lead] = S
    ts = torch.zeros(R * m, dtype=torch.float32)
    te = torch.ones(R * m, dtype=torch.float32)
    counts = torch.full((R,), m, dtype=torch.int64)
    return {"counts": counts, "t_starts": ts, "t_ends": te, "sigmas": sig.reshape(-1),
            "probe": torch.arange(R, dtype=torch.int64) * m + lead + 1}
