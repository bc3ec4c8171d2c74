"""Float64 restatements of the packed (segmented) ops, in plain torch, for the kernel-variant tests.

Nothing from nerfacc_amd is used here: rays are laid out as a padded ``(R, S_max)`` table with torch indexing, the scans
run along ``dim=1`` with ``cumsum`` / ``cumprod``, and every reference gradient comes from torch autograd over these
functions.  ``tests/test_seg_reference_cpu.py`` checks them against a per-ray Python loop.

Besides the values, the helpers return per-element error scales for float32 kernels: a float32 result that is a sum of
``m`` rounded terms is within ``(m + K) * 2^-23 * sum|terms|`` of the exact value (2^-23 = two units of roundoff, so the
bound also holds for any summation order), and ``exp(-S)`` inherits ``|error of S|`` as a relative error.  ``bound``
turns a scale into that tolerance with ``m`` = the ray's sample count.
"""
from __future__ import annotations

import torch

EPS32 = 2.0 ** -23
K_ROUND = 8          # roundings outside the sums (exp, products, the difference t_end - t_start, ...)


# ----------------------------------------------------------------------------- layout
class Rays:
    """Padded view of packed samples: ``counts`` (R,) samples per ray, rays stored one after the other."""

    def __init__(self, counts: torch.Tensor):
        self.counts = counts.to(torch.int64)
        self.R = int(self.counts.numel())
        self.n = int(self.counts.sum()) if self.R else 0
        self.S = int(self.counts.max()) if self.R else 0
        self.starts = torch.cumsum(self.counts, 0) - self.counts
        k = torch.arange(self.S, device=self.counts.device)
        self.mask = k[None, :] < self.counts[:, None]                      # (R, S)
        self.index = torch.where(self.mask, self.starts[:, None] + k[None, :], torch.zeros_like(self.mask, dtype=torch.int64))
        self.ray_ids = torch.repeat_interleave(torch.arange(self.R, device=self.counts.device), self.counts)
        self.elem_counts = self.counts[self.ray_ids]                       # (n,) the sample count of each sample's ray

    def pad(self, x: torch.Tensor, fill: float = 0.0) -> torch.Tensor:
        """(n, ...) -> (R, S, ...), ``fill`` outside the rays."""
        if self.n == 0:
            return x.new_full((self.R, self.S) + tuple(x.shape[1:]), fill)
        g = x[self.index]
        m = self.mask.view(self.R, self.S, *([1] * (x.dim() - 1)))
        return torch.where(m, g, torch.full_like(g, fill))

    def unpad(self, xp: torch.Tensor) -> torch.Tensor:
        """(R, S, ...) -> (n, ...) in packed order."""
        return xp[self.mask]

    def packed_info(self) -> torch.Tensor:
        return torch.stack([self.starts, self.counts], -1)


def bound(rays: Rays, scale: torch.Tensor, per_ray: bool = False, extra: int = 0) -> torch.Tensor:
    """Tolerance ``(m + K + extra) * 2^-23 * scale``; ``m`` the sample count of the element's ray (or of the ray itself)."""
    m = rays.counts if per_ray else rays.elem_counts
    m = m.to(scale.dtype)
    if scale.dim() > m.dim():
        m = m.view(-1, *([1] * (scale.dim() - 1)))
    return (m + K_ROUND + extra) * EPS32 * scale


# ----------------------------------------------------------------------------- scans
def excl_sum_rows(xp: torch.Tensor) -> torch.Tensor:
    return torch.cat([torch.zeros_like(xp[:, :1]), torch.cumsum(xp[:, :-1], 1)], 1)


def excl_prod_rows(xp: torch.Tensor) -> torch.Tensor:
    return torch.cat([torch.ones_like(xp[:, :1]), torch.cumprod(xp[:, :-1], 1)], 1)


def rev_sum_rows(xp: torch.Tensor, inclusive: bool) -> torch.Tensor:
    """sum over j >= i (inclusive) or j > i along each row."""
    r = torch.flip(torch.cumsum(torch.flip(xp, [1]), 1), [1])
    return r if inclusive else torch.cat([r[:, 1:], torch.zeros_like(r[:, :1])], 1)


def scan(rays: Rays, x: torch.Tensor, kind: str) -> torch.Tensor:
    """inclusive_sum / exclusive_sum / inclusive_prod / exclusive_prod of packed x."""
    if kind.endswith("sum"):
        xp = rays.pad(x, 0.0)
        y = torch.cumsum(xp, 1) if kind.startswith("inclusive") else excl_sum_rows(xp)
    else:
        xp = rays.pad(x, 1.0)
        y = torch.cumprod(xp, 1) if kind.startswith("inclusive") else excl_prod_rows(xp)
    return rays.unpad(y)


def scan_scales(rays: Rays, x: torch.Tensor, y: torch.Tensor, g: torch.Tensor, kind: str):
    """Scales of a scan's output and of its input gradient under the incoming gradient g (all float64)."""
    incl = kind.startswith("inclusive")
    if kind.endswith("sum"):
        fwd = scan(rays, x.abs(), kind)
        bwd = rays.unpad(rev_sum_rows(rays.pad(g.abs()), incl))
    else:   # relative: every factor and every product rounds once; the gradient is a suffix sum of g * y over x
        fwd = y.abs()
        bwd = rays.unpad(rev_sum_rows(rays.pad((g * y).abs()), incl)) / x.abs()
    return fwd, bwd


# ----------------------------------------------------------------------------- transmittance, alphas, weights
def from_density(rays: Rays, ts, te, sig, prefix=None):
    """(weights, trans, alphas) of ``render_weight_from_density``."""
    sdt = sig * (te - ts)
    S = rays.unpad(excl_sum_rows(rays.pad(sdt)))
    trans = torch.exp(-S)
    if prefix is not None:
        trans = trans * prefix
    alphas = 1.0 - torch.exp(-sdt)
    return trans * alphas, trans, alphas


def from_alpha(rays: Rays, alphas, prefix=None):
    """(weights, trans) of ``render_weight_from_alpha``."""
    trans = rays.unpad(excl_prod_rows(rays.pad(1.0 - alphas, 1.0)))
    if prefix is not None:
        trans = trans * prefix
    return trans * alphas, trans


def density_scales(rays: Rays, ts, te, sig, trans, alphas, gw=None, gt=None, ga=None):
    """Scales of (weights, trans, alphas) and of dL/d(sigma * delta) with L = sum gw w + gt T + ga a.

    float32 kernels form S = exclusive sum of x = sigma * delta (error <= (m + K) 2^-23 S), T = exp(-S) (so T picks up that
    error relatively), alpha = 1 - exp(-x) and w = T alpha.  The gradient is
        dL/dx_i = (gw_i T_i + ga_i)(1 - a_i) - sum_{j > i} (gw_j a_j + gt_j) T_j,
    and every T in it carries the relative error of its S.
    """
    x = (sig * (te - ts)).abs()
    S = rays.unpad(excl_sum_rows(rays.pad(x)))
    T, a = trans.abs(), alphas.abs()
    rel = 1.0 + S + x
    s_t = T * rel
    s_a = (1.0 - a) * (1.0 + x) + a
    s_w = a * s_t + T * s_a
    z = torch.zeros_like(T)
    gw = z if gw is None else gw.abs()
    gt = z if gt is None else gt.abs()
    ga = z if ga is None else ga.abs()
    direct = (gw * T + ga) * ((1.0 - a) * rel + s_a)
    chain = rays.unpad(rev_sum_rows(rays.pad((gw * a + gt) * T * (1.0 + rel) + gw * T * s_a), False))
    return s_w, s_t, s_a, direct + chain


def alpha_scales(rays: Rays, alphas, trans, gw=None, gt=None):
    """Scales of (weights, trans) and of dL/dalpha for ``render_weight_from_alpha``: every T is a product of rounded
    factors (relative error), dL/da_i = gw_i T_i - sum_{j > i} (gw_j a_j + gt_j) T_j / (1 - a_i)."""
    T, a = trans.abs(), alphas.abs()
    z = torch.zeros_like(T)
    gw = z if gw is None else gw.abs()
    gt = z if gt is None else gt.abs()
    chain = rays.unpad(rev_sum_rows(rays.pad((gw * a + gt) * T), False)) / (1.0 - a)
    return T * a, T, gw * T + chain


# ----------------------------------------------------------------------------- accumulations
def accumulate(rays: Rays, weights, values=None):
    """``accumulate_along_rays``: out[r] = sum_{i in r} w_i v_i (float64 index_add_)."""
    src = weights[:, None] if values is None else weights[:, None] * values
    out = torch.zeros((rays.R, src.shape[1]), dtype=src.dtype, device=src.device)
    return out.index_add(0, rays.ray_ids, src)


def render_accumulate(rays: Rays, weights, rgbs, ts, te):
    """The three accumulations of ``rendering`` before the depth is normalised: colours, opacity, depth * opacity."""
    return (accumulate(rays, weights, rgbs), accumulate(rays, weights),
            accumulate(rays, weights, ((ts + te) / 2.0)[:, None]))


def finish_rendering(colors, opac, depth_raw, eps: float = 2.0 ** -23):
    """``rendering``'s depth normalisation (``depth / opacity.clamp_min(eps)``), float32's eps as the product uses."""
    return colors, opac, depth_raw / opac.clamp_min(eps)


def render_step(rays: Rays, ts, te, sig, rgbs, opac_in, alpha_thre: float):
    """One iteration of the test-mode loop (``nfa_render_step_accumulate``): samples of a ray start behind the opacity
    it already has, T = (1 - opacity) exp(-S); samples below the alpha threshold contribute nothing (they still count in
    S).  Returns the increments of (colours, opacity, depth)."""
    _, trans, alphas = from_density(rays, ts, te, sig, prefix=(1.0 - opac_in[rays.ray_ids]))
    keep = alphas >= alpha_thre if alpha_thre > 0 else torch.ones_like(alphas, dtype=torch.bool)
    w = torch.where(keep, trans * alphas, torch.zeros_like(alphas))
    return accumulate(rays, w, rgbs), accumulate(rays, w), accumulate(rays, w, ((ts + te) / 2.0)[:, None]), keep


def cdf_rows(ts2, te2, sig2):
    """PropNetEstimator's CDF rows ``1 - cat([T, 0], -1)`` of batched (R, S) rows."""
    sdt = sig2 * (te2 - ts2)
    T = torch.exp(-excl_sum_rows(sdt))
    return 1.0 - torch.cat([T, torch.zeros_like(T[:, :1])], -1)
