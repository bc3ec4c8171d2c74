"""numpy restatement of the photometric-loss contract (csrc/photo.hip's header): float32 terms, every operation rounded on
its own, float64 sums rounded to float32 once after the division by 3 N.  Shared by tests/test_photometric_{cpu,gpu}.py."""
import numpy as np
import torch

KINDS = ("l1", "l2", "smooth_l1", "huber", "relative_l2", "charbonnier")
PARAMS = {"l1": 0.0, "l2": 0.0, "smooth_l1": 0.25, "huber": 0.3, "relative_l2": 0.0, "charbonnier": 1e-3}
F = np.float32


def target(images=None, ids=None, x=None, y=None, pixels=None, bkgd=None):
    """(n, 3) float32 targets: the gather with clamped indices, byte / 255, the blend."""
    if images is not None:
        n_images, H, W, C = images.shape
        if x is None:
            src = images.reshape(-1, C)
        else:
            i = np.zeros_like(x) if ids is None else np.clip(ids, 0, n_images - 1)
            src = images[i, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        p = src.astype(F) / F(255.0) if images.dtype == np.uint8 else src.astype(F)
    else:
        p = pixels.astype(F)
    if p.shape[-1] == 3 or bkgd is None:
        return np.ascontiguousarray(p[:, :3])
    a = p[:, 3:4]
    return p[:, :3] * a + bkgd.astype(F) * (F(1.0) - a)


def sign0(d):
    return np.where(d > 0, F(1.0), np.where(d < 0, F(-1.0), d)).astype(F)


def term(kind, param, d, rgb, grad=False):
    """The per-element term (grad: its derivative with respect to d) in float32."""
    P, ad = F(param), np.abs(d)
    with np.errstate(all="ignore"):
        if kind == "l1":
            out = sign0(d) if grad else ad
        elif kind == "l2":
            out = F(2.0) * d if grad else d * d
        elif kind == "smooth_l1":
            if P == 0:
                out = sign0(d) if grad else ad
            else:
                out = np.where(ad < P, d / P, sign0(d)) if grad else np.where(ad < P, ((F(0.5) * d) * d) / P, ad - F(0.5) * P)
        elif kind == "huber":
            out = np.where(ad <= P, d, P * sign0(d)) if grad else np.where(ad <= P, (F(0.5) * d) * d, P * (ad - F(0.5) * P))
        elif kind == "relative_l2":
            den = rgb * rgb + F(0.01)
            out = (F(2.0) * d) / den if grad else (d * d) / den
        elif kind == "charbonnier":
            r = np.sqrt(d * d + P * P)
            out = d / r if grad else r
        else:
            raise KeyError(kind)
    assert out.dtype == F
    return out


def forward(rgb, pixels, kind, param, weights=None):
    """(loss, mse, per_ray) for float32 rgb and targets of shape (n, 3)."""
    rgb, pixels = rgb.astype(F), pixels.astype(F)
    n = rgb.shape[0]
    d = rgb - pixels
    t = term(kind, param, d, rgb)
    wt = t if weights is None else weights.astype(F)[:, None] * t
    s = (t[:, 0] + t[:, 1]) + t[:, 2]
    per_ray = (s if weights is None else weights.astype(F) * s) / F(3.0)
    with np.errstate(all="ignore"):
        loss = F(np.sum(wt.astype(np.float64)) / np.float64(3 * n))
        mse = F(np.sum((d * d).astype(np.float64)) / np.float64(3 * n))
    return loss, mse, per_ray


def backward(rgb, pixels, kind, param, g, weights=None):
    """g_rgb (n, 3) float32, before the rounding to rgb's type: ((g * w) * inv) * dterm/dd, inv = float32(1) / float32(3 n)."""
    rgb, pixels = rgb.astype(F), pixels.astype(F)
    n = rgb.shape[0]
    inv = F(1.0) / F(3 * n)
    coef = np.full(n, F(g) * inv, F) if weights is None else (F(g) * weights.astype(F)) * inv
    out = coef[:, None] * term(kind, param, rgb - pixels, rgb, grad=True)
    assert out.dtype == F
    return out


def rounded(values, dtype):
    """float32 values rounded once (to nearest even) to a torch dtype, as a CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(values)).to(dtype)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def random_stack(seed, shape=(3, 5, 7, 4)):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def random_indices(seed, n, shape=(3, 5, 7), dtype=np.int64):
    r = np.random.default_rng(seed)
    return tuple(r.integers(0, s, n).astype(dtype) for s in shape)


def exact_case(seed, n):
    """rgb and targets that are multiples of 2^-6 in [0, 1]: with beta = 1 every smooth_l1 term and every sum is exact."""
    r = np.random.default_rng(seed)
    return (r.integers(0, 65, (n, 3)) / 64.0).astype(F), (r.integers(0, 65, (n, 3)) / 64.0).astype(F)
