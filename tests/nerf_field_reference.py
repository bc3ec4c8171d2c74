"""The float64 restatement of the fused NeRF field query (nerfacc_amd/csrc/nerf_field.hip, nerfacc_amd.fields.VanillaNeRFRadianceField).

Its input is the encoded rows as the native ``SinusoidalEncoding(out_dtype=elem)`` stores them (pinned by that module's own tests:
a float64 sine rounded to half differs from an accurate float32 sincosf rounded to half on a few values in ten thousand).  Behind
them: the trunk, the split, the cat and the head through the functions and the bound rule of tests/mlp_stream_reference.py.
"""
import torch

import mlp_bias_skip_reference as S
import mlp_reference as R
import mlp_stream_reference as M
from mlp_reference import U32, rnd, ulp, worst_ratio  # noqa: F401

POS_DIMS, DIR_DIMS = 63, 27


def perm_weights(width, depth, skip_layer, depth_c, roll):
    """The 'perm' family for both networks with ONE term in every sum: at a cat layer the even neurons keep their H entry and
    the odd ones their x entry.  ``roll = (trunk, head)`` moves the columns of the two first layers, so that other columns of
    the encoded rows reach the four outputs.  Biases are zero: every number of the run is +-1 or +-2 times an encoded value."""
    mask = S.skip_mask_of(skip_layer, depth)
    tw = S.exact_weights("perm", POS_DIMS, width + 1, width, depth, mask)
    for l in range(1, depth + 1):
        if S.is_cat(mask, l):
            odd = (torch.arange(tw[l].shape[0]) % 2 == 1).view(-1, 1)
            tw[l] = torch.cat([tw[l][:, :width] * ~odd, tw[l][:, width:] * odd], 1)
    hw = R.exact_weights("perm", width + DIR_DIMS, 3, 128, depth_c)
    tw[0], hw[0] = torch.roll(tw[0], roll[0], 1), torch.roll(hw[0], roll[1], 1)
    zeros = lambda ws: [torch.zeros(w.shape[0]) for w in ws]
    return mask, tw, zeros(tw), hw, zeros(hw)


def query(enc_x, enc_d, tw, tb, hw, hb, mask, dtype, exact=False):
    """enc_x [N, 63], enc_d [N, 27] or None: tensors of ``dtype``.  Returns the raw float32-side values and their bounds:
    dict(sigma, e_sigma, rgb, e_rgb).  ``exact``: every rounding is asserted to be a no-op and the bounds are zero; otherwise
    the encoded rows carry one rounding as incoming error."""
    W = tw[0].shape[0]
    if exact:
        t = S.forward(enc_x, tw, tb, mask, dtype, out_f32=True, exact=True)
    else:
        x0 = enc_x.double()
        t = M.forward_with_error(x0, ulp(dtype, x0), tw, tb, mask, dtype, out_f32=True)
    z, e = t["y"], t["e_y"]
    out = dict(sigma=z[:, W], e_sigma=e[:, W])
    if enc_d is not None:
        bott, e_b = rounded(z[:, :W], e[:, :W], dtype, exact)
        if exact:
            h = S.forward(torch.cat([bott.to(dtype), enc_d], 1), hw, hb, 0, dtype, out_f32=True, exact=True)
        else:
            d0 = enc_d.double()
            h = M.forward_with_error(torch.cat([bott, d0], 1), torch.cat([e_b, ulp(dtype, d0)], 1), hw, hb, 0, dtype, out_f32=True)
        out.update(rgb=h["y"], e_rgb=h["e_y"])
    return out


def head(bott, enc_d, hw, hb, dtype):
    """The head alone on inputs that carry no error: ``bott`` [N, W] the bottleneck as the native trunk stores it (the fused
    launch forms the same bits: its trunk sums in the trunk's order) and ``enc_d``, tensors of ``dtype``.  The bound is then
    the head's own: the float32 sums of its one to four layers in any order and a rounding per hidden activation, a few ulps
    of ``dtype``, so it separates a wrong bias, k-step or epilogue from a right one.  Returns dict(rgb, e_rgb), float32 side."""
    x0 = torch.cat([bott.double(), enc_d.double()], 1)
    h = M.forward_with_error(x0, torch.zeros_like(x0), hw, hb, 0, dtype, out_f32=True)
    return dict(rgb=h["y"], e_rgb=h["e_y"])


def rounded(v, e, dtype, exact=False):
    """A raw value stored in ``dtype``."""
    return rnd(v, dtype, exact), e + ulp(dtype, v.abs() + e)


def activated(v, e, dtype, colour, exact=False):
    """The activated output in float32: relu, or the sigmoid (slope <= 1/4; expf, the sum and the quotient each within an
    ulp or two of a value <= 1: 8 U32) of the raw value rounded to ``dtype`` (``exact``: that rounding is a no-op)."""
    r, er = (rnd(v, dtype, True), e) if exact else rounded(v, e, dtype)
    return (torch.sigmoid(r), er / 4 + 8 * U32) if colour else (torch.relu(r), er)
