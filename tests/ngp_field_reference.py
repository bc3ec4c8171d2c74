"""Float64 restatement of the fused Instant-NGP field query (nerfacc_amd/csrc/ngp_field.hip) with the kernel's rounding points
and a derived error bound per element.

The encoded features, the harmonics and the box coordinates are NOT restated here: they are the package's own op-for-op float32
torch forms (encodings._hashgrid_torch, _sh_torch, the field's _normalise), widened and rounded ONCE to the half type.  So
against the module's CPU path only the network chains and their roundings are independent; against the kernel the encoding
is compared too (another implementation), and the integer-valued GPU test pins its lane maps.  The networks are float64 sums of exact
products with tests/mlp_reference.py's roundings (hidden activations after the ReLU, the base output tile, the raw colour).

Bound: mlp_reference's per-element rule, started from a non-zero input error (its forward() starts from zero): an encoded
feature or harmonic carries one ulp of the half type at its value (the kernel forms it in float32, so a value next to a tie
may round to the neighbour), the geometry feature carries what the rule derives for the base network's output.
"""
import torch

import mlp_reference as R
from nerfacc_amd.encodings import _hashgrid_torch, _sh_torch


def chain(h, e, weights, dtype):
    """mlp_reference.forward's loop from input ``h`` (float64 values of ``dtype`` numbers) with input error ``e``: (y, e_y)."""
    for l, w in enumerate(weights):
        wq = R.rnd(w.double(), dtype)
        z = h @ wq.t() + 0.0
        e_pre = e @ wq.abs().t() + (wq.shape[1] + 2) * R.U32 * (h.abs() @ wq.abs().t())
        h = R.rnd(torch.relu(z) if l < len(weights) - 1 else z, dtype)
        e = e_pre + R.ulp(dtype, z.abs() + e_pre)
    return h, e


def query(field, positions, directions=None):
    """``field``: a CPU NGPRadianceField / NGPDensityField.  Returns dict(sigma, e_sigma, feat, selector[, rgb, e_rgb])."""
    dtype = field.dtype
    with torch.no_grad():
        x, selector = field._normalise(positions.float())
        enc = _hashgrid_torch(x, field.encoding.params.detach(), field.encoding.table, 2, field.encoding.interp).double()
        h = R.rnd(enc, dtype)
        y, e_y = chain(h, R.ulp(dtype, h), [w.detach() for w in field.mlp_base._views(field.mlp_base.params)], dtype)
        out = dict(sigma=y[:, 0], e_sigma=e_y[:, 0], feat=y[:, 1:], selector=selector)
        if directions is not None:
            sh = R.rnd(_sh_torch((directions.float() + 1.0) / 2.0, 4).double(), dtype)
            out["rgb"], out["e_rgb"] = chain(torch.cat([sh, y[:, 1:]], 1), torch.cat([R.ulp(dtype, sh), e_y[:, 1:]], 1),
                                             [w.detach() for w in field.mlp_head._views(field.mlp_head.params)], dtype)
    return out
