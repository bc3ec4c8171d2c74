"""CPU: the NDR T-NeRF field's composed chain against the reference's own class (tests/golden/ref_ndr_field.npz, written by
scripts/gen_ndr_golden.py), its state-dict loader, what fused_supported accepts, and the new entries' names."""
import os

import numpy as np
import pytest
import torch

import mlp_stream_reference as M
import ndr_field_reference as R
from conftest import ROOT
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import NDRTNeRFRadianceField, VanillaNeRFRadianceField
from nerfacc_amd.mlp import reference_mlp

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_ndr_field.npz")


def test_entries_state_dict_and_fused_supported():
    assert {"nfa_ndr_field", "nfa_ndr_density", "nfa_ndr_warp", "nfa_ndr_time_features"} <= set(B.EXPORTED_SYMBOLS)
    assert B.ABI_VERSION == 403 and B.load().nfa_version() == 403
    f = NDRTNeRFRadianceField()
    assert f.fused_supported(True) and f.fused_supported(False)
    for net, depth in ((f.warp_layers_1[2], 2), (f.warp_layers_2[0], 1)):
        out = net.weight(depth).detach()
        assert net.out_dtype == torch.float32 and 0 <= float(out.min()) and 0 < float(out.max()) <= 1e-4 and not net.bias(depth).any()
    sd = R.reference_state_dict("rot")
    for name, n in (("time_encoder", 4), ("posi_encoder_1", 4), ("posi_encoder_2", 4), ("nerf.posi_encoder", 10), ("nerf.view_encoder", 4)):
        sd[name + ".scales"] = 2.0 ** torch.arange(n)
    f.nerf = VanillaNeRFRadianceField(2, 128, 4)
    f.load_reference_state_dict(sd)
    assert torch.equal(f.warp_layers_1[1].weight(1), sd["warp_layers_1.1.hidden_layers.1.weight"])
    assert torch.equal(f.warp_layers_2[2].bias(1), sd["warp_layers_2.2.output_layer.bias"])
    assert torch.equal(f.time_layers_2[1].weight, sd["time_layers_2.1.output_layer.weight"])
    for bad in ({**sd, "warp_layers_3.0.weight": torch.zeros(1)}, {**sd, "posi_encoder_1.scales": 2.0 ** torch.arange(5)},
                {k: v for k, v in sd.items() if k != "warp_layers_2.1.output_layer.bias"}, {k: v for k, v in sd.items() if k != "time_layers_1.0.output_layer.bias"},
                {**sd, "warp_layers_1.0.hidden_layers.1.weight": torch.zeros(64, 64)}, {**sd, "time_layers_2.2.output_layer.weight": torch.zeros(64, 8)}):
        with pytest.raises(ValueError):
            f.load_reference_state_dict(bad)
    f.warp_layers_1[0] = reference_mlp(82, 1, 2, 64, None, out_dtype=torch.float32)
    assert not f.fused_supported(True) and not f.fused_supported(False)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(R.FIELDS))
def test_composed_chain_against_the_reference(name, dtype):
    """`warp` against the reference's float64 run within the derived bound of the half-type chain.  Both families' bound is a few
    roundings: for a third of the elements at least it is under a tenth of the element's move and, for `rot`, a quarter of theta
    (asserted: a loose bound must not pass silently), so a wrong block order, roll, rotation sign or a dropped bias fails.  The
    outputs are the vanilla field's at `warped` bit for bit; that field has its own fixture."""
    g = np.load(GOLDEN)
    depth, width, skip, kind = R.FIELDS[name]
    f = NDRTNeRFRadianceField(dtype=dtype)
    f.nerf = VanillaNeRFRadianceField(depth, width, skip, dtype=dtype)
    sd = R.reference_state_dict(name)
    assert abs(M.checksum(sd) - float(g[name + "/checksum"])) <= 1e-9 * abs(float(g[name + "/checksum"]))
    f.load_reference_state_dict(sd)
    x, t, want = torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g[name + "/warped"]).double()
    d = torch.nn.functional.normalize(x.flip(-1) + 0.5, dim=-1)
    with torch.no_grad():
        rgb, sigma = f(x, t, d)
        density, xw = f.query_density(x, t), f.warp(x, t)
        assert all(torch.equal(a, b) for a, b in zip((rgb, sigma, density), (*f.nerf(xw, d), f.nerf.query_density(xw))))
    b = R.golden_bound(R.perm_weights(kind == "rot"), f, x, t, dtype)
    bound, theta = b["e_warped"] + R.ulp(torch.float32, want.abs()), b["theta"]
    frac = lambda what: float((bound < what).double().mean())   # the share of elements whose bound is well under an effect
    ratio, sharp, sharp_rot = R.worst_ratio(xw, want, bound), frac(0.1 * (want - x).abs()), frac(0.25 * theta)
    print(f"NDR golden (cpu) {name} {dtype}: error / bound {ratio:.2e}; bound median {float(bound.median()):.1e}, max {float(bound.max()):.1e}; "
          f"moved (median) {float((want - x).abs().median()):.2f}, largest theta {theta:.2f}; bound < move / 10 for {sharp:.2f}, < theta / 4 for {sharp_rot:.2f}")
    assert xw.dtype == torch.float32 and rgb.shape == (x.shape[0], 3) and sigma.shape == density.shape == (x.shape[0], 1)
    assert sharp >= 1 / 3 and (sharp_rot >= 1 / 3 if kind == "rot" else theta == 0)
    assert ratio <= 1.0
