"""TNeRFRadianceField without a GPU: the composed chain on CPU tensors against a golden fixture of the reference's own class, the
reference's state dict, and the argument checks of the T-NeRF entries of csrc/nerf_field.hip (no check launches anything)."""
import os

import numpy as np
import pytest
import torch

import mlp_stream_reference as M
import tnerf_field_reference as T
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import TNeRFRadianceField, VanillaNeRFRadianceField, tnerf_field_limits_error

P = 0x10000   # a non-null, 16-byte aligned address that no refused call reads
F16, BF16, F32 = 1, 2, 0
WARP = dict(n_in=36, n_out=3, width=64, n_hidden=4, bias=1, skip_mask=8)
TRUNK, HEAD = dict(n_in=63, n_out=257, width=256, n_hidden=8, bias=1, skip_mask=32), dict(n_in=283, n_out=3, width=128, n_hidden=1, bias=1, skip_mask=0)
ENTRIES = ["nfa_tnerf_field", "nfa_tnerf_density", "nfa_tnerf_warp"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tnerf.npz")


def _calls(elem=F16, n=64, warp=None, trunk=None, head=None, img=P, bias=P, out=P, warped=P, times=P, inp=True, positions=P, dirs=P,
           activated=0, out_elem=F32, descs=True):
    lib = B.load()
    w, t, h = [B.MLPDesc(**{**base, **(kw or {})}) if descs else None for base, kw in ((WARP, warp), (TRUNK, trunk), (HEAD, head))]
    i = B.NGPInput(positions, dirs, None, None, None, None, None, 0) if inp else None
    return {
        "nfa_tnerf_field": lambda: lib.nfa_tnerf_field(elem, w, t, h, img, img, img, bias, bias, bias, i, times, n, activated, out, out_elem, out,
                                                       out_elem, warped, None),
        "nfa_tnerf_density": lambda: lib.nfa_tnerf_density(elem, w, t, img, img, bias, bias, i, times, n, activated, out, out_elem, warped, None),
        "nfa_tnerf_warp": lambda: lib.nfa_tnerf_warp(elem, w, img, bias, i, times, n, warped, None),
    }


@pytest.mark.parametrize("entry,kw,msg", [(e, kw, msg) for e in ENTRIES for kw, msg in [
    (dict(descs=False), b"descriptor is null"), (dict(elem=F32), b"elem 0"), (dict(n=-1), b"n_points -1 is negative"),
    (dict(inp=False), b"input descriptor is null"), (dict(times=None), b"null pointer (warp image, warp bias or times)"),
    (dict(img=P + 8), b"misaligned"), (dict(warped=P + 2), b"misaligned"), (dict(warp=dict(n_in=63)), b"warp n_in 63"),
]] + [
    ("nfa_tnerf_field", dict(dirs=None), b"null input pointer"), ("nfa_tnerf_field", dict(activated=2), b"activated must be 0"),
    ("nfa_tnerf_density", dict(out=None), b"no output requested"), ("nfa_tnerf_warp", dict(warped=None), b"no output requested"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    assert _calls(**kw)[entry]() == -1
    assert msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()
    assert _calls(n=0, img=None, bias=None, out=None, warped=None, times=None, positions=None, dirs=None)[entry]() == 0   # reads no pointer


@pytest.mark.parametrize("warp,trunk,head", [
    (dict(width=128), {}, {}), (dict(n_hidden=5), {}, {}), (dict(n_in=27), {}, {}), (dict(n_out=4), {}, {}), (dict(bias=0), {}, {}),
    (dict(skip_mask=3), {}, {}), (dict(n_hidden=2, skip_mask=8), {}, {}), ({}, dict(n_hidden=9), {}), ({}, {}, dict(n_hidden=5)),
])
def test_python_and_the_entries_refuse_in_the_same_words(warp, trunk, head):
    w, t, h = {**WARP, **warp}, {**TRUNK, **trunk}, {**HEAD, **head}
    want = tnerf_field_limits_error(tuple(w.values()), tuple(t.values()), tuple(h.values()))
    lib = B.load()
    assert want and _calls(warp=warp, trunk=trunk, head=head)["nfa_tnerf_field"]() == -1
    assert lib.nfa_last_error().decode() == "nfa_tnerf_field: " + want
    for entry in ["nfa_tnerf_density"] * (not head) + ["nfa_tnerf_warp"] * bool(warp):
        assert _calls(warp=warp, trunk=trunk)[entry]() == -1 and lib.nfa_last_error().decode() == entry + ": " + want
    assert tnerf_field_limits_error(tuple(WARP.values()), tuple(TRUNK.values()), tuple(HEAD.values())) is None


def test_reference_state_dict():
    f = TNeRFRadianceField()
    assert f.warp.out_dtype == torch.float32 and f.warp.skip_mask == 8 and f.fused_supported(True) and f.fused_supported(False)
    out = f.warp.weight(4).detach()
    assert 0 <= float(out.min()) and float(out.max()) <= 1e-4 and float(out.max()) > 0 and not f.warp.bias(4).any()
    sd = T.reference_state_dict("ref")
    for name, n in (("posi_encoder", 4), ("time_encoder", 4), ("nerf.posi_encoder", 10), ("nerf.view_encoder", 4)):
        sd[name + ".scales"] = 2.0 ** torch.arange(n)
    f.load_reference_state_dict(sd)
    assert torch.equal(f.warp.weight(3), sd["warp.hidden_layers.3.weight"]) and torch.equal(f.warp.bias(4), sd["warp.output_layer.bias"])
    assert torch.equal(f.nerf.mlp.head.weight(0), sd["nerf.mlp.rgb_layer.hidden_layers.0.weight"])
    for bad in ({**sd, "warp2.weight": torch.zeros(1)}, {**sd, "time_encoder.scales": 2.0 ** torch.arange(5)},
                {k: v for k, v in sd.items() if k != "warp.output_layer.bias"}, {**sd, "warp.hidden_layers.3.weight": torch.zeros(64, 64)},
                {k: v for k, v in sd.items() if k != "nerf.mlp.sigma_layer.output_layer.bias"}):
        with pytest.raises(ValueError):
            f.load_reference_state_dict(bad)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(T.FIELDS))
def test_composed_chain_against_the_reference(name, dtype):
    """Against the reference's float64 run, within the derived bound of the half-type chain.  `perm` is the sharp case: deformations
    up to 2.0 against a bound on `warped` of 5e-3 (fp16) and 7e-2 (bf16), largest error / bound 0.25; a zeroed warp misses it 127 to
    1009 times over.  That the outputs are the vanilla field's at `warped` is asserted bit for bit.  With Xavier weights the bound on
    `warped` is loose (0.4 / 3.6), and the outputs' is for every field (the trunk's 2^9 slope: 1e2 to 1e11); asserted all the same."""
    g = np.load(GOLDEN)
    depth, width, skip, _ = T.FIELDS[name]
    f = TNeRFRadianceField(dtype=dtype)
    f.nerf = VanillaNeRFRadianceField(depth, width, skip, dtype=dtype)
    sd = T.reference_state_dict(name)
    assert abs(M.checksum(sd) - float(g[name + "/checksum"])) <= 1e-9 * abs(float(g[name + "/checksum"]))
    f.load_reference_state_dict(sd)
    x, t, d = [torch.from_numpy(g[k]) for k in ("x", "t", "dir")]
    with torch.no_grad():
        rgb, sigma = f(x, t, d)
        density, xw = f.query_density(x, t), f.warped_positions(x, t)
        assert all(torch.equal(a, b) for a, b in zip((rgb, sigma, density), (*f.nerf(xw, d), f.nerf.query_density(xw))))
    b = T.golden_bound(f, x, t, d, dtype)
    want = lambda k: torch.from_numpy(g[name + "/" + k]).double()
    ratios = {k: T.worst_ratio(v, want(k), b[e] + T.ulp(torch.float32, want(k).abs()))
              for k, v, e in (("warped", xw, "e_warped"), ("rgb", rgb, "e_rgb"), ("sigma", sigma, "e_sigma"), ("density", density, "e_sigma"))}
    print(f"T-NeRF golden (cpu) {name} {dtype}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items())
          + "; bounds <= " + ", ".join(f"{k} {float(v.max()):.1e}" for k, v in b.items()) + f"; deformation <= {float((xw - x).abs().max()):.2f}")
    assert xw.dtype == torch.float32 and rgb.shape == (x.shape[0], 3) and sigma.shape == density.shape == (x.shape[0], 1)
    assert all(r <= 1.0 for r in ratios.values())
