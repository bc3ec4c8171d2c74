"""nerfacc_amd.fields.VanillaNeRFRadianceField without a GPU: the torch path, the reference's state dict, the table of fused
shapes, and the argument checks of the entries of nerfacc_amd/csrc/nerf_field.hip (no check launches anything)."""
import pytest
import torch

import mlp_stream_reference as M
from nerfacc_amd import _backend as B
from nerfacc_amd.encodings import _sinusoidal_torch
from nerfacc_amd.fields import VanillaNeRFRadianceField, nerf_field_limits_error

P = 0x10000   # a non-null, 16-byte aligned address that no refused call reads
F16, BF16, F32 = 1, 2, 0
TRUNK, HEAD = dict(n_in=63, n_out=257, width=256, n_hidden=8, bias=1, skip_mask=32), dict(n_in=283, n_out=3, width=128, n_hidden=1, bias=1, skip_mask=0)
ENTRIES = ["nfa_nerf_field", "nfa_nerf_density", "nfa_nerf_pack_head"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cpu_tensors_take_the_torch_restatement(dtype):
    f = VanillaNeRFRadianceField(2, 128, 1, 2, dtype=dtype)   # a cat output layer
    f.mlp.load_reference_state_dict(M.nerf_state_dict("xavier", 63, 27, 2, 128, 1, 2, 128))
    gen = torch.Generator().manual_seed(1)
    x, d = torch.rand(50, 3, generator=gen) * 2 - 1, torch.randn(50, 3, generator=gen)
    rgb, sigma = f.mlp(_sinusoidal_torch(x, 0, 10, True).to(dtype), _sinusoidal_torch(d, 0, 4, True).to(dtype))
    got = f(x, d)
    assert torch.equal(got[0], torch.sigmoid(rgb)) and torch.equal(got[1], torch.relu(sigma)) and got[1].shape == (50, 1)
    assert torch.equal(f.query_density(x), torch.relu(sigma)) and torch.equal(f.query_opacity(x, 0.5), torch.relu(sigma) * 0.5)
    raw = f.query_raw(x, d)
    assert torch.equal(raw[0], rgb) and torch.equal(raw[1], sigma[:, 0])


def test_reference_state_dict():
    f = VanillaNeRFRadianceField(3, 128, 2, 2)
    inner = M.nerf_state_dict("xavier", 63, 27, 3, 128, 2, 2, 128)
    sd = {"mlp." + k: v for k, v in inner.items()}
    sd["posi_encoder.scales"], sd["view_encoder.scales"] = 2.0 ** torch.arange(10), 2.0 ** torch.arange(4)
    f.load_reference_state_dict(sd)
    assert torch.equal(f.mlp.head.weight(0), inner["rgb_layer.hidden_layers.0.weight"])
    assert torch.equal(f.mlp.trunk.weight(3)[128:], inner["sigma_layer.output_layer.weight"])
    assert set("mlp." + k for k in f.mlp.reference_keys()) == set(sd) - {"posi_encoder.scales", "view_encoder.scales"}
    for bad in ({**sd, "warp.weight": torch.zeros(1)}, {**sd, "view_encoder.scales": 2.0 ** torch.arange(5)},
                {k: v for k, v in sd.items() if k != "mlp.sigma_layer.output_layer.bias"}):
        with pytest.raises(ValueError):
            f.load_reference_state_dict(bad)


@pytest.mark.parametrize("kw,full,density", [
    (dict(), True, True), (dict(net_width=128, net_depth=1, skip_layer=None), True, True), (dict(net_depth=8, skip_layer=1), True, True),
    (dict(net_depth_condition=4), True, True), (dict(net_depth_condition=5), False, True), (dict(net_width_condition=256), False, True),
])
def test_fused_supported(kw, full, density):
    f = VanillaNeRFRadianceField(**kw)
    assert f.fused_supported(True) is full and f.fused_supported(False) is density


def _calls(elem=F16, n=64, trunk=None, head=None, tw=256, img=P, bias=P, out=P, inp=True, positions=P, dirs=P, activated=0, out_elem=F32,
           elems=None, descs=True):
    lib = B.load()
    t, h = (B.MLPDesc(**{**TRUNK, **(trunk or {})}), B.MLPDesc(**{**HEAD, **(head or {})})) if descs else (None, None)
    i = B.NGPInput(positions, dirs, None, None, None, None, None, 0) if inp else None
    fe = (4 * 18 + 8) * 512 if elems is None else elems   # the reference head's image: 4 row tiles x 18 k-steps, one output tile x 8
    return {
        "nfa_nerf_field": lambda: lib.nfa_nerf_field(elem, t, h, img, img, bias, bias, i, n, activated, out, out_elem, out, out_elem, None),
        "nfa_nerf_density": lambda: lib.nfa_nerf_density(elem, t, img, bias, i, n, activated, out, out_elem, None),
        "nfa_nerf_pack_head": lambda: lib.nfa_nerf_pack_head(elem, h, tw, bias, img, fe, None),
    }


@pytest.mark.parametrize("entry,kw,msg", [(e, kw, msg) for e in ENTRIES[:2] for kw, msg in [
    (dict(descs=False), b"descriptor is null"), (dict(elem=F32), b"elem 0"), (dict(n=-1), b"n_points -1 is negative"),
    (dict(inp=False), b"input descriptor is null"), (dict(activated=2), b"activated must be 0"), (dict(out_elem=BF16), b"sigma_elem 2"),
    (dict(img=None), b"null pointer (image or bias)"), (dict(bias=None), b"null pointer (image or bias)"), (dict(out=None), b"no output requested"),
    (dict(img=P + 8), b"misaligned"), (dict(bias=P + 2), b"misaligned"), (dict(out=P + 2), b"misaligned"),
    (dict(trunk=dict(width=64, n_out=65)), b"trunk width 64"), (dict(trunk=dict(n_in=64)), b"trunk n_in 64"), (dict(trunk=dict(skip_mask=2)), b"skip_mask 0x2"),
]] + [
    ("nfa_nerf_field", dict(dirs=None), b"null input pointer"), ("nfa_nerf_field", dict(head=dict(width=256)), b"head width 256"),
    ("nfa_nerf_pack_head", dict(descs=False), b"descriptor is null"), ("nfa_nerf_pack_head", dict(tw=64), b"trunk width 64"),
    ("nfa_nerf_pack_head", dict(elems=512), b"the image holds 40960 elements for this shape, got 512"),
    ("nfa_nerf_pack_head", dict(img=None), b"null pointer"), ("nfa_nerf_pack_head", dict(img=P + 8), b"misaligned"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    assert _calls(**kw)[entry]() == -1
    assert msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()


def test_empty_queries_read_no_pointer():
    for entry in ENTRIES[:2]:
        assert _calls(n=0, img=None, bias=None, out=None, positions=None, dirs=None)[entry]() == 0


@pytest.mark.parametrize("trunk,head", [
    (dict(width=64, n_out=65), {}), (dict(n_hidden=9), {}), (dict(n_in=27), {}), (dict(n_out=256), {}), (dict(bias=0), {}), (dict(skip_mask=3), {}),
    ({}, dict(width=64)), ({}, dict(n_hidden=5)), ({}, dict(n_in=155)), ({}, dict(n_out=4)), ({}, dict(bias=0)), ({}, dict(skip_mask=4)),
])
def test_python_and_the_entries_refuse_in_the_same_words(trunk, head):
    t, h = {**TRUNK, **trunk}, {**HEAD, **head}
    want = nerf_field_limits_error(tuple(t.values()), tuple(h.values()))
    lib = B.load()
    assert want and _calls(trunk=trunk, head=head)["nfa_nerf_field"]() == -1
    assert lib.nfa_last_error().decode() == "nfa_nerf_field: " + want
    if not trunk:   # the pack entry knows the trunk by its width
        assert _calls(head=head)["nfa_nerf_pack_head"]() == -1
        assert lib.nfa_last_error().decode() == "nfa_nerf_pack_head: " + nerf_field_limits_error(None, tuple(h.values()), 256)
