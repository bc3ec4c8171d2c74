"""VanillaNeRFRadianceField(fused_training=True) without a GPU: CPU tensors keep the composed chain, and the argument checks of
nfa_nerf_train_fwd (nerfacc_amd/csrc/nerf_field.hip) and nfa_nerf_train_bwd (nerfacc_amd/csrc/nerf_train.hip), none of which
launches anything."""
import pytest
import torch

from nerfacc_amd import _backend as B
from nerfacc_amd.fields import VanillaNeRFRadianceField, nerf_field_limits_error
from test_nerf_field_cpu import BF16, F16, F32, HEAD, P, TRUNK


def test_cpu_tensors_keep_the_composed_chain():
    on, off = VanillaNeRFRadianceField(2, 128, 1, 2, fused_training=True), VanillaNeRFRadianceField(2, 128, 1, 2)
    off.load_state_dict(on.state_dict())
    gen = torch.Generator().manual_seed(1)
    x, d = torch.rand(50, 3, generator=gen) * 2 - 1, torch.randn(50, 3, generator=gen)
    grads = []
    for f in (on, off):
        rgb, sigma = f(x, d)
        (rgb.float().sum() + sigma.float().sum()).backward()
        grads.append((rgb.detach(), sigma.detach(), f.mlp.trunk.params.grad, f.mlp.head.params.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads)) and grads[0][2].abs().max() > 0


def _call(entry, elem=F16, n=64, trunk=None, head=None, descs=True, img=P, activated=0, save=True, grads=True, g_elem=F32, y_elem=F16, hidden=P,
          dz=P, dzo=P, g=P, y=None, inp=True, out=P, enc_x=P):
    lib = B.load()
    t, h = (B.MLPDesc(**{**TRUNK, **(trunk or {})}), B.MLPDesc(**{**HEAD, **(head or {})})) if descs else (None, None)
    sv = B.NerfSaved(enc_x, hidden, P, hidden) if save else None
    if entry == "nfa_nerf_train_fwd":
        i = B.NGPInput(P, P, None, None, None, None, None, 0) if inp else None
        return lib.nfa_nerf_train_fwd(elem, t, h, img, img, P, P, i, n, activated, sv, out, F32, out, F32, None)
    gr = B.NerfGrads(g, g_elem, g, g_elem, y, y_elem, y, y_elem, dz, P, dz, dzo) if grads else None
    return lib.nfa_nerf_train_bwd(elem, t, h, img, img, n, activated, sv, gr, None)


FWD, BWD = "nfa_nerf_train_fwd", "nfa_nerf_train_bwd"


# in the entries' order of checking: the later a row, the more of the earlier arguments are valid
@pytest.mark.parametrize("entry,kw,msg", [
    (FWD, dict(elem=F32), b"elem 0"), (FWD, dict(descs=False), b"descriptor is null"), (FWD, dict(trunk=dict(n_in=64)), b"trunk n_in 64"),
    (FWD, dict(n=-1), b"n_points -1 is negative"), (FWD, dict(inp=False), b"input descriptor is null"),
    (FWD, dict(save=False), b"saved-buffers descriptor is null"), (FWD, dict(activated=2), b"activated must be 0"),
    (FWD, dict(img=None), b"null pointer (image or bias)"), (FWD, dict(out=None), b"no output requested"), (FWD, dict(out=P + 2), b"misaligned"),
    (FWD, dict(hidden=None), b"null pointer (enc_x, trunk_hidden, head_in or head_hidden)"), (FWD, dict(enc_x=P + 8), b"the saved buffers 16"),
    (BWD, dict(elem=F32), b"elem 0"), (BWD, dict(descs=False), b"descriptor is null"), (BWD, dict(head=dict(width=256)), b"head width 256"),
    (BWD, dict(n=-1), b"n_points -1 is negative"), (BWD, dict(save=False), b"saved-buffers descriptor is null"),
    (BWD, dict(grads=False), b"gradients descriptor is null"), (BWD, dict(activated=2), b"activated must be 0"),
    (BWD, dict(g_elem=BF16), b"g_rgb_elem 2"), (BWD, dict(activated=1, y_elem=BF16), b"y_rgb_elem 2"), (BWD, dict(img=None), b"null pointer (image)"),
    (BWD, dict(hidden=None), b"null pointer (trunk_hidden or head_hidden)"), (BWD, dict(dz=None), b"null pointer (head_dz"),
    (BWD, dict(activated=1), b"y_rgb and y_sigma are read"), (BWD, dict(dzo=P + 8), b"misaligned"), (BWD, dict(g=P + 2), b"misaligned"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    assert _call(entry, **kw) == -1
    assert msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()


def test_empty_queries_and_null_gradients_read_no_pointer():
    assert _call(FWD, n=0, img=None, out=None, hidden=None, enc_x=None) == 0
    assert _call(BWD, n=0, img=None, hidden=None, dz=None, dzo=None, g=None) == 0


@pytest.mark.parametrize("entry", [FWD, BWD])
@pytest.mark.parametrize("trunk,head", [(dict(width=64, n_out=65), {}), (dict(n_hidden=9), {}), (dict(skip_mask=3), {}), ({}, dict(n_hidden=5)),
                                        ({}, dict(n_in=155)), ({}, dict(skip_mask=4))])
def test_python_and_the_entries_refuse_in_the_same_words(entry, trunk, head):
    want = nerf_field_limits_error(tuple({**TRUNK, **trunk}.values()), tuple({**HEAD, **head}.values()))
    assert want and _call(entry, trunk=trunk, head=head) == -1
    assert B.load().nfa_last_error().decode() == f"{entry}: {want}"
