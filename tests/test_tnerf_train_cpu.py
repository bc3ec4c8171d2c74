"""TNeRFRadianceField(fused_training=True) without a GPU: CPU tensors keep the composed chain, and the argument checks of
nfa_tnerf_train_fwd (nerfacc_amd/csrc/nerf_field.hip) and nfa_tnerf_train_bwd (nerfacc_amd/csrc/nerf_train.hip), none of which
launches anything."""
import pytest
import torch

import tnerf_field_reference as T
from nerfacc_amd import _backend as B
from nerfacc_amd.fields import TNeRFRadianceField, VanillaNeRFRadianceField, tnerf_field_limits_error
from test_tnerf_field_cpu import BF16, F16, F32, HEAD, P, TRUNK, WARP

FWD, BWD = "nfa_tnerf_train_fwd", "nfa_tnerf_train_bwd"


def test_cpu_tensors_keep_the_composed_chain():
    fields = []
    for ft in (True, False):
        f = TNeRFRadianceField(fused_training=ft)
        f.nerf = VanillaNeRFRadianceField(2, 128, 1, 2)
        f.warp.load_linear_weights(*T.xavier_weights())
        f.load_state_dict(fields[0].state_dict()) if fields else None
        fields.append(f)
    gen = torch.Generator().manual_seed(1)
    x, t, d = torch.rand(50, 3, generator=gen) * 2 - 1, torch.rand(50, 1, generator=gen), torch.randn(50, 3, generator=gen)
    grads = []
    for f in fields:
        rgb, sigma = f(x, t, d)
        (rgb.float().sum() + sigma.float().sum()).backward()
        grads.append((rgb.detach(), sigma.detach(), *[p.grad for p in f.parameters()]))
    assert all(torch.equal(a, b) for a, b in zip(*grads)) and all(g.abs().max() > 0 for g in grads[0][2:])


def _call(entry, elem=F16, n=64, warp=None, trunk=None, head=None, descs=True, img=P, activated=0, save=True, wsave=True, grads=True, wgrads=True,
          g_elem=F32, y_elem=F16, hidden=P, dz=P, dzo=P, g=P, y=None, inp=True, out=P, enc_x=P, times=P, w_in=P, w_hidden=P, warped=P, wdz=P,
          wdzo=P):
    lib = B.load()
    w, t, h = [B.MLPDesc(**{**base, **(kw or {})}) if descs else None for base, kw in ((WARP, warp), (TRUNK, trunk), (HEAD, head))]
    sv = B.NerfSaved(enc_x, hidden, P, hidden) if save else None
    wsv = B.TNerfSaved(w_in, w_hidden, warped) if wsave else None
    if entry == FWD:
        i = B.NGPInput(P, P, None, None, None, None, None, 0) if inp else None
        return lib.nfa_tnerf_train_fwd(elem, w, t, h, img, img, img, P, P, P, i, times, n, activated, sv, wsv, out, F32, out, F32, None)
    gr = B.NerfGrads(g, g_elem, g, g_elem, y, y_elem, y, y_elem, dz, P, dz, dzo) if grads else None
    wgr = B.TNerfGrads(wdz, wdzo) if wgrads else None
    return lib.nfa_tnerf_train_bwd(elem, w, t, h, img, img, img, n, activated, sv, wsv, gr, wgr, None)


# in the entries' order of checking: the later a row, the more of the earlier arguments are valid
@pytest.mark.parametrize("entry,kw,msg", [
    (FWD, dict(elem=F32), b"elem 0"), (FWD, dict(descs=False), b"descriptor is null"), (FWD, dict(warp=dict(n_in=63)), b"warp n_in 63"),
    (FWD, dict(trunk=dict(n_in=64)), b"trunk n_in 64"), (FWD, dict(n=-1), b"n_points -1 is negative"),
    (FWD, dict(inp=False), b"input descriptor is null"), (FWD, dict(save=False), b"saved-buffers descriptor is null"),
    (FWD, dict(wsave=False), b"saved-buffers descriptor is null"), (FWD, dict(activated=2), b"activated must be 0"),
    (FWD, dict(img=None), b"null pointer (image or bias)"), (FWD, dict(out=None), b"no output requested"), (FWD, dict(out=P + 2), b"misaligned"),
    (FWD, dict(times=None), b"null pointer (warp image, warp bias or times)"), (FWD, dict(hidden=None), b"null pointer (enc_x, trunk_hidden"),
    (FWD, dict(warped=None), b"null pointer (warp_in, warp_hidden or warped)"), (FWD, dict(w_in=P + 8), b"the saved buffers 16"),
    (BWD, dict(elem=F32), b"elem 0"), (BWD, dict(warp=dict(width=128)), b"warp width 128"), (BWD, dict(head=dict(width=256)), b"head width 256"),
    (BWD, dict(n=-1), b"n_points -1 is negative"), (BWD, dict(wsave=False), b"saved-buffers descriptor is null"),
    (BWD, dict(wgrads=False), b"gradients descriptor is null"), (BWD, dict(activated=2), b"activated must be 0"),
    (BWD, dict(g_elem=BF16), b"g_rgb_elem 2"), (BWD, dict(img=None), b"null pointer (image)"),
    (BWD, dict(hidden=None), b"null pointer (trunk_hidden or head_hidden)"), (BWD, dict(warped=None), b"null pointer (warp_hidden or warped)"),
    (BWD, dict(dz=None), b"null pointer (head_dz"), (BWD, dict(wdzo=None), b"null pointer (warp_dz or warp_dz_out)"),
    (BWD, dict(activated=1), b"y_rgb and y_sigma are read"), (BWD, dict(dzo=P + 8), b"misaligned"), (BWD, dict(wdz=P + 8), b"warp_dz 16"),
])
def test_entry_argument_checks(entry, kw, msg):
    lib = B.load()
    assert _call(entry, **kw) == -1
    assert msg in lib.nfa_last_error() and entry.encode() in lib.nfa_last_error(), lib.nfa_last_error()
    none = dict(n=0, img=None, hidden=None, enc_x=None, times=None, w_in=None, w_hidden=None, warped=None, wdz=None, wdzo=None, dz=None, dzo=None)
    assert _call(entry, **none, out=None, g=None) == 0   # an empty query reads no pointer


@pytest.mark.parametrize("entry", [FWD, BWD])
@pytest.mark.parametrize("warp,trunk,head", [(dict(n_hidden=5), {}, {}), (dict(bias=0), {}, {}), (dict(n_hidden=2, skip_mask=8), {}, {}),
                                             ({}, dict(n_hidden=9), {}), ({}, {}, dict(n_in=155))])
def test_python_and_the_entries_refuse_in_the_same_words(entry, warp, trunk, head):
    want = tnerf_field_limits_error(*[tuple({**base, **kw}.values()) for base, kw in ((WARP, warp), (TRUNK, trunk), (HEAD, head))])
    assert want and _call(entry, warp=warp, trunk=trunk, head=head) == -1
    assert B.load().nfa_last_error().decode() == f"{entry}: {want}"
