"""GPU: unpack_info / unpack_data / pack_data on the native kernels (csrc/pack.hip, nfa_fill_ray_indices) -- bit-exact
against a loop restatement for every dtype and width, gradients, the segment bookkeeping they hand to rendering(), layout
equivalence of the render ops, round trips, the path taken, and the input checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.bool]


def ref_unpack(pi, data, S, pad):
    """Loop restatement on the CPU in data's own dtype (pure data movement: exact)."""
    pi, data = pi.cpu(), data.cpu()
    out = torch.full((pi.shape[0], S, *data.shape[1:]), pad, dtype=data.dtype)
    for r in range(pi.shape[0]):
        start, cnt = int(pi[r, 0]), int(pi[r, 1])
        k = min(cnt, S)
        if k:
            out[r, :k] = data[start:start + k]
    return out


def ref_pack(data, mask):
    data, mask = data.cpu(), mask.cpu()
    cnts = mask.sum(1, dtype=torch.int64)
    return data[mask], torch.stack([torch.cumsum(cnts, 0) - cnts, cnts], dim=-1)


def rand_data(shape, dtype, g):
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) < 0.5
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g).to(dtype)
    return torch.randint(-1000, 1000, shape, generator=g).to(dtype)


def ragged(counts):
    counts = torch.as_tensor(counts, dtype=torch.int64)
    return torch.stack([torch.cumsum(counts, 0) - counts, counts], dim=-1)


def same(a, b):
    """Same shape, dtype and bytes."""
    bits = lambda t: t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 16])
def test_unpack_data_bit_exact(dev, dtype, D):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(D)
    counts = torch.randint(0, 40, (300,), generator=g)
    counts[::7] = 0
    pi = ragged(counts)
    N = int(counts.sum())
    data = rand_data((N, D), dtype, g)
    pad = True if dtype == torch.bool else 3
    for S in (None, 17, 64):
        out = na.unpack_data(pi.to(dev), data.to(dev), S, pad_value=pad)
        S_eff = int(counts.max()) if S is None else S
        assert same(out, ref_unpack(pi, data, S_eff, pad)), (dtype, D, S)
    # 1-D data
    out = na.unpack_data(pi.to(dev), data[:, 0].to(dev), 17, pad_value=pad)
    assert same(out, ref_unpack(pi, data[:, :1], 17, pad)[..., 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 16])
def test_pack_data_bit_exact(dev, dtype, D):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(100 + D)
    R, S = 257, 70                                   # S > 64: two ballot groups per row
    data = rand_data((R, S, D), dtype, g)
    mask = torch.rand(R, S, generator=g) < 0.45
    mask[3] = False
    mask[4] = True
    packed, pi = na.pack_data(data.to(dev), mask.to(dev))
    ref, ref_pi = ref_pack(data, mask)
    assert pi.dtype == torch.int64 and torch.equal(pi.cpu(), ref_pi)
    assert same(packed, ref)
    packed1, _ = na.pack_data(data[..., 0].to(dev), mask.to(dev))
    assert same(packed1, ref[:, 0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.int64])
def test_misaligned_views(dev, dtype):
    """Views with a storage offset take the narrower chunks and still move the right bytes."""
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(9)
    counts = torch.randint(0, 30, (200,), generator=g)
    pi = ragged(counts)
    N = int(counts.sum())
    for D, off in ((4, 1), (4, 2), (8, 3), (3, 1)):
        base = rand_data((N * D + off,), dtype, g)
        view = base.to(dev)[off:].view(N, D)
        assert view.storage_offset() == off
        out = na.unpack_data(pi.to(dev), view, 25, pad_value=0)
        assert same(out, ref_unpack(pi, base[off:].view(N, D), 25, 0))
        R, S = 50, 33
        big = rand_data((R * S * D + off,), dtype, g)
        pview = big.to(dev)[off:].view(R, S, D)
        mask = torch.rand(R, S, generator=g) < 0.5
        packed, _ = na.pack_data(pview, mask.to(dev))
        assert same(packed, ref_pack(big[off:].view(R, S, D), mask)[0])


def test_gaps_out_of_order_and_truncation(dev):
    import nerfacc_amd as na
    data = torch.arange(40, dtype=torch.float32).view(20, 2)
    pi = torch.tensor([[12, 5], [0, 3], [8, 0], [17, 3], [5, 2]])       # gaps at 3, 4, 7..11; out of order
    for S in (2, 4, 6):
        out = na.unpack_data(pi.to(dev), data.to(dev), S, pad_value=-1.0)
        assert same(out, ref_unpack(pi, data, S, -1.0))
    x = data.to(dev).requires_grad_(True)
    na.unpack_data(pi.to(dev), x, 2).backward(torch.full((5, 2, 2), 2.0, device=dev))
    want = torch.zeros(20)
    for r in range(5):
        s, c = pi[r].tolist()
        want[s:s + min(c, 2)] = 2.0
    assert torch.equal(x.grad.cpu(), want[:, None].expand(20, 2))


def test_empty(dev):
    import nerfacc_amd as na
    z = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    assert na.unpack_info(z, 0).shape == (0,)
    assert na.unpack_data(z, torch.zeros(0, 3, device=dev)).shape == (0, 0, 3)
    pi = torch.zeros((4, 2), dtype=torch.int64, device=dev)        # 4 empty rays, no samples
    out = na.unpack_data(pi, torch.zeros(0, 3, device=dev), 5, pad_value=7.0)
    assert out.shape == (4, 5, 3) and (out == 7.0).all()
    assert na.unpack_data(pi, torch.zeros(0, 3, device=dev)).shape == (4, 0, 3)
    packed, pi2 = na.pack_data(torch.zeros(4, 5, 3, device=dev), torch.zeros(4, 5, dtype=torch.bool, device=dev))
    assert packed.shape == (0, 3) and torch.equal(pi2, pi)
    packed, pi3 = na.pack_data(torch.zeros(0, 5, device=dev), torch.zeros(0, 5, dtype=torch.bool, device=dev))
    assert packed.shape == (0,) and pi3.shape == (0, 2)
    x = torch.zeros(4, 5, 3, device=dev, requires_grad=True)
    na.pack_data(x, torch.zeros(4, 5, dtype=torch.bool, device=dev))[0].sum().backward()
    assert (x.grad == 0).all()


def test_gradcheck(dev):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(1)
    counts = torch.tensor([3, 0, 5, 1, 4])
    pi = ragged(counts).to(dev)
    x = torch.randn(13, 3, generator=g, dtype=torch.float64).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d: na.unpack_data(pi, d, 4, pad_value=0.5), (x,))
    gap = torch.tensor([[8, 3], [0, 2], [4, 1]], device=dev)
    assert torch.autograd.gradcheck(lambda d: na.unpack_data(gap, d, 2), (x,))
    y = torch.randn(5, 6, 2, generator=g, dtype=torch.float64).to(dev).requires_grad_(True)
    mask = (torch.rand(5, 6, generator=g) < 0.5).to(dev)
    assert torch.autograd.gradcheck(lambda d: na.pack_data(d, mask)[0], (y,))


def test_unpack_info_roundtrip_and_rendering(dev, monkeypatch):
    import nerfacc_amd as na
    from nerfacc_amd import _backend as B
    g = torch.Generator().manual_seed(2)
    counts = torch.randint(0, 50, (3000,), generator=g)
    counts[5:9] = 0
    pi = ragged(counts).to(dev)
    N, R = int(counts.sum()), 3000
    ri = na.unpack_info(pi, N)
    assert torch.equal(ri.cpu(), torch.repeat_interleave(torch.arange(R), counts))
    assert torch.equal(na.pack_info(ri, R), pi)
    assert torch.equal(na.unpack_info(pi.to(torch.int32), N), ri)
    # rendering on unpack_info output needs no pack_info and no read-back of the indices
    ts = torch.rand(N, generator=g).to(dev)
    te = ts + 0.01
    sig = torch.rand(N, generator=g).to(dev)
    rgb = torch.rand(N, 3, generator=g).to(dev)
    ri = na.unpack_info(pi, N)
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    colors, _, _, _ = na.rendering(ts, te, ri, n_rays=R, rgb_sigma_fn=lambda t0, t1, i: (rgb, sig))
    assert "nfa_pack_info" not in calls and calls, calls
    monkeypatch.setattr(B, "call", real)
    colors_ref, _, _, _ = na.rendering(ts, te, ri.clone(), n_rays=R, rgb_sigma_fn=lambda t0, t1, i: (rgb, sig))
    assert torch.equal(colors, colors_ref)


def _occ_samples(dev):
    import nerfacc_amd as na
    rng = np.random.default_rng(4)
    R, res = 2048, 64
    o = torch.from_numpy(rng.standard_normal((R, 3)).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((R, 3)).astype(np.float32)), dim=-1).to(dev)
    est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=res).to(dev)
    b = torch.from_numpy(rng.random((1, res, res, res)) < 0.3).to(dev)
    est.binaries = b
    est.occs = b.reshape(-1).float()
    ri, ts, te = est.sampling(o, d, render_step_size=2 * 3 ** 0.5 / 256)
    assert ri.numel() > 5000
    sig = torch.from_numpy(rng.random(ri.numel()).astype(np.float32) * 20).to(dev)
    return ri, ts, te, sig, R


def test_layout_equivalence_occgrid(dev):
    """render_weight_from_density on packed OccGridEstimator samples, moved to the padded layout, equals the batched op on
    the padded samples (padding has delta = 0, hence alpha = 0 and weight 0)."""
    import nerfacc_amd as na
    ri, ts, te, sig, R = _occ_samples(dev)
    pi = na.pack_info(ri, R)
    w_packed, _, _ = na.render_weight_from_density(ts, te, sig, ray_indices=ri, n_rays=R)
    w_a = na.unpack_data(pi, w_packed)
    pts, pte, psig = (na.unpack_data(pi, t, pad_value=0) for t in (ts, te, sig))
    w_b, _, _ = na.render_weight_from_density(pts, pte, psig)
    assert w_a.shape == w_b.shape == (R, int(pi[:, 1].max()))
    assert (w_a - w_b).abs().max().item() <= 1e-6


def test_roundtrips(dev):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(3)
    counts = torch.randint(0, 30, (1000,), generator=g)
    pi = ragged(counts).to(dev)
    N = int(counts.sum())
    d = torch.randn(N, 5, generator=g).to(dev)
    S = int(counts.max())
    mask = torch.arange(S, device=dev)[None, :] < pi[:, 1:2]
    packed, pi2 = na.pack_data(na.unpack_data(pi, d, S), mask)
    assert torch.equal(packed, d) and torch.equal(pi2, pi)
    # pack_data output flows on: unpack_info takes its packed_info without a check
    assert torch.equal(na.unpack_info(pi2, N), na.unpack_info(pi, N))


def test_pack_data_visibility_mask_propnet(dev):
    import nerfacc_amd as na
    est = na.PropNetEstimator().to(dev)
    n_rays = 1031
    off = torch.linspace(-0.6, 0.6, n_rays, device=dev)[:, None]
    fn = lambda ts, te: torch.exp(-((ts + te) * 0.5 - 4.0 - off) ** 2 * 2.0) * 3.0 + 0.05
    ts, te = est.sampling([fn], [64], 48, n_rays, 2.0, 6.0, sampling_type="uniform")
    sig = fn(ts, te) * 4
    vis = na.render_visibility_from_density(ts, te, sig, early_stop_eps=1e-2, alpha_thre=1e-3)
    assert 0 < vis.sum() < vis.numel()
    for t in (ts, sig, torch.stack([ts, te, sig], -1)):
        packed, pi = na.pack_data(t, vis)
        assert torch.equal(packed, t[vis])
        assert torch.equal(pi[:, 1], vis.sum(1))
    # the survivors render packed
    packed_ts, pi = na.pack_data(ts, vis)
    packed_te, _ = na.pack_data(te, vis)
    packed_sig, _ = na.pack_data(sig, vis)
    w, _, _ = na.render_weight_from_density(packed_ts, packed_te, packed_sig, packed_info=pi)
    assert w.shape == (int(vis.sum()),) and torch.isfinite(w).all()


def test_native_path_taken(dev, monkeypatch):
    import nerfacc_amd as na
    from nerfacc_amd import _backend as B
    from nerfacc_amd import pack
    for name in ("_unpack_info_torch", "_unpack_data_torch", "_pack_data_torch"):
        monkeypatch.setattr(pack, name, lambda *a, _n=name: pytest.fail(f"torch path {_n} taken"))
    pi = ragged([3, 0, 4]).to(dev)
    x = torch.randn(7, 2, device=dev, requires_grad=True)
    mask = torch.rand(3, 4, device=dev) < 0.5
    calls = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    na.unpack_info(pi, 7)
    assert calls[0] == "nfa_fill_ray_indices", calls
    calls.clear()
    na.unpack_data(pi, x, 4).sum().backward()
    assert calls == ["nfa_unpack_rows", "nfa_pack_rows"], calls
    calls.clear()
    y = torch.randn(3, 4, 2, device=dev, requires_grad=True)
    na.pack_data(y, mask)[0].sum().backward()
    assert calls[:3] == ["nfa_mask_row_counts", "nfa_exclusive_cumsum_pairs_i64", "nfa_pack_rows"], calls
    assert calls[-1] == "nfa_unpack_rows", calls


def test_foreign_packed_info_checked_before_launch(dev, monkeypatch):
    import nerfacc_amd as na
    from nerfacc_amd import _backend as B
    monkeypatch.setattr(B, "call", lambda name, *a: pytest.fail(f"{name} launched on bad input"))
    data = torch.zeros(10, 3, device=dev)
    for bad in ([[0, 4], [4, 7]], [[-2, 3]], [[0, -1]], [[0, 5], [3, 2]]):
        with pytest.raises(ValueError):
            na.unpack_data(torch.tensor(bad, device=dev), data)
    with pytest.raises(ValueError):
        na.unpack_info(torch.tensor([[0, 4], [5, 5]], device=dev), 10)
