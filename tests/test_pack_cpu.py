"""CPU: nerfacc_amd.unpack_info / unpack_data / pack_data (nerfacc 0.3's layout conversions) -- the names, the torch path
against a float64 Python-loop restatement, input checks, and the C ABI's argument checks of nfa_{unpack,pack}_rows and
nfa_mask_row_counts."""
import ctypes

import pytest
import torch


def loop_unpack(pi, data, S, pad):
    """float64 restatement, one sample at a time."""
    R = pi.shape[0]
    out = torch.full((R, S, *data.shape[1:]), float(pad), dtype=torch.float64)
    for r in range(R):
        start, cnt = int(pi[r, 0]), int(pi[r, 1])
        for s in range(min(cnt, S)):
            out[r, s] = data[start + s].to(torch.float64)
    return out


def loop_pack(data, mask):
    rows, info = [], []
    for r in range(mask.shape[0]):
        info.append([len(rows), int(mask[r].sum())])
        rows += [data[r, s].to(torch.float64) for s in range(mask.shape[1]) if mask[r, s]]
    packed = torch.stack(rows) if rows else torch.zeros((0, *data.shape[2:]), dtype=torch.float64)
    return packed, torch.tensor(info, dtype=torch.int64).view(-1, 2)


def ragged_info(counts):
    counts = torch.as_tensor(counts, dtype=torch.int64)
    return torch.stack([torch.cumsum(counts, 0) - counts, counts], dim=-1)


def test_names_exported_not_in_all():
    import nerfacc_amd as na
    for name in ("unpack_info", "unpack_data", "pack_data"):
        assert callable(getattr(na, name))
        assert name not in na.__all__
    assert len(na.__all__) == 22


def test_unpack_info_cpu():
    import nerfacc_amd as na
    pi = ragged_info([2, 0, 3, 1, 0])
    ri = na.unpack_info(pi, 6)
    assert ri.dtype == torch.int64 and ri.tolist() == [0, 0, 2, 2, 2, 3]
    assert na.unpack_info(pi.to(torch.int32), 6).tolist() == ri.tolist()
    assert na.unpack_info(torch.zeros((0, 2), dtype=torch.int64), 0).numel() == 0
    for bad, n in ((pi, 7), (torch.tensor([[1, 2], [3, 3]]), 6), (torch.tensor([[3, 3], [0, 3]]), 6),
                   (torch.tensor([[0, 3], [2, 4]]), 6), (torch.tensor([[0, -1], [0, 1]]), 0)):
        with pytest.raises(ValueError):
            na.unpack_info(bad, n)


@pytest.mark.parametrize("D", [1, 3, 7])
@pytest.mark.parametrize("S", [None, 2, 9])
@pytest.mark.parametrize("pad", [0, -2.5])
def test_unpack_data_cpu_matches_loop(D, S, pad):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(D * 10 + (S or 0))
    counts = torch.randint(0, 7, (11,), generator=g)
    counts[3] = 0
    pi = ragged_info(counts)
    N = int(counts.sum())
    data = torch.randn(N, D, generator=g, dtype=torch.float64)
    out = na.unpack_data(pi, data, S, pad_value=pad)
    S_eff = int(counts.max()) if S is None else S
    assert out.shape == (11, S_eff, D)
    assert torch.equal(out, loop_unpack(pi, data, S_eff, pad))
    # 1-D data gives (n_rays, S)
    out1 = na.unpack_data(pi, data[:, 0], S, pad_value=pad)
    assert torch.equal(out1, loop_unpack(pi, data[:, :1], S_eff, pad)[..., 0])


def test_unpack_data_cpu_gaps_and_order():
    import nerfacc_amd as na
    data = torch.arange(20, dtype=torch.float64).view(10, 2)
    pi = torch.tensor([[7, 2], [0, 3], [4, 0], [5, 1]])     # gaps at 3, 4, 6, 9; out of order
    out = na.unpack_data(pi, data, 3, pad_value=1.5)
    assert torch.equal(out, loop_unpack(pi, data, 3, 1.5))
    x = data.clone().requires_grad_(True)
    na.unpack_data(pi, x, 2).sum().backward()
    covered = torch.tensor([1, 1, 0, 0, 0, 1, 0, 1, 1, 0], dtype=torch.float64)   # ray 1's third sample is dropped
    assert torch.equal(x.grad, covered[:, None].expand(10, 2))


def test_unpack_data_rejects_bad_packed_info():
    import nerfacc_amd as na
    data = torch.zeros(6, 2)
    for bad in (torch.tensor([[0, 3], [3, 4]]), torch.tensor([[-1, 2]]), torch.tensor([[0, -1]]),
                torch.tensor([[0, 3], [2, 2]])):   # the last overlaps
        with pytest.raises(ValueError):
            na.unpack_data(bad, data)
    with pytest.raises(ValueError):
        na.unpack_data(torch.zeros(3, 3, dtype=torch.int64), data)


@pytest.mark.parametrize("D", [None, 1, 3, 7])
def test_pack_data_cpu_random_masks(D):
    import nerfacc_amd as na
    g = torch.Generator().manual_seed(7 + (D or 0))
    R, S = 13, 10
    shape = (R, S) if D is None else (R, S, D)
    data = torch.randn(*shape, generator=g, dtype=torch.float64)
    mask = torch.rand(R, S, generator=g) < 0.4
    mask[2] = False
    mask[5] = True
    packed, pi = na.pack_data(data, mask)
    ref, ref_pi = loop_pack(data if D is not None else data[..., None], mask)
    assert pi.dtype == torch.int64 and torch.equal(pi, ref_pi)
    assert torch.equal(packed, ref if D is not None else ref[:, 0])
    # gradient: ones where the mask is set
    x = data.clone().requires_grad_(True)
    na.pack_data(x, mask)[0].sum().backward()
    assert torch.equal(x.grad, mask.to(torch.float64).view(R, S, *([1] if D else [])).expand(shape))


def test_roundtrip_cpu():
    import nerfacc_amd as na
    counts = torch.tensor([3, 0, 5, 1])
    pi = ragged_info(counts)
    data = torch.randn(9, 4, dtype=torch.float64)
    padded = na.unpack_data(pi, data)
    mask = torch.arange(5)[None, :] < counts[:, None]
    packed, pi2 = na.pack_data(padded, mask)
    assert torch.equal(packed, data) and torch.equal(pi2, pi)
    assert torch.equal(na.unpack_info(pi2, 9), torch.repeat_interleave(torch.arange(4), counts))


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # never dereferenced: every case below is decided on the host before a launch


def test_pack_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    pad = ctypes.create_string_buffer(16)
    padp = ctypes.addressof(pad)
    # nfa_unpack_rows(packed, packed_info, mask, n_rays, n_per_ray, n_packed, row_bytes, pad_host, pad_bytes, padded, stream)
    unpack = [
        ((P, P, None, -1, 4, 4, 4, None, 0, P, None), "unpack_rows: negative size"),
        ((P, P, None, 2, -4, 4, 4, None, 0, P, None), "unpack_rows: negative size"),
        ((P, P, None, 2, 4, -1, 4, None, 0, P, None), "unpack_rows: negative size"),
        ((P, P, None, 2, 4, 4, 0, None, 0, P, None), "unpack_rows: row_bytes must be >= 1"),
        ((P, P, None, 2, 4, 4, 4, padp, 3, P, None), "unpack_rows: pad_bytes must be 0, or 1, 2, 4, 8 or 16 with pad_host set"),
        ((P, P, None, 2, 4, 4, 4, None, 4, P, None), "unpack_rows: pad_bytes must be 0, or 1, 2, 4, 8 or 16 with pad_host set"),
        ((P, None, None, 2, 4, 4, 4, None, 0, P, None), "unpack_rows: null pointer"),
        ((P, P, None, 2, 4, 4, 4, None, 0, None, None), "unpack_rows: null pointer"),
        ((None, P, None, 2, 4, 4, 4, None, 0, P, None), "unpack_rows: null pointer"),
        ((P + 1, P, None, 2, 1 << 31, 4, 1, None, 0, P, None), "unpack_rows: a padded row of 2^31 or more 1-byte chunks"),
        ((None, None, None, 0, 4, 4, 4, None, 0, None, None), None),   # no rays: nothing to do
        ((None, None, None, 2, 0, 4, 4, None, 0, None, None), None),   # no slots: nothing to do
    ]
    # nfa_pack_rows(padded, packed_info, mask, n_rays, n_per_ray, n_packed, row_bytes, packed, stream)
    pack = [
        ((P, P, P, -1, 4, 4, 4, P, None), "pack_rows: negative size"),
        ((P, P, P, 2, 4, 4, -4, P, None), "pack_rows: row_bytes must be >= 1"),
        ((None, P, P, 2, 4, 4, 4, P, None), "pack_rows: null pointer"),
        ((P, P, P, 2, 4, 4, 4, None, None), "pack_rows: null pointer"),
        ((P, None, P, 2, 4, 4, 4, P, None), "pack_rows: null pointer"),
        ((None, None, None, 2, 4, 0, 4, None, None), None),   # no packed rows: nothing to write
    ]
    counts = [
        ((P, -1, 4, P, None), "mask_row_counts: negative size"),
        ((P, 2, -4, P, None), "mask_row_counts: negative size"),
        ((P, 2, 4, None, None), "mask_row_counts: null pointer"),
        ((None, 2, 4, P, None), "mask_row_counts: null pointer"),
        ((None, 0, 4, None, None), None),
    ]
    for fn, cases in (("nfa_unpack_rows", unpack), ("nfa_pack_rows", pack), ("nfa_mask_row_counts", counts)):
        for args, msg in cases:
            assert len(args) == len(B._SIGS[fn])
            lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
            rc = getattr(lib, fn)(*args)
            if msg is None:
                assert rc == 0, (fn, args, rc, lib.nfa_last_error())
            else:
                assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, args, rc, lib.nfa_last_error())
