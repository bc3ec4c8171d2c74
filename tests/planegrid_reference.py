"""The K-Planes form of the plane grid, written from the paper's definition with ``torch.nn.functional.grid_sample``, in
float64: the reference of tests/test_planegrid_cpu.py and tests/test_planegrid_gpu.py.

``interpolate_ms_features`` with ``concat_features=True`` (Fridovich-Keil et al. 2023): per scale, every plane ``(a, b)``,
``a < b``, of ``itertools.combinations(range(D), 2)`` is a ``[1, F, R_b, R_a]`` image sampled bilinearly at
``(u_a, u_b)``, ``u = 2 x - 1``, with ``align_corners=True`` and ``padding_mode="border"``; the samples of a scale are
multiplied (or added), and the scales concatenated.  Nothing here is shared with nerfacc_amd/encodings.py except the
parameter layout, which is the documented one: scale-major, then plane order, each plane row-major ``[R_b, R_a, F]``.
"""
import itertools

import torch
import torch.nn.functional as TF


# the resolutions of the tests: non-square on purpose (an a / b swap or a scaled time axis changes a shape or a value)
RES = {3: (5, 7, 4), 4: (5, 7, 4, 3)}
MS = (1, 2)


def edge_points(D):
    """Rows whose axis 0 (and, in the last three rows, every axis) is a border, outside, infinite or NaN; the other axes
    inside.  Rows 0..2: on the borders (0, 1, -0); 3..9: outside or not finite; 10..12: all NaN, all inf, all -inf."""
    inf, nan = float("inf"), float("nan")
    vals = [0.0, 1.0, -0.0, -0.3, 1.7, -1e30, 1e30, inf, -inf, nan]
    x = torch.full((len(vals) + 3, D), 0.37)
    for r, v in enumerate(vals):
        x[r, 0] = v
    x[len(vals)] = nan
    x[len(vals) + 1] = inf
    x[len(vals) + 2] = -inf
    return x


def scale_resolutions(resolution, multiscale_res):
    """R_{s,d}: the three spatial axes are multiplied by the scale's factor, the time axis (3) is not."""
    return [[r * m if d < 3 else r for d, r in enumerate(resolution)] for m in multiscale_res]


def split_planes(params, resolution, multiscale_res, n_features):
    """[[the [1, F, R_b, R_a] image of plane k of scale s]] as views of the flat table (any dtype)."""
    D = len(resolution)
    out, at = [], 0
    for res in scale_resolutions(resolution, multiscale_res):
        row = []
        for a, b in itertools.combinations(range(D), 2):
            n = res[a] * res[b] * n_features
            row.append(params[at: at + n].view(res[b], res[a], n_features).permute(2, 0, 1)[None])
            at += n
        out.append(row)
    assert at == params.numel()
    return out


def planegrid_reference(x, params, resolution, multiscale_res, n_features, reduce="product"):
    """x [N, D] in [0, 1] (any value is legal), params flat; both are taken to float64.  Differentiable by autograd."""
    x, params = x.double(), params.double()
    D = len(resolution)
    u = 2.0 * x - 1.0
    outs = []
    for planes in split_planes(params, resolution, multiscale_res, n_features):
        acc = None
        for img, (a, b) in zip(planes, itertools.combinations(range(D), 2)):
            grid = torch.stack([u[:, a], u[:, b]], -1)[None, None]            # [1, 1, N, 2]: (x -> W = R_a, y -> H = R_b)
            v = TF.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].t()  # [N, F]
            acc = v if acc is None else (acc * v if reduce == "product" else acc + v)
        outs.append(acc)
    return torch.cat(outs, -1)


def off_node_points(n, resolution, multiscale_res, seed, lo=0.0, hi=1.0, margin=1e-3):
    """n float32 points uniform in [lo, hi]^D none of whose coordinates lies within ``margin`` (in node units) of a grid
    node of any scale, nor of the borders 0 and 1: where the bilinear sample has one derivative."""
    g = torch.Generator().manual_seed(seed)
    D = len(resolution)
    x = torch.rand(4 * n + 64, D, generator=g) * (hi - lo) + lo
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for res in scale_resolutions(resolution, multiscale_res):
        for d in range(D):
            p = x[:, d].double() * (res[d] - 1)
            ok &= (p - p.round()).abs() > margin
    x = x[ok][:n]
    assert x.shape[0] == n
    return x.contiguous()
