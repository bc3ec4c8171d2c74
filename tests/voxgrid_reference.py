"""A dense voxel grid the way DVGO and TiNeuVox write it (Sun et al. 2022; Fang et al. 2022), with
``torch.nn.functional.grid_sample`` and ``F.interpolate`` in float64: the reference of tests/test_voxgrid_cpu.py and
tests/test_voxgrid_gpu.py.

The grid is a ``[1, C, N_x, N_y, N_z]`` tensor; a point ``x`` in [0, 1]^3 is sampled at ``u = 2 x - 1`` with the coordinates
flipped to ``(u_z, u_y, u_x)`` (``grid_sample`` takes them in the order W, H, D), ``mode="bilinear"`` and
``align_corners=True``.  TiNeuVox's ``mult_dist_interp`` samples the views ``grid[:, :, ::s, ::s, ::s]`` as well and
concatenates.  ``scale_volume_grid`` is ``F.interpolate(mode="trilinear", align_corners=True)``.  ``padding_mode="border"`` is
this project's rule outside the box (zeros differ there only).  Nothing here is shared with nerfacc_amd/encodings.py except
the documented parameter layout: one row-major ``[R_z, R_y, R_x, C]`` block.
"""
import torch
import torch.nn.functional as TF

from planegrid_reference import edge_points  # noqa: F401  (the edge rows of the tests)

# the resolutions of the tests: all axes different on purpose (a swap of axes changes a shape or a value)
RES_SMALL, RES_TINY, RES_ODD, RES_WIDE = (5, 4, 7), (2, 2, 2), (6, 7, 9), (33, 17, 65)


def dvgo_grid(params, resolution, n_features):
    """The ``[1, C, N_x, N_y, N_z]`` tensor as a view of the flat table."""
    Rx, Ry, Rz = resolution
    return params.view(Rz, Ry, Rx, n_features).permute(3, 2, 1, 0)[None]


def voxgrid_reference(x, params, resolution, n_features, strides=(1,)):
    """x [N, 3] in [0, 1] (any finite value is legal), params flat; both are taken to float64.  Differentiable by autograd."""
    x, params = x.double(), params.double()
    grid = dvgo_grid(params, resolution, n_features)
    ind_norm = (2.0 * x - 1.0).flip(-1)[None, None, None]                                      # [1, 1, 1, N, 3], (z, y, x)
    outs = []
    for s in strides:
        v = TF.grid_sample(grid[:, :, ::s, ::s, ::s], ind_norm, mode="bilinear", padding_mode="border", align_corners=True)
        outs.append(v[0, :, 0, 0].t())                                                         # [N, C]
    return torch.cat(outs, -1)


def resample_reference(params, resolution, new_resolution, n_features):
    """``scale_volume_grid`` in float64: the flat table at ``new_resolution``."""
    grid = dvgo_grid(params.double(), resolution, n_features)
    new = TF.interpolate(grid, size=tuple(new_resolution), mode="trilinear", align_corners=True)
    return new[0].permute(3, 2, 1, 0).reshape(-1)


def stride_nodes(resolution, strides):
    """Nodes per axis of every stride: ceil(R / s)."""
    return [[-(-r // s) for r in resolution] for s in strides]


def off_node_points(n, resolution, strides, seed, lo=0.0, hi=1.0, margin=1e-3):
    """n float32 points uniform in [lo, hi]^3 none of whose coordinates lies within ``margin`` (in node units) of a node of
    any stride, nor of the borders 0 and 1: where the trilinear sample has one derivative."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(6 * n + 64, 3, generator=g) * (hi - lo) + lo
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for nodes in stride_nodes(resolution, strides):
        for d in range(3):
            p = x[:, d].double() * (nodes[d] - 1)
            ok &= (p - p.round()).abs() > margin
    x = x[ok][:n]
    assert x.shape[0] == n
    return x.contiguous()


def edge_rows(resolution):
    """planegrid_reference.edge_points (rows 0..2 on the borders, 3..9 outside or not finite on axis 0, 10..12 all NaN / inf /
    -inf) and rows on exact nodes."""
    r = resolution
    nodes = torch.tensor([[i / (r[0] - 1), j / (r[1] - 1), k / (r[2] - 1)]
                          for i, j, k in [(0, 0, 0), (1, 1, 1), (r[0] - 1, r[1] - 1, r[2] - 1), (1, 0, r[2] - 1)]])
    return torch.cat([edge_points(3), nodes, torch.tensor([[0.5, 0.2, 0.25], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])])
