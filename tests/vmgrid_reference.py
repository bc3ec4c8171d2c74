"""TensoRF's vector-matrix grid the way ``TensorVMSplit`` writes it (Chen et al. 2022), with
``torch.nn.functional.grid_sample`` and ``F.interpolate`` in float64: the reference of tests/test_vmgrid_cpu.py and
tests/test_vmgrid_gpu.py.

Per mode ``m`` the plane is a ``[1, C, R_b, R_a]`` image over the axes ``matMode[m] = (a, b)`` and the line a
``[1, C, R_c, 1]`` image along ``vecMode[m] = c``; both are sampled bilinearly at ``u = 2 x - 1`` with
``align_corners=True`` (the line at ``(0, u_c)``, as ``coordinate_line`` stacks it) and multiplied.  The products are
concatenated over the modes (``compute_appfeature`` before ``basis_mat``) or summed over modes and components
(``compute_densityfeature``).  ``up_sampling_VM`` is ``F.interpolate(mode="bilinear", align_corners=True)`` of every plane
and line.  ``padding_mode="border"`` is this project's rule outside the box (TensoRF's zeros differ there only).  Nothing
here is shared with nerfacc_amd/encodings.py except the documented parameter layout: per mode the plane, row-major
``[R_b, R_a, C]``, then the line ``[R_c, C]``.
"""
import torch
import torch.nn.functional as TF

from planegrid_reference import off_node_points as _off_node_points

MAT_MODE = ((0, 1), (0, 2), (1, 2))
VEC_MODE = (2, 1, 0)

# the resolutions of the tests: all axes different on purpose (a swap of axes changes a shape or a value)
RES_SMALL, RES_WIDE = (7, 6, 5), (33, 20, 9)


def off_node_points(n, resolution, seed, lo=0.0, hi=1.0):
    return _off_node_points(n, resolution, (1,), seed, lo, hi)


def split(params, resolution, n_components):
    """([the [1, C, R_b, R_a] plane of mode m], [the [1, C, R_c, 1] line of mode m]) as views of the flat table."""
    C, planes, lines, at = n_components, [], [], 0
    for (a, b), c in zip(MAT_MODE, VEC_MODE):
        n = resolution[a] * resolution[b] * C
        planes.append(params[at: at + n].view(resolution[b], resolution[a], C).permute(2, 0, 1)[None])
        at += n
        n = resolution[c] * C
        lines.append(params[at: at + n].view(resolution[c], C).t()[None, :, :, None])
        at += n
    assert at == params.numel()
    return planes, lines


def vmgrid_reference(x, params, resolution, n_components, reduce="concat"):
    """x [N, 3] in [0, 1] (any value is legal), params flat; both are taken to float64.  Differentiable by autograd."""
    x, params = x.double(), params.double()
    u = 2.0 * x - 1.0
    planes, lines = split(params, resolution, n_components)
    kw = dict(mode="bilinear", padding_mode="border", align_corners=True)
    terms = []
    for plane, line, (a, b), c in zip(planes, lines, MAT_MODE, VEC_MODE):
        coordinate_plane = torch.stack([u[:, a], u[:, b]], -1)[None, None]                       # [1, 1, N, 2]
        coordinate_line = torch.stack([torch.zeros_like(u[:, c]), u[:, c]], -1)[None, None]
        pv = TF.grid_sample(plane, coordinate_plane, **kw)[0, :, 0]                               # [C, N]
        lv = TF.grid_sample(line, coordinate_line, **kw)[0, :, 0]
        terms.append(pv * lv)
    if reduce == "concat":
        return torch.cat(terms, 0).t()
    return torch.cat(terms, 0).sum(0)[:, None]


def resample_reference(params, resolution, new_resolution, n_components):
    """``up_sampling_VM`` in float64: the flat table at ``new_resolution``."""
    planes, lines = split(params.double(), resolution, n_components)
    out = []
    for plane, line, (a, b), c in zip(planes, lines, MAT_MODE, VEC_MODE):
        p = TF.interpolate(plane, size=(new_resolution[b], new_resolution[a]), mode="bilinear", align_corners=True)
        q = TF.interpolate(line, size=(new_resolution[c], 1), mode="bilinear", align_corners=True)
        out += [p[0].permute(1, 2, 0).reshape(-1), q[0, :, :, 0].t().reshape(-1)]
    return torch.cat(out)
