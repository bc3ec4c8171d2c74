"""The reference's Instant-NGP fields (ref: examples/radiance_fields/ngp.py: ``NGPRadianceField``, ``NGPDensityField``) on the
native encodings and networks of this package, with the no-grad query fused into one launch (csrc/ngp_field.hip).

Both classes are compositions of :class:`~nerfacc_amd.encodings.HashGridEncoding` (half ``out_dtype``),
:class:`~nerfacc_amd.mlp.FusedMLP` and :class:`~nerfacc_amd.encodings.SphericalHarmonicsEncoding`, so parameters, the state
dict and :class:`~nerfacc_amd.optim.FusedAdam` work as for those modules.  With grad enabled and something that requires it
a query runs those native passes in their usual order (the *composed chain*).  Under ``torch.no_grad()``, or when nothing
requires grad -- ``OccGridEstimator.sampling(sigma_fn=...)``, ``update_every_n_steps``, the test-mode loop -- a supported
configuration takes ONE launch instead: normalise / contract, hash grid, base network, harmonics, head network and the
activations, with nothing between them in memory.  Everything the fused launch does not serve (see ``fused_supported``)
takes the composed chain instead of raising.  (``NGPRadianceField.forward`` without view directions raises ``ValueError``
on either path: the reference fails there too, with an unbound ``rgb``.)  The base network's outputs (raw density, geometry
feature) are the composed chain's bits; the raw colour may differ from it in the last bit of a float32 sum (the head's second k-step is summed in
another order).

Differences from the reference, all in what cannot be expressed natively: ``density_activation`` is a name of
:data:`nerfacc_amd.rawrender.DENSITY_ACTIVATIONS` with ``density_bias`` (default ``"trunc_exp"``, ``-1.0``: the reference's
``trunc_exp(x - 1)``); a callable is accepted and always takes the composed chain.  The geometry feature that
``query_density(return_feat=True)`` returns stays in the networks' ``dtype``.  Outside the box the density is an exact zero
(a select, as :func:`nerfacc_amd.rawrender.activate_density`).

Not part of ``nerfacc_amd.__all__``: ``from nerfacc_amd.fields import NGPRadianceField, NGPDensityField``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, List, Optional, Union

import torch
from torch import Tensor, nn

from . import _backend as B
from .encodings import HashGridEncoding, SphericalHarmonicsEncoding
from .mlp import FusedMLP, image_elems
from .rawrender import DENSITY_ACTIVATIONS, activate_density
from .samples import _contract_torch, sample_positions

FUSED_MAX_LEVELS = 16


class _NGPField(nn.Module):
    """What the two fields share: the box, the grid, the base network and the fused launch."""

    def __init__(self, aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, geo_feat_dim,
                 n_levels, log2_hashmap_size, dtype, interpolation, fused):
        super().__init__()
        if not isinstance(aabb, Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32)
        self.register_buffer("aabb", aabb.to(torch.float32).reshape(-1))
        if not callable(density_activation) and density_activation not in DENSITY_ACTIVATIONS:
            raise ValueError(f"density_activation {density_activation!r}: one of {', '.join(DENSITY_ACTIVATIONS)} or a callable")
        self.num_dim, self.unbounded = int(num_dim), bool(unbounded)
        self.density_activation, self.density_bias = density_activation, float(density_bias)
        self.base_resolution, self.max_resolution = base_resolution, max_resolution
        self.geo_feat_dim, self.n_levels, self.log2_hashmap_size = int(geo_feat_dim), int(n_levels), int(log2_hashmap_size)
        self.dtype, self.fused = dtype, bool(fused)
        per_level_scale = math.exp((math.log(max_resolution) - math.log(base_resolution)) / (n_levels - 1)) if n_levels > 1 else 1.0
        self.encoding = HashGridEncoding(self.num_dim, n_levels, 2, log2_hashmap_size, base_resolution, per_level_scale, out_dtype=dtype,
                                         interpolation=interpolation)
        self.mlp_base = FusedMLP(2 * self.n_levels, 1 + self.geo_feat_dim, 64, 1, dtype=dtype)
        self._head_packed = None   # (key, image)

    # ---------------------------------------------------------------- the composed chain

    def _normalise(self, x: Tensor):
        lo, hi = self.aabb[: self.num_dim].to(x), self.aabb[self.num_dim:].to(x)
        x = (x - lo) / (hi - lo)
        if self.unbounded:
            x = _contract_torch(x, 1)
        return x, ((x > 0.0) & (x < 1.0)).all(dim=-1)

    def _activate(self, raw: Tensor, selector: Tensor) -> Tensor:
        if callable(self.density_activation):
            return self.density_activation(raw) * selector[..., None]
        return activate_density(raw, self.density_activation, self.density_bias, selector[..., None])

    def _base(self, positions: Tensor):
        """(raw density [..., 1] float32, feature [..., G] in ``dtype``, selector [...]) by the native passes in their order."""
        x, selector = self._normalise(positions)
        out = self.mlp_base(self.encoding(x.reshape(-1, self.num_dim))).view(*positions.shape[:-1], 1 + self.geo_feat_dim)
        return out[..., :1].to(positions.dtype), out[..., 1:], selector

    # ---------------------------------------------------------------- the fused launch

    def fused_supported(self, full: bool) -> bool:
        """The configurations csrc/ngp_field.hip serves: 3-D, at most 16 levels, a named density activation, and for the full
        query view directions with a geometry feature of 1..15."""
        ok = self.num_dim == 3 and self.n_levels <= FUSED_MAX_LEVELS and not callable(self.density_activation) and self.geo_feat_dim <= 15
        return ok and (not full or (getattr(self, "use_viewdirs", False) and self.geo_feat_dim >= 1))

    def _use_fused(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        if not (self.fused and self.fused_supported(full)):
            return False
        ts = [t for t in tensors if t is not None]
        if not all(t.is_cuda and t.device == self.encoding.params.device for t in ts) or not all(t.dtype == torch.float32 for t in ts[:4]):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in [*self.parameters(), *ts]))

    def _head_image(self) -> Tensor:
        """The head's forward image in the fused launch's k order, rebuilt when the masters change (as FusedMLP's images)."""
        p = self.mlp_head.params
        key = (p.data_ptr(), p._version, p.device)
        if self._head_packed is None or self._head_packed[0] != key:
            img = torch.empty(image_elems(16 + self.geo_feat_dim, 3, 64, 2)[0], dtype=self.dtype, device=p.device)
            with torch.cuda.device(p.device):
                B.call("nfa_ngp_pack_head", B.ELEM_CODES[self.dtype], B.ptr(p), self.geo_feat_dim, B.ptr(img), img.numel(), B.stream())
            self._head_packed = (key, img)
        return self._head_packed[1]

    def _launch(self, full: bool, n: int, shape, want: List[str], positions=None, dirs=None, rays=None, rgb_dtype=torch.float32,
                outputs: Optional[dict] = None):
        """One fused launch; returns the outputs named in ``want`` (sigma, density, selector, feat, rgb, rgb_act), shaped ``shape``
        (``outputs``: the caller's own contiguous tensors for them)."""
        dev, enc, t = self.encoding.params.device, self.encoding, self.encoding.table
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
        grid = B.NGPGrid(B.ptr(enc.params), enc.params.numel(), enc.n_levels, 2, t.log2_hashmap_size, enc.interp, vp(t.c_scales), vp(t.c_res),
                         vp(t.c_sizes))
        keep = [x.contiguous() for x in (rays[:5] if rays is not None else (positions, dirs)) if x is not None]
        if rays is not None:
            ri = keep[4] if keep[4].dtype == torch.int64 else keep[4].to(torch.int64)
            keep[4] = ri
            inp = B.NGPInput(None, None, *[B.ptr(x) for x in keep], keep[0].shape[0])
        else:
            inp = B.NGPInput(B.ptr(keep[0]), B.ptr(keep[1]) if full else None, None, None, None, None, None, 0)
        specs = {"sigma": ((1,), torch.float32), "density": ((1,), torch.float32), "selector": ((), torch.bool),
                 "feat": ((self.geo_feat_dim,), self.dtype), "rgb": ((3,), rgb_dtype), "rgb_act": ((3,), torch.float32)}
        out = dict.fromkeys(specs)
        for k in want:
            tail, dtype = specs[k]
            out[k] = outputs[k] if outputs is not None else torch.empty(*shape, *tail, dtype=dtype, device=dev)
        if n == 0:
            return out
        act = DENSITY_ACTIVATIONS[self.density_activation]
        box = (None, B.ptr(self.aabb)) if self.aabb.is_cuda else ((ctypes.c_float * 6)(*self.aabb.tolist()), None)
        lead = (B.ELEM_CODES[self.dtype], ctypes.byref(grid), B.ptr(self.mlp_base._images(self.mlp_base.params)[0]))
        tail = (self.geo_feat_dim, ctypes.byref(inp), n, *box, int(self.unbounded), act, self.density_bias, B.ptr(out["sigma"]),
                B.ELEM_CODES[torch.float32])
        with torch.cuda.device(dev):
            if full:
                B.call("nfa_ngp_field", *lead, B.ptr(self._head_image()), *tail, B.ptr(out["rgb"]), B.ELEM_CODES[rgb_dtype],
                       B.ptr(out["density"]), B.ptr(out["selector"]), B.ptr(out["rgb_act"]), B.stream())
            else:
                B.call("nfa_ngp_density", *lead, *tail, B.ptr(out["density"]), B.ptr(out["selector"]), B.ptr(out["feat"]), B.stream())
        return out

    def density_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor) -> Tensor:
        """Densities ``[n]`` at the midpoints of packed ray samples: a trainer's ``sigma_fn``."""
        if self._use_fused(False, rays_o, rays_d, t_starts, t_ends, ray_indices):
            n = t_starts.numel()
            return self._launch(False, n, (n,), ["density"], rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))["density"].view(n)
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices)
        raw, _, selector = self._base(s.positions)
        return self._activate(raw, selector).squeeze(-1)


class NGPRadianceField(_NGPField):
    """Instant-NGP radiance field (the reference's constructor arguments; ``dtype`` fp16 or bf16 is the networks' type,
    ``interpolation`` the hash grid's, ``fused=False`` switches the fused dispatch off)."""

    def __init__(self, aabb: Union[Tensor, List[float]], num_dim: int = 3, use_viewdirs: bool = True,
                 density_activation: Union[str, Callable] = "trunc_exp", unbounded: bool = False, base_resolution: int = 16,
                 max_resolution: int = 4096, geo_feat_dim: int = 15, n_levels: int = 16, log2_hashmap_size: int = 19, *,
                 density_bias: float = -1.0, dtype: torch.dtype = torch.float16, interpolation: str = "Linear", fused: bool = True):
        super().__init__(aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, geo_feat_dim,
                         n_levels, log2_hashmap_size, dtype, interpolation, fused)
        self.use_viewdirs = bool(use_viewdirs)
        if self.use_viewdirs:
            self.direction_encoding = SphericalHarmonicsEncoding(3, 4, out_dtype=dtype)
        if self.geo_feat_dim > 0:
            self.mlp_head = FusedMLP((16 if self.use_viewdirs else 0) + self.geo_feat_dim, 3, 64, 2, dtype=dtype)

    def query_density(self, x: Tensor, return_feat: bool = False):
        if self._use_fused(False, x):
            want = ["density"] + (["feat"] if return_feat and self.geo_feat_dim else [])
            out = self._launch(False, x.numel() // 3, x.shape[:-1], want, positions=x.reshape(-1, 3))
            density, feat = out["density"], out["feat"]
            if return_feat and feat is None:
                feat = torch.empty(*x.shape[:-1], 0, dtype=self.dtype, device=x.device)
        else:
            raw, feat, selector = self._base(x)
            density = self._activate(raw, selector)
        return (density, feat) if return_feat else density

    def _query_rgb(self, dir: Tensor, embedding: Tensor, apply_act: bool = True) -> Tensor:
        h = embedding.reshape(-1, self.geo_feat_dim).to(self.dtype)
        if self.use_viewdirs:
            d = self.direction_encoding(((dir + 1.0) / 2.0).reshape(-1, dir.shape[-1]))
            h = torch.cat([d, h], dim=-1)
        rgb = self.mlp_head(h.contiguous()).reshape(*embedding.shape[:-1], 3).to(torch.float32)
        return torch.sigmoid(rgb) if apply_act else rgb

    def forward(self, positions: Tensor, directions: Optional[Tensor] = None):
        if not (self.use_viewdirs and directions is not None):
            raise ValueError("NGPRadianceField.forward needs view directions (use_viewdirs=True); query_density takes positions alone")
        assert positions.shape == directions.shape, f"{positions.shape} v.s. {directions.shape}"
        if self._use_fused(True, positions, directions):
            out = self._launch(True, positions.numel() // 3, positions.shape[:-1], ["rgb_act", "density"],
                               positions=positions.reshape(-1, 3), dirs=directions.reshape(-1, 3))
            return out["rgb_act"], out["density"]
        density, embedding = self.query_density(positions, return_feat=True)
        return self._query_rgb(directions, embedding), density

    def query_raw(self, positions: Tensor, directions: Tensor):
        """``(raw_rgbs [..., 3], raw_sigmas [...], selector [...])`` at world positions, before any activation."""
        if self._use_fused(True, positions, directions):
            out = self._launch(True, positions.numel() // 3, positions.shape[:-1], ["rgb", "sigma", "selector"],
                               positions=positions.reshape(-1, 3), dirs=directions.reshape(-1, 3))
            return out["rgb"], out["sigma"].squeeze(-1), out["selector"]
        raw_sigma, embedding, selector = self._base(positions)
        return self._query_rgb(directions, embedding, apply_act=False), raw_sigma.squeeze(-1), selector

    def query_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, raw: bool = True):
        """The field at the midpoints of packed ray samples.  ``raw=True``: ``(raw_rgbs [n, 3], raw_sigmas [n], selector [n])``,
        what :func:`nerfacc_amd.rendering_from_raw` takes; otherwise ``(rgbs [n, 3], sigmas [n])`` activated."""
        n = t_starts.numel()
        if self._use_fused(True, rays_o, rays_d, t_starts, t_ends, ray_indices):
            want = ["rgb", "sigma", "selector"] if raw else ["rgb_act", "density"]
            out = self._launch(True, n, (n,), want, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))
            return (out["rgb"], out["sigma"].view(n), out["selector"]) if raw else (out["rgb_act"], out["density"].view(n))
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="raw")
        raw_sigma, embedding, selector = self._base(s.positions)
        rgb = self._query_rgb(s.dirs, embedding, apply_act=not raw)
        return (rgb, raw_sigma.squeeze(-1), selector) if raw else (rgb, self._activate(raw_sigma, selector).squeeze(-1))


class NGPDensityField(_NGPField):
    """Instant-NGP density field for resampling (the reference's constructor arguments; ``dtype``, ``interpolation`` and
    ``fused`` as for :class:`NGPRadianceField`)."""

    def __init__(self, aabb: Union[Tensor, List[float]], num_dim: int = 3, density_activation: Union[str, Callable] = "trunc_exp",
                 unbounded: bool = False, base_resolution: int = 16, max_resolution: int = 128, n_levels: int = 5,
                 log2_hashmap_size: int = 17, *, density_bias: float = -1.0, dtype: torch.dtype = torch.float16,
                 interpolation: str = "Linear", fused: bool = True):
        super().__init__(aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, 0, n_levels,
                         log2_hashmap_size, dtype, interpolation, fused)

    def forward(self, positions: Tensor) -> Tensor:
        if self._use_fused(False, positions):
            return self._launch(False, positions.numel() // 3, positions.shape[:-1], ["density"], positions=positions.reshape(-1, 3))["density"]
        raw, _, selector = self._base(positions)
        return self._activate(raw, selector)
