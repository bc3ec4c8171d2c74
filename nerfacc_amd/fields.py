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

``fused_training=True`` (off by default) gives a query WITH grad the same treatment when only parameters require grad: one
launch forward that saves what the backward needs (``nfa_ngp_train_fwd``), one launch backward for both networks' data gradients
and the table scatter (``nfa_ngp_train_bwd``), then the networks' usual weight-gradient passes.  Its outputs are the no-grad
launch's bits; its gradients have the composed chain's rounding points.  Positions, directions or rays that require grad, a
``deterministic=True`` or ``table_gradient="merged"`` encoding, ``return_feat=True`` and every configuration outside
``fused_supported`` take the composed chain.  ``table_gradient`` is handed to the hash grid (:class:`HashGridEncoding`).

The reference's vanilla NeRF field (ref: examples/radiance_fields/mlp.py: ``VanillaNeRFRadianceField``) is
:class:`VanillaNeRFRadianceField` at the end of this module: two :class:`~nerfacc_amd.encodings.SinusoidalEncoding` and a
:class:`~nerfacc_amd.mlp.NerfMLP`, with the no-grad query as one launch of csrc/nerf_field.hip.  Its dynamic-scene field
(``TNeRFRadianceField``) is :class:`TNeRFRadianceField` behind it: a warp network in front of the vanilla field, the no-grad query
one launch of the same kernel with a warp stage.  ``NDRTNeRFRadianceField``, the dynamic-scene field with NDR's invertible warp,
is :class:`NDRTNeRFRadianceField` at the end: three coupling blocks whose weights stream through the trunk's LDS ring.

Not part of ``nerfacc_amd.__all__``: ``from nerfacc_amd.fields import NGPRadianceField, NGPDensityField,
VanillaNeRFRadianceField, TNeRFRadianceField, NDRTNeRFRadianceField``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, List, Optional, Union

import torch
from torch import Tensor, nn

from . import _backend as B
from .encodings import HashGridEncoding, SinusoidalEncoding, SphericalHarmonicsEncoding
from .mlp import FusedMLP, NerfMLP, image_elems, reference_mlp
from .rawrender import DENSITY_ACTIVATIONS, activate_density
from .samples import _contract_torch, sample_positions

FUSED_MAX_LEVELS = 16


class _NGPTrainFn(torch.autograd.Function):
    """A query with grad as one launch: the no-grad launch's outputs, and the buffers the backward reads."""

    @staticmethod
    def forward(ctx, table: Tensor, base_p: Tensor, head_p: Optional[Tensor], field: "_NGPField", full: bool, activated: bool, n: int,
                shape: tuple, inputs: dict):
        ctx.set_materialize_grads(False)
        dev, dt, G = table.device, field.dtype, field.geo_feat_dim
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        saved = [new(n, 2 * field.n_levels), new(1, n, 64), new(n, 1 + G)] + ([new(n, 16 + G), new(2, n, 64)] if full else [])
        if not full:
            want = ["density"]
        else:   # the activated mode keeps the raw colour: the backward forms the sigmoid from it
            want = ["rgb_act", "density", "rgb"] if activated else ["rgb", "sigma", "selector"]
        out = field._launch(full, n, shape, want, rgb_dtype=dt if activated else torch.float32, save=B.NGPSaved(*[B.ptr(t) for t in saved]),
                            **inputs)
        keep = field._operands(full, **inputs)[3]
        ctx.field, ctx.full, ctx.activated, ctx.n, ctx.keys, ctx.n_keep = field, full, activated, n, list(inputs), len(keep)
        ctx.save_for_backward(table, base_p, head_p, *keep, *saved, *([out["rgb"]] if full and activated else []))
        if not full:
            return out["density"]
        if activated:
            return out["rgb_act"], out["density"]
        ctx.mark_non_differentiable(out["selector"])
        return out["rgb"], out["sigma"].view(shape), out["selector"]

    @staticmethod
    def backward(ctx, *grads):
        need = ctx.needs_input_grad[:3]
        g_rgb, g_sigma = (grads[0], grads[1]) if ctx.full else (None, grads[0])
        if not any(need) or (g_rgb is None and g_sigma is None):
            return (None,) * 9
        table, base_p, head_p, *rest = ctx.saved_tensors
        g = _NGPTrainBwdFn.apply(table, base_p, head_p, g_rgb, g_sigma, ctx.field, ctx.full, ctx.activated, ctx.n, ctx.keys, ctx.n_keep, need,
                                 *[t.detach() for t in rest])
        return (*g, None, None, None, None, None, None)


class _NGPTrainBwdFn(torch.autograd.Function):
    """The backward as a function of its own, so that differentiating it again (``create_graph=True``) fails with a message that
    names the module (as ``mlp._MLPBwdFn`` does)."""

    @staticmethod
    def forward(ctx, table, base_p, head_p, g_rgb, g_sigma, field, full, activated, n, keys, n_keep, need, *rest):
        ctx.set_materialize_grads(False)
        ctx.name = type(field).__name__
        need_t, need_b, need_h = need[0], need[1], bool(full and need[2])
        if n == 0:
            return tuple(torch.zeros_like(p) if w else None for p, w in ((table, need_t), (base_p, need_b), (head_p, need_h)))
        keep, saved = list(rest[:n_keep]), list(rest[n_keep:])
        raw_rgb = saved.pop() if full and activated else None
        dev, dt, G = table.device, field.dtype, field.geo_feat_dim
        elem = B.ELEM_CODES[dt]

        def grad(t):   # float32 or the networks' type, contiguous; the kernel rounds once
            if t is None:
                return None, B.ELEM_CODES[torch.float32]
            t = (t if t.dtype in (torch.float32, dt) else t.float()).contiguous()
            return t, B.ELEM_CODES[t.dtype]

        (g_rgb, rgb_elem), (g_sigma, sigma_elem) = grad(g_rgb), grad(g_sigma)
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        bdz, bdzo = new(1, n, 64), new(n, 1 + G)
        hdz, hdzo = (new(2, n, 64), new(n, 3)) if full else (None, None)
        g_t = torch.zeros_like(table) if need_t else None
        rays = len(keys) == 1 and keys[0] == "rays"
        grid, inp, box, keep = field._operands(full, rays=tuple(keep)) if rays else field._operands(full, **dict(zip(keys, keep)))
        gr = B.NGPGrads(B.ptr(g_rgb), rgb_elem, B.ptr(g_sigma), sigma_elem, B.ptr(raw_rgb), B.ptr(hdz), B.ptr(hdzo), B.ptr(bdz), B.ptr(bdzo),
                        B.ptr(g_t))
        sv = B.NGPSaved(*[B.ptr(t) for t in saved])
        g_b = g_h = None
        with torch.cuda.device(dev):
            B.call("nfa_ngp_train_bwd", elem, int(full), int(activated), ctypes.byref(grid), B.ptr(field._bwd_image(False)),
                   B.ptr(field._bwd_image(True)) if full else None, G, ctypes.byref(inp), n, *box, int(field.unbounded),
                   DENSITY_ACTIVATIONS[field.density_activation], field.density_bias, ctypes.byref(sv), ctypes.byref(gr), B.stream())
            for mlp, want, x, hidden, dz, dzo in ((field.mlp_base, need_b, saved[0], saved[1], bdz, bdzo),
                                                  (getattr(field, "mlp_head", None), need_h, *(saved[3:5] if full else (None, None)), hdz, hdzo)):
                if not want:
                    continue
                P = mlp.params.numel()
                partials = torch.empty(mlp._slices(n) * P, dtype=torch.float32, device=dev)
                g_p = torch.empty(P, dtype=torch.float32, device=dev)
                mlp._weight_gradient(elem, x, hidden, dz, dzo, n, partials, g_p, zero_bias=False)
                if mlp is field.mlp_base:
                    g_b = g_p
                else:
                    g_h = g_p
        return g_t, g_b, g_h

    @staticmethod
    def backward(ctx, *gg):
        raise NotImplementedError(f"{ctx.name}(fused_training=True): the second order (differentiating the parameters' gradients again, "
                                  "create_graph=True) is not implemented by the fused training pass; construct the module with "
                                  "fused_training=False")


class _NGPField(nn.Module):
    """What the two fields share: the box, the grid, the base network and the fused launch."""

    def __init__(self, aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, geo_feat_dim,
                 n_levels, log2_hashmap_size, dtype, interpolation, fused, fused_training=False, table_gradient="atomic"):
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
        self.dtype, self.fused, self.fused_training = dtype, bool(fused), bool(fused_training)
        per_level_scale = math.exp((math.log(max_resolution) - math.log(base_resolution)) / (n_levels - 1)) if n_levels > 1 else 1.0
        self.encoding = HashGridEncoding(self.num_dim, n_levels, 2, log2_hashmap_size, base_resolution, per_level_scale, out_dtype=dtype,
                                         interpolation=interpolation, table_gradient=table_gradient)
        self.mlp_base = FusedMLP(2 * self.n_levels, 1 + self.geo_feat_dim, 64, 1, dtype=dtype)
        self._head_packed = None   # (key, image)
        self._bwd_packed = {}      # head?: (key, image)

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

    def _on_device(self, ts: List[Tensor]) -> bool:
        return all(t.is_cuda and t.device == self.encoding.params.device for t in ts) and all(t.dtype == torch.float32 for t in ts[:4])

    def _use_fused(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        if not (self.fused and self.fused_supported(full)):
            return False
        ts = [t for t in tensors if t is not None]
        if not self._on_device(ts):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in [*self.parameters(), *ts]))

    def _train_params(self, full: bool) -> List[Tensor]:
        return [self.encoding.params, self.mlp_base.params] + ([self.mlp_head.params] if full else [])

    def _use_train(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        """The fused training pass serves this query: grad is on and wanted by parameters only."""
        if not (self.fused_training and torch.is_grad_enabled() and self.fused_supported(full)) or self.encoding.deterministic \
                or self.encoding.table_gradient != "atomic":   # (the fused backward scatters per point: the atomic path)
            return False
        ts = [t for t in tensors if t is not None]
        if not self._on_device(ts) or any(t.requires_grad for t in ts):
            return False
        return any(p.requires_grad for p in self._train_params(full))

    def _train(self, full: bool, activated: bool, n: int, shape, **inputs):
        """The outputs of one training launch: raw ``(rgb, sigma, selector)``, activated ``(rgb_act, density)``, without ``full``
        the density alone."""
        params = self._train_params(full)
        return _NGPTrainFn.apply(params[0], params[1], params[2] if full else None, self, full, activated, n, tuple(shape), inputs)

    def _bwd_image(self, head: bool) -> Tensor:
        """A network's backward image for the fused training backward, cached and rebuilt like ``_head_image``."""
        mlp = self.mlp_head if head else self.mlp_base
        p = mlp.params
        key = (p.data_ptr(), p._version, p.device)
        if head not in self._bwd_packed or self._bwd_packed[head][0] != key:
            shape = (16 + self.geo_feat_dim, 3, 64, 2) if head else (2 * self.n_levels, 1 + self.geo_feat_dim, 64, 1)
            img = torch.empty(image_elems(*shape)[1], dtype=self.dtype, device=p.device)
            with torch.cuda.device(p.device):
                B.call("nfa_ngp_pack_bwd", B.ELEM_CODES[self.dtype], int(head), B.ptr(p), self.n_levels, self.geo_feat_dim, B.ptr(img),
                       img.numel(), B.stream())
            self._bwd_packed[head] = (key, img)
        return self._bwd_packed[head][1]

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

    def _operands(self, full: bool, positions=None, dirs=None, rays=None):
        """(grid descriptor, input descriptor, the box's two arguments, the tensors they point into) of a native call."""
        enc, t = self.encoding, self.encoding.table
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
        box = (None, B.ptr(self.aabb)) if self.aabb.is_cuda else ((ctypes.c_float * 6)(*self.aabb.tolist()), None)
        return grid, inp, box, keep

    def _launch(self, full: bool, n: int, shape, want: List[str], positions=None, dirs=None, rays=None, rgb_dtype=torch.float32,
                outputs: Optional[dict] = None, save: Optional["B.NGPSaved"] = None):
        """One fused launch; returns the outputs named in ``want`` (sigma, density, selector, feat, rgb, rgb_act), shaped ``shape``
        (``outputs``: the caller's own contiguous tensors for them).  ``save``: the training forward, which fills its buffers."""
        dev = self.encoding.params.device
        grid, inp, box, keep = self._operands(full, positions, dirs, rays)
        specs = {"sigma": ((1,), torch.float32), "density": ((1,), torch.float32), "selector": ((), torch.bool),
                 "feat": ((self.geo_feat_dim,), self.dtype), "rgb": ((3,), rgb_dtype), "rgb_act": ((3,), torch.float32)}
        out = dict.fromkeys(specs)
        for k in want:
            tail, dtype = specs[k]
            out[k] = outputs[k] if outputs is not None else torch.empty(*shape, *tail, dtype=dtype, device=dev)
        if n == 0:
            return out
        act = DENSITY_ACTIVATIONS[self.density_activation]
        lead = (B.ELEM_CODES[self.dtype], ctypes.byref(grid), B.ptr(self.mlp_base._images(self.mlp_base.params)[0]))
        tail = (self.geo_feat_dim, ctypes.byref(inp), n, *box, int(self.unbounded), act, self.density_bias, B.ptr(out["sigma"]),
                B.ELEM_CODES[torch.float32])
        with torch.cuda.device(dev):
            if save is not None:
                B.call("nfa_ngp_train_fwd", lead[0], int(full), lead[1], lead[2], B.ptr(self._head_image()) if full else None,
                       *tail[:-2], ctypes.byref(save), *tail[-2:], B.ptr(out["rgb"]), B.ELEM_CODES[rgb_dtype], B.ptr(out["density"]),
                       B.ptr(out["selector"]), B.ptr(out["rgb_act"]), B.stream())
            elif full:
                B.call("nfa_ngp_field", *lead, B.ptr(self._head_image()), *tail, B.ptr(out["rgb"]), B.ELEM_CODES[rgb_dtype],
                       B.ptr(out["density"]), B.ptr(out["selector"]), B.ptr(out["rgb_act"]), B.stream())
            else:
                B.call("nfa_ngp_density", *lead, *tail, B.ptr(out["density"]), B.ptr(out["selector"]), B.ptr(out["feat"]), B.stream())
        return out

    def density_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor) -> Tensor:
        """Densities ``[n]`` at the midpoints of packed ray samples: a trainer's ``sigma_fn``."""
        if self._use_train(False, rays_o, rays_d, t_starts, t_ends, ray_indices):
            n = t_starts.numel()
            return self._train(False, True, n, (n,), rays=(rays_o, rays_d, t_starts, t_ends, ray_indices)).view(n)
        if self._use_fused(False, rays_o, rays_d, t_starts, t_ends, ray_indices):
            n = t_starts.numel()
            return self._launch(False, n, (n,), ["density"], rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))["density"].view(n)
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices)
        raw, _, selector = self._base(s.positions)
        return self._activate(raw, selector).squeeze(-1)


class NGPRadianceField(_NGPField):
    """Instant-NGP radiance field (the reference's constructor arguments; ``dtype`` fp16 or bf16 is the networks' type,
    ``interpolation`` the hash grid's, ``fused=False`` switches the fused dispatch off, ``fused_training=True`` the fused
    training pass on)."""

    def __init__(self, aabb: Union[Tensor, List[float]], num_dim: int = 3, use_viewdirs: bool = True,
                 density_activation: Union[str, Callable] = "trunc_exp", unbounded: bool = False, base_resolution: int = 16,
                 max_resolution: int = 4096, geo_feat_dim: int = 15, n_levels: int = 16, log2_hashmap_size: int = 19, *,
                 density_bias: float = -1.0, dtype: torch.dtype = torch.float16, interpolation: str = "Linear", fused: bool = True,
                 fused_training: bool = False, table_gradient: str = "atomic"):
        super().__init__(aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, geo_feat_dim,
                         n_levels, log2_hashmap_size, dtype, interpolation, fused, fused_training, table_gradient)
        self.use_viewdirs = bool(use_viewdirs)
        if self.use_viewdirs:
            self.direction_encoding = SphericalHarmonicsEncoding(3, 4, out_dtype=dtype)
        if self.geo_feat_dim > 0:
            self.mlp_head = FusedMLP((16 if self.use_viewdirs else 0) + self.geo_feat_dim, 3, 64, 2, dtype=dtype)

    def query_density(self, x: Tensor, return_feat: bool = False):
        if not return_feat and self._use_train(False, x):
            return self._train(False, True, x.numel() // 3, x.shape[:-1], positions=x.reshape(-1, 3))
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
        if self._use_train(True, positions, directions):
            return self._train(True, True, positions.numel() // 3, positions.shape[:-1], positions=positions.reshape(-1, 3),
                               dirs=directions.reshape(-1, 3))
        if self._use_fused(True, positions, directions):
            out = self._launch(True, positions.numel() // 3, positions.shape[:-1], ["rgb_act", "density"],
                               positions=positions.reshape(-1, 3), dirs=directions.reshape(-1, 3))
            return out["rgb_act"], out["density"]
        density, embedding = self.query_density(positions, return_feat=True)
        return self._query_rgb(directions, embedding), density

    def query_raw(self, positions: Tensor, directions: Tensor):
        """``(raw_rgbs [..., 3], raw_sigmas [...], selector [...])`` at world positions, before any activation."""
        if self._use_train(True, positions, directions):
            return self._train(True, False, positions.numel() // 3, positions.shape[:-1], positions=positions.reshape(-1, 3),
                               dirs=directions.reshape(-1, 3))
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
        if self._use_train(True, rays_o, rays_d, t_starts, t_ends, ray_indices):
            out = self._train(True, not raw, n, (n,), rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))
            return out if raw else (out[0], out[1].view(n))
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
                 interpolation: str = "Linear", fused: bool = True, fused_training: bool = False, table_gradient: str = "atomic"):
        super().__init__(aabb, num_dim, density_activation, density_bias, unbounded, base_resolution, max_resolution, 0, n_levels,
                         log2_hashmap_size, dtype, interpolation, fused, fused_training, table_gradient)

    def forward(self, positions: Tensor) -> Tensor:
        if self._use_train(False, positions):
            return self._train(False, True, positions.numel() // 3, positions.shape[:-1], positions=positions.reshape(-1, 3))
        if self._use_fused(False, positions):
            return self._launch(False, positions.numel() // 3, positions.shape[:-1], ["density"], positions=positions.reshape(-1, 3))["density"]
        raw, _, selector = self._base(positions)
        return self._activate(raw, selector)


# ---------------------------------------------------------------- the vanilla NeRF field (csrc/nerf_field.hip)

NERF_POS_DIMS, NERF_DIR_DIMS = 63, 27   # SinusoidalEncoding(3, 0, 10, True) and (3, 0, 4, True)
NERF_HEAD_WIDTH, NERF_MAX_HIDDEN, NERF_HEAD_MAX_HIDDEN = 128, 8, 4


def nerf_field_limits_error(trunk: Optional[tuple], head: Optional[tuple], trunk_width: int = 0) -> Optional[str]:
    """What csrc/nerf_field.hip's check_field_shape refuses, in its order and its words; None for networks the fused query
    holds.  ``trunk`` / ``head``: ``(n_in, n_out, width, n_hidden, bias, skip_mask)`` of struct nfa_mlp_desc, or None."""
    if trunk is not None:
        n_in, n_out, w, d, bias, mask = trunk
        if w not in (128, 256):
            return f"trunk width {w}: 128 or 256 neurons are supported"
        if not 1 <= d <= NERF_MAX_HIDDEN:
            return f"trunk n_hidden {d}: 1 to {NERF_MAX_HIDDEN} hidden layers are supported"
        if n_in != NERF_POS_DIMS:
            return f"trunk n_in {n_in}: the encoded position has {NERF_POS_DIMS} features"
        if n_out != w + 1:
            return f"trunk n_out {n_out}: width + 1 = {w + 1} outputs (the bottleneck, then sigma)"
        if bias != 1:
            return f"trunk bias {bias}: the field's networks have biases (1)"
        if mask & ~((2 << d) - 4):
            return (f"trunk skip_mask 0x{mask:x}: only bits 2 to n_hidden ({d}) may be set: layer 0 takes x itself and layer 1 "
                    "follows it")
        trunk_width = w
    if head is not None:
        n_in, n_out, w, d, bias, mask = head
        if trunk_width not in (128, 256):
            return f"trunk width {trunk_width}: 128 or 256 neurons are supported"
        if w != NERF_HEAD_WIDTH:
            return f"head width {w}: {NERF_HEAD_WIDTH} neurons are supported"
        if not 1 <= d <= NERF_HEAD_MAX_HIDDEN:
            return f"head n_hidden {d}: 1 to {NERF_HEAD_MAX_HIDDEN} hidden layers are supported"
        if n_in != trunk_width + NERF_DIR_DIMS:
            return (f"head n_in {n_in}: trunk width + {NERF_DIR_DIMS} = {trunk_width + NERF_DIR_DIMS} inputs (the bottleneck, then the "
                    "encoded direction)")
        if n_out != 3:
            return f"head n_out {n_out}: 3 outputs (the colour)"
        if bias != 1:
            return f"head bias {bias}: the field's networks have biases (1)"
        if mask:
            return f"head skip_mask 0x{mask:x}: the head has no skip"
    return None


class _NerfTrainFn(torch.autograd.Function):
    """A full query with grad as one launch (``nfa_nerf_train_fwd``): the no-grad launch's outputs, and the buffers the backward
    and the weight-gradient passes read."""

    @staticmethod
    def forward(ctx, trunk_p: Tensor, head_p: Tensor, field: "VanillaNeRFRadianceField", activated: bool, n: int, inputs: dict,
                rgb_dtype, sigma_dtype):
        ctx.set_materialize_grads(False)
        t, h = field.mlp.trunk, field.mlp.head
        dev, dt, W = trunk_p.device, field.dtype, t.n_neurons
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        saved = [new(n, NERF_POS_DIMS), new(t.n_hidden_layers, n, W), new(n, W + NERF_DIR_DIMS), new(h.n_hidden_layers, n, NERF_HEAD_WIDTH)]
        rgb, sigma = field._launch(True, n, activated, rgb_dtype=rgb_dtype, sigma_dtype=sigma_dtype, save=saved, **inputs)
        ctx.field, ctx.activated, ctx.n = field, activated, n
        ctx.save_for_backward(trunk_p, head_p, *saved, *([rgb, sigma] if activated else []))
        return rgb, sigma

    @staticmethod
    def backward(ctx, g_rgb, g_sigma):
        need = ctx.needs_input_grad[:2]
        if not any(need) or (g_rgb is None and g_sigma is None):
            return (None,) * 8
        trunk_p, head_p, *rest = ctx.saved_tensors
        g = _NerfTrainBwdFn.apply(trunk_p, head_p, g_rgb, g_sigma, ctx.field, ctx.activated, ctx.n, need, *[t.detach() for t in rest])
        return (*g, None, None, None, None, None, None)


class _NerfTrainBwdFn(torch.autograd.Function):
    """The backward as a function of its own (as ``_NGPTrainBwdFn``): one launch for both networks' data gradients
    (``nfa_nerf_train_bwd``), then the two streamed weight-gradient passes.  Differentiating it again raises."""

    @staticmethod
    def forward(ctx, trunk_p, head_p, g_rgb, g_sigma, field, activated, n, need, *saved):
        ctx.set_materialize_grads(False)
        ctx.name = type(field).__name__
        if n == 0:
            return tuple(torch.zeros_like(p) if w else None for p, w in ((trunk_p, need[0]), (head_p, need[1])))
        t, h = field.mlp.trunk, field.mlp.head
        dev, dt, W = trunk_p.device, field.dtype, t.n_neurons
        elem, f32 = B.ELEM_CODES[dt], B.ELEM_CODES[torch.float32]
        enc_x, t_hidden, h_in, h_hidden, *ys = saved
        y_rgb, y_sigma = ys if activated else (None, None)

        def grad(g):   # float32 or the networks' type, contiguous; the kernel rounds once
            if g is None:
                return None, f32
            g = (g if g.dtype in (torch.float32, dt) else g.float()).contiguous()
            return g, B.ELEM_CODES[g.dtype]

        (g_rgb, rgb_elem), (g_sigma, sigma_elem) = grad(g_rgb), grad(g_sigma)
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        hdz, hdzo, tdz, tdzo = new(h.n_hidden_layers, n, NERF_HEAD_WIDTH), new(n, 3), new(t.n_hidden_layers, n, W), new(n, W + 1)
        gr = B.NerfGrads(B.ptr(g_rgb), rgb_elem, B.ptr(g_sigma), sigma_elem, B.ptr(y_rgb), B.ELEM_CODES[y_rgb.dtype] if activated else f32,
                         B.ptr(y_sigma), B.ELEM_CODES[y_sigma.dtype] if activated else f32, B.ptr(hdz), B.ptr(hdzo), B.ptr(tdz), B.ptr(tdzo))
        sv = B.NerfSaved(B.ptr(enc_x), B.ptr(t_hidden), B.ptr(h_in), B.ptr(h_hidden))
        out = []
        with torch.cuda.device(dev):
            B.call("nfa_nerf_train_bwd", elem, t._desc, h._desc, B.ptr(t._images(trunk_p)[1]), B.ptr(h._images(head_p)[1]), n, int(activated),
                   ctypes.byref(sv), ctypes.byref(gr), B.stream())
            for mlp, params, want, x, hidden, dz, dzo in ((t, trunk_p, need[0], enc_x, t_hidden, tdz, tdzo),
                                                          (h, head_p, need[1], h_in, h_hidden, hdz, hdzo)):
                g_p = None
                if want:
                    P = params.numel()
                    partials = torch.empty(mlp._slices(n) * P, dtype=torch.float32, device=dev)
                    g_p = torch.empty(P, dtype=torch.float32, device=dev)
                    mlp._weight_gradient(elem, x, hidden, dz, dzo, n, partials, g_p, zero_bias=False)
                out.append(g_p)
        return tuple(out)

    @staticmethod
    def backward(ctx, *gg):
        raise NotImplementedError(f"{ctx.name}(fused_training=True): the second order (differentiating the parameters' gradients again, "
                                  "create_graph=True) is not implemented by the fused training pass; construct the module with "
                                  "fused_training=False")


class VanillaNeRFRadianceField(nn.Module):
    """The reference's vanilla NeRF field (its constructor arguments; ``dtype`` fp16 or bf16 is the networks' type,
    ``generator`` seeds their initial weights, ``fused=False`` switches the fused dispatch off): ``posi_encoder`` and
    ``view_encoder`` (:class:`SinusoidalEncoding` of degrees (0, 10) and (0, 4) with identity, ``out_dtype=dtype``) in front of
    ``mlp`` (:class:`NerfMLP` (63, 27)).  It takes world positions: there is no box and no selector.

    With grad enabled and something that requires it, on CPU tensors, with ``fused=False`` and for a shape outside
    :meth:`fused_supported` a query runs those native passes in their order (the *composed chain*: encoder, trunk, split,
    encoder, cat, head, activation).  Under ``torch.no_grad()``, or when nothing requires grad, a supported field on its device
    takes ONE launch instead (csrc/nerf_field.hip): nothing between the positions and the outputs exists in memory, and
    ``query_density`` computes one output tile of the trunk instead of nine.  Rounding points are the composed chain's, sigma
    has its bits; the raw colour may differ in the last bit of a float32 sum (the head's first layer sums in another order).
    Outputs are ``dtype`` on both paths, as :class:`NerfMLP`'s are.

    ``fused`` is a bool, or a dict ``{"density": bool, "full": bool}`` per query kind (default: both on; DESIGN.md, "Fused NeRF
    field", has the measurements behind the defaults).

    ``fused_training=True`` (off by default) gives a full query WITH grad the same treatment when only parameters require grad:
    ``forward(x, condition)``, ``query_raw`` and ``query_on_rays`` take one launch forward that also saves what the backward
    needs (``nfa_nerf_train_fwd``), one launch backward for both networks' data gradients (``nfa_nerf_train_bwd``,
    csrc/nerf_train.hip), then the networks' usual weight-gradient passes.  Outputs are the no-grad launch's bits, gradients
    have the composed chain's rounding points and are the same bits on every run; differentiating them again raises
    ``NotImplementedError``.  Positions, directions or rays that require grad, ``condition=None`` or a broadcast condition, CPU
    tensors, density-only queries, ``fused={"full": False}`` and shapes outside :meth:`fused_supported` keep the composed chain
    ("Fused NeRF field: training")."""

    def __init__(self, net_depth: int = 8, net_width: int = 256, skip_layer: Optional[int] = 4, net_depth_condition: int = 1,
                 net_width_condition: int = 128, dtype: torch.dtype = torch.float16, generator: Optional[torch.Generator] = None,
                 fused: Union[bool, dict] = True, fused_training: bool = False):
        super().__init__()
        self.fused_training = bool(fused_training)
        self.posi_encoder = SinusoidalEncoding(3, 0, 10, True, out_dtype=dtype)
        self.view_encoder = SinusoidalEncoding(3, 0, 4, True, out_dtype=dtype)
        self.mlp = NerfMLP(self.posi_encoder.latent_dim, self.view_encoder.latent_dim, net_depth, net_width, skip_layer,
                           net_depth_condition, net_width_condition, dtype=dtype, generator=generator)
        self.dtype = dtype
        self.fused = dict(density=bool(fused), full=bool(fused)) if not isinstance(fused, dict) else \
            dict(density=bool(fused.get("density", True)), full=bool(fused.get("full", True)))
        self._head_packed = None   # (key, image)

    # ---------------------------------------------------------------- the fused launch

    def _descs(self):
        t, h = self.mlp.trunk, self.mlp.head
        return ((*t._shape, int(t.bias_enabled), t.skip_mask), (*h._shape, int(h.bias_enabled), h.skip_mask))

    def fused_supported(self, full: bool = True) -> bool:
        """The shapes csrc/nerf_field.hip serves: ``net_width`` 128 or 256, ``net_depth`` 1..8, any ``skip_layer``,
        ``net_width_condition`` 128, ``net_depth_condition`` 1..4 (the encoders are fixed at the reference's degrees)."""
        trunk, head = self._descs()
        return nerf_field_limits_error(trunk, head if full else None) is None

    def _use_fused(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        if not (self.fused["full" if full else "density"] and self.fused_supported(full)):
            return False
        ts = [t for t in tensors if t is not None]
        dev = self.mlp.trunk.params.device
        if not (all(t.is_cuda and t.device == dev for t in ts) and all(t.dtype == torch.float32 for t in ts[:4])):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in [*self.parameters(), *ts]))

    def _use_train(self, *tensors: Tensor) -> bool:
        """The fused training pass serves this full query: grad is on and wanted by parameters only (``fused={"full": False}``
        switches it off with the fused full query, whose kernel it is)."""
        if not (self.fused_training and self.fused["full"] and torch.is_grad_enabled() and self.fused_supported(True)):
            return False
        dev = self.mlp.trunk.params.device
        if not (all(t.is_cuda and t.device == dev for t in tensors) and all(t.dtype == torch.float32 for t in tensors[:4])):
            return False
        if any(t.requires_grad for t in tensors):
            return False
        return self.mlp.trunk.params.requires_grad or self.mlp.head.params.requires_grad

    def _train(self, activated: bool, n: int, rgb_dtype=None, sigma_dtype=None, **inputs):
        """``(rgb [n, 3], sigma [n])`` of one training launch, raw or activated, differentiable towards the parameters."""
        with torch.autocast("cuda", enabled=False):
            return _NerfTrainFn.apply(self.mlp.trunk.params, self.mlp.head.params, self, activated, n, inputs, rgb_dtype, sigma_dtype)

    def _head_image(self) -> Tensor:
        """The head's forward image in the fused launch's k order, rebuilt when the masters change (as StreamedMLP's images)."""
        h = self.mlp.head
        p = h.params
        key = (p.data_ptr(), p._version, p.device)
        if self._head_packed is None or self._head_packed[0] != key:
            img = torch.empty(h._image_elems[0], dtype=self.dtype, device=p.device)
            with torch.cuda.device(p.device):
                B.call("nfa_nerf_pack_head", B.ELEM_CODES[self.dtype], h._desc, self.mlp.net_width, B.ptr(p), B.ptr(img), img.numel(),
                       B.stream())
            self._head_packed = (key, img)
        return self._head_packed[1]

    def _launch(self, full: bool, n: int, activated: bool, positions=None, dirs=None, rays=None, rgb_dtype=None, sigma_dtype=None,
                save: Optional[List[Tensor]] = None):
        """One fused launch: ``(rgb [n, 3] or None, sigma [n])``, raw or activated, in ``dtype`` unless told otherwise.  ``save``:
        the training forward, which fills these four buffers (struct nfa_nerf_saved)."""
        t, h = self.mlp.trunk, self.mlp.head
        dev = t.params.device
        sigma = torch.empty(n, dtype=sigma_dtype or self.dtype, device=dev)
        rgb = torch.empty(n, 3, dtype=rgb_dtype or self.dtype, device=dev) if full else None
        if n == 0:
            return rgb, sigma
        keep = [x.contiguous() for x in (rays[:5] if rays is not None else (positions, dirs)) if x is not None]
        if rays is not None:
            keep[4] = keep[4] if keep[4].dtype == torch.int64 else keep[4].to(torch.int64)
            inp = B.NGPInput(None, None, *[B.ptr(x) for x in keep], keep[0].shape[0])
        else:
            inp = B.NGPInput(B.ptr(keep[0]), B.ptr(keep[1]) if full else None, None, None, None, None, None, 0)
        elem = B.ELEM_CODES[self.dtype]
        with torch.cuda.device(dev):
            tp = t.params
            timg = t._images(tp)[0]
            if save is not None:
                hp, sv = h.params, B.NerfSaved(*[B.ptr(b) for b in save])
                B.call("nfa_nerf_train_fwd", elem, t._desc, h._desc, B.ptr(timg), B.ptr(self._head_image()), t._bias_ptr(tp), h._bias_ptr(hp),
                       ctypes.byref(inp), n, int(activated), ctypes.byref(sv), B.ptr(sigma), B.ELEM_CODES[sigma.dtype], B.ptr(rgb),
                       B.ELEM_CODES[rgb.dtype], B.stream())
            elif full:
                hp = h.params
                B.call("nfa_nerf_field", elem, t._desc, h._desc, B.ptr(timg), B.ptr(self._head_image()), t._bias_ptr(tp), h._bias_ptr(hp),
                       ctypes.byref(inp), n, int(activated), B.ptr(sigma), B.ELEM_CODES[sigma.dtype], B.ptr(rgb), B.ELEM_CODES[rgb.dtype],
                       B.stream())
            else:
                B.call("nfa_nerf_density", elem, t._desc, B.ptr(timg), t._bias_ptr(tp), ctypes.byref(inp), n, int(activated), B.ptr(sigma),
                       B.ELEM_CODES[sigma.dtype], B.stream())
        return rgb, sigma

    # ---------------------------------------------------------------- the reference's methods

    def query_density(self, x: Tensor) -> Tensor:
        if self._use_fused(False, x):
            return self._launch(False, x.numel() // 3, True, positions=x.reshape(-1, 3))[1].view(*x.shape[:-1], 1)
        return torch.relu(self.mlp.query_density(self.posi_encoder(x)))

    def query_opacity(self, x: Tensor, step_size) -> Tensor:
        return self.query_density(x) * step_size   # (small densities: 1 - exp(-density * step_size) is the same)

    def forward(self, x: Tensor, condition: Optional[Tensor] = None):
        if condition is not None and condition.shape == x.shape and self._use_train(x, condition):
            rgb, sigma = self._train(True, x.numel() // 3, positions=x.reshape(-1, 3), dirs=condition.reshape(-1, 3))
            return rgb.view(*x.shape[:-1], 3), sigma.view(*x.shape[:-1], 1)
        if condition is not None and condition.shape == x.shape and self._use_fused(True, x, condition):
            rgb, sigma = self._launch(True, x.numel() // 3, True, positions=x.reshape(-1, 3), dirs=condition.reshape(-1, 3))
            return rgb.view(*x.shape[:-1], 3), sigma.view(*x.shape[:-1], 1)
        rgb, sigma = self.mlp(self.posi_encoder(x), None if condition is None else self.view_encoder(condition))
        return torch.sigmoid(rgb), torch.relu(sigma)

    # ---------------------------------------------------------------- the methods in the NGP fields' shape

    def query_raw(self, positions: Tensor, directions: Tensor):
        """``(raw_rgbs [..., 3], raw_sigmas [...])`` at world positions, before any activation."""
        if positions.shape == directions.shape and self._use_train(positions, directions):
            rgb, sigma = self._train(False, positions.numel() // 3, positions=positions.reshape(-1, 3), dirs=directions.reshape(-1, 3))
            return rgb.view(*positions.shape[:-1], 3), sigma.view(positions.shape[:-1])
        if positions.shape == directions.shape and self._use_fused(True, positions, directions):
            rgb, sigma = self._launch(True, positions.numel() // 3, False, positions=positions.reshape(-1, 3),
                                      dirs=directions.reshape(-1, 3))
            return rgb.view(*positions.shape[:-1], 3), sigma.view(positions.shape[:-1])
        rgb, sigma = self.mlp(self.posi_encoder(positions), self.view_encoder(directions))
        return rgb, sigma.squeeze(-1)

    def density_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor) -> Tensor:
        """Densities ``[n]`` at the midpoints of packed ray samples: a trainer's ``sigma_fn``."""
        if self._use_fused(False, rays_o, rays_d, t_starts, t_ends, ray_indices):
            return self._launch(False, t_starts.numel(), True, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))[1]
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices)
        return self.query_density(s.positions).squeeze(-1)

    def query_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, raw: bool = True):
        """The field at the midpoints of packed ray samples.  ``raw=True``: ``(raw_rgbs [n, 3], raw_sigmas [n])``, what
        :func:`nerfacc_amd.rendering_from_raw` takes; otherwise ``(rgbs [n, 3], sigmas [n])`` activated."""
        if self._use_train(rays_o, rays_d, t_starts, t_ends, ray_indices):
            return self._train(not raw, t_starts.numel(), rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))
        if self._use_fused(True, rays_o, rays_d, t_starts, t_ends, ray_indices):
            return self._launch(True, t_starts.numel(), not raw, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices))
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="raw")
        if raw:
            return self.query_raw(s.positions, s.dirs)
        rgb, sigma = self.forward(s.positions, s.dirs)
        return rgb, sigma.squeeze(-1)

    def load_reference_state_dict(self, sd: dict) -> None:
        """Takes the reference module's state dict: ``mlp.base.*``, ``mlp.sigma_layer.*``, ``mlp.bottleneck_layer.*``,
        ``mlp.rgb_layer.*`` (through :meth:`NerfMLP.load_reference_state_dict`) and the encoders' ``scales`` buffers, which
        must be the reference's ``2^k``.  Any other key, a missing key and a wrong shape raise ``ValueError``."""
        sd = dict(sd)
        for name, enc in (("posi_encoder", self.posi_encoder), ("view_encoder", self.view_encoder)):
            scales = sd.pop(name + ".scales", None)
            if scales is not None:
                want = torch.tensor([2.0 ** k for k in range(enc.min_deg, enc.max_deg)], dtype=torch.float64)
                if scales.numel() != want.numel() or not torch.equal(scales.detach().cpu().double().reshape(-1), want):
                    raise ValueError(f"VanillaNeRFRadianceField: load_reference_state_dict: '{name}.scales' is not 2^k for k in "
                                     f"{enc.min_deg} .. {enc.max_deg - 1}")
        other = sorted(k for k in sd if not k.startswith("mlp."))
        if other:
            raise ValueError(f"VanillaNeRFRadianceField: load_reference_state_dict: unexpected keys {other}")
        self.mlp.load_reference_state_dict({k[len("mlp."):]: v for k, v in sd.items()})


# ---------------------------------------------------------------- the T-NeRF field (csrc/nerf_field.hip, the WARP instantiations)

TNERF_WARP_DIMS, TNERF_WARP_WIDTH, TNERF_WARP_MAX_HIDDEN = 36, 64, 4   # SinusoidalEncoding(3, 0, 4, True) and (1, 0, 4, True)


def tnerf_field_limits_error(warp: tuple, trunk: Optional[tuple], head: Optional[tuple]) -> Optional[str]:
    """What csrc/nerf_field.hip's check_warp_shape and then check_field_shape refuse, in their order and their words; None
    for networks the fused T-NeRF query holds.  Each: ``(n_in, n_out, width, n_hidden, bias, skip_mask)``, or None."""
    n_in, n_out, w, d, bias, mask = warp
    if w != TNERF_WARP_WIDTH:
        return f"warp width {w}: {TNERF_WARP_WIDTH} neurons are supported"
    if not 1 <= d <= TNERF_WARP_MAX_HIDDEN:
        return f"warp n_hidden {d}: 1 to {TNERF_WARP_MAX_HIDDEN} hidden layers are supported"
    if n_in != TNERF_WARP_DIMS:
        return f"warp n_in {n_in}: the encoded position and time have {TNERF_WARP_DIMS} features"
    if n_out != 3:
        return f"warp n_out {n_out}: 3 outputs (the deformation)"
    if bias != 1:
        return f"warp bias {bias}: the field's networks have biases (1)"
    if mask & ~((2 << d) - 4):
        return f"warp skip_mask 0x{mask:x}: only bits 2 to n_hidden ({d}) may be set: layer 0 takes x itself and layer 1 follows it"
    return nerf_field_limits_error(trunk, head)


class _TNerfTrainFn(torch.autograd.Function):
    """A full T-NeRF query with grad as one launch (``nfa_tnerf_train_fwd``): the no-grad launch's outputs, and the buffers the
    backward and the three weight-gradient passes read (shaped like ``_NerfTrainFn``)."""

    @staticmethod
    def forward(ctx, warp_p: Tensor, trunk_p: Tensor, head_p: Tensor, field: "TNeRFRadianceField", activated: bool, n: int, inputs: dict,
                rgb_dtype, sigma_dtype):
        ctx.set_materialize_grads(False)
        w, t, h = field.warp, field.nerf.mlp.trunk, field.nerf.mlp.head
        dev, dt, W = trunk_p.device, field.dtype, t.n_neurons
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        saved = [new(n, NERF_POS_DIMS), new(t.n_hidden_layers, n, W), new(n, W + NERF_DIR_DIMS), new(h.n_hidden_layers, n, NERF_HEAD_WIDTH),
                 new(n, TNERF_WARP_DIMS), new(w.n_hidden_layers, n, TNERF_WARP_WIDTH)]
        rgb, sigma, xw = field._launch("full", n, activated, rgb_dtype=rgb_dtype, sigma_dtype=sigma_dtype, warped=True, save=saved, **inputs)
        ctx.field, ctx.activated, ctx.n = field, activated, n
        ctx.save_for_backward(warp_p, trunk_p, head_p, *saved, xw, *([rgb, sigma] if activated else []))
        return rgb, sigma

    @staticmethod
    def backward(ctx, g_rgb, g_sigma):
        need = ctx.needs_input_grad[:3]
        if not any(need) or (g_rgb is None and g_sigma is None):
            return (None,) * 9
        warp_p, trunk_p, head_p, *rest = ctx.saved_tensors
        g = _TNerfTrainBwdFn.apply(warp_p, trunk_p, head_p, g_rgb, g_sigma, ctx.field, ctx.activated, ctx.n, need, *[t.detach() for t in rest])
        return (*g, None, None, None, None, None, None)


class _TNerfTrainBwdFn(torch.autograd.Function):
    """The backward as a function of its own (as ``_NerfTrainBwdFn``): one launch for all three networks' data gradients
    (``nfa_tnerf_train_bwd``), then the warp's and the two streamed weight-gradient passes.  Differentiating it again raises."""

    @staticmethod
    def forward(ctx, warp_p, trunk_p, head_p, g_rgb, g_sigma, field, activated, n, need, *saved):
        ctx.set_materialize_grads(False)
        ctx.name = type(field).__name__
        if n == 0:
            return tuple(torch.zeros_like(p) if want else None for p, want in zip((warp_p, trunk_p, head_p), need))
        w, t, h = field.warp, field.nerf.mlp.trunk, field.nerf.mlp.head
        dev, dt, W = trunk_p.device, field.dtype, t.n_neurons
        elem, f32 = B.ELEM_CODES[dt], B.ELEM_CODES[torch.float32]
        enc_x, t_hidden, h_in, h_hidden, w_in, w_hidden, xw, *ys = saved
        y_rgb, y_sigma = ys if activated else (None, None)

        def grad(g):   # float32 or the networks' type, contiguous; the kernel rounds once
            if g is None:
                return None, f32
            g = (g if g.dtype in (torch.float32, dt) else g.float()).contiguous()
            return g, B.ELEM_CODES[g.dtype]

        (g_rgb, rgb_elem), (g_sigma, sigma_elem) = grad(g_rgb), grad(g_sigma)
        new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
        hdz, hdzo, tdz, tdzo = new(h.n_hidden_layers, n, NERF_HEAD_WIDTH), new(n, 3), new(t.n_hidden_layers, n, W), new(n, W + 1)
        wdz, wdzo = new(w.n_hidden_layers, n, TNERF_WARP_WIDTH), new(n, 3)
        gr = B.NerfGrads(B.ptr(g_rgb), rgb_elem, B.ptr(g_sigma), sigma_elem, B.ptr(y_rgb), B.ELEM_CODES[y_rgb.dtype] if activated else f32,
                         B.ptr(y_sigma), B.ELEM_CODES[y_sigma.dtype] if activated else f32, B.ptr(hdz), B.ptr(hdzo), B.ptr(tdz), B.ptr(tdzo))
        sv = B.NerfSaved(B.ptr(enc_x), B.ptr(t_hidden), B.ptr(h_in), B.ptr(h_hidden))
        wsv, wgr = B.TNerfSaved(B.ptr(w_in), B.ptr(w_hidden), B.ptr(xw)), B.TNerfGrads(B.ptr(wdz), B.ptr(wdzo))
        out = []
        with torch.cuda.device(dev):
            B.call("nfa_tnerf_train_bwd", elem, w._desc, t._desc, h._desc, B.ptr(w._images(warp_p)[1]), B.ptr(t._images(trunk_p)[1]),
                   B.ptr(h._images(head_p)[1]), n, int(activated), ctypes.byref(sv), ctypes.byref(wsv), ctypes.byref(gr), ctypes.byref(wgr),
                   B.stream())
            for mlp, params, want, x, hidden, dz, dzo in ((w, warp_p, need[0], w_in, w_hidden, wdz, wdzo), (t, trunk_p, need[1], enc_x, t_hidden, tdz, tdzo),
                                                          (h, head_p, need[2], h_in, h_hidden, hdz, hdzo)):
                g_p = None
                if want:
                    P = params.numel()
                    partials = torch.empty(mlp._slices(n) * P, dtype=torch.float32, device=dev)
                    g_p = torch.empty(P, dtype=torch.float32, device=dev)
                    mlp._weight_gradient(elem, x, hidden, dz, dzo, n, partials, g_p, zero_bias=False)
                out.append(g_p)
        return tuple(out)

    @staticmethod
    def backward(ctx, *gg):
        raise NotImplementedError(f"{ctx.name}(fused_training=True): the second order (differentiating the parameters' gradients again, "
                                  "create_graph=True) is not implemented by the fused training pass; construct the module with "
                                  "fused_training=False")


class TNeRFRadianceField(nn.Module):
    """The reference's dynamic-scene field (ref: examples/radiance_fields/mlp.py: ``TNeRFRadianceField``, the field of
    ``train_mlp_tnerf.py``): ``posi_encoder`` and ``time_encoder`` (:class:`SinusoidalEncoding` (3, 0, 4) and (1, 0, 4) with
    identity, ``out_dtype=dtype``) feed ``warp`` (:func:`reference_mlp` (36, 3, 4, 64, skip_layer 2), float32 output, its output
    layer initialised ``uniform_(0, 1e-4)`` with a zero bias as in the reference), and ``nerf``
    (:class:`VanillaNeRFRadianceField`) is queried at ``x + warp(cat(posi_encoder(x), time_encoder(t)))``.  The deformation is
    never rounded to the half type: the sum is float32.

    With grad enabled and something that requires it, on CPU tensors, with ``fused=False`` and for a shape outside
    :meth:`fused_supported` a query runs the native passes in their order (the *composed chain*: two encoders, ``cat``,
    :class:`FusedMLP`, add, then ``nerf``'s own methods), which trains: the warp network's gradients come through the trunk's
    ``dL/dx`` and the position encoder's backward.  Under ``torch.no_grad()``, or when nothing requires grad, a supported field
    takes ONE launch (csrc/nerf_field.hip, the WARP instantiations): the warp network's image stays in LDS, and nothing between
    ``(x, t, dir)``, or a ray sample and its ray's timestamp, and the outputs exists in memory.  The warped positions and sigma
    are the composed chain's bits; the raw colour carries the vanilla field's one last-bit difference.

    ``fused`` is a bool or ``{"density": bool, "full": bool}`` (:meth:`warped_positions` follows ``"density"``); it is handed
    to ``nerf`` as well.  DESIGN.md, "Fused T-NeRF field", has the measurements behind the defaults.

    ``fused_training=True`` (off by default) gives a full query WITH grad the same treatment when only parameters require grad
    and ``warp.params`` is among them: ``forward(x, t, condition)``, ``query_raw`` and ``query_on_rays`` take one launch forward
    (``nfa_tnerf_train_fwd``: the no-grad launch's bits, and what the backward reads), one launch backward for all three
    networks' data gradients (``nfa_tnerf_train_bwd``, csrc/nerf_train.hip: the trunk's ``dL/dx``, the position encoder's
    backward and the warp network's chain follow the vanilla pass in registers and LDS), then the three networks' usual
    weight-gradient passes.  Gradients have the composed chain's rounding points and are the same bits on every run;
    differentiating them again raises ``NotImplementedError``.  Inputs that require grad, ``condition=None`` or a broadcast
    condition, a ``t`` or ``timestamps`` of another shape, CPU tensors, density-only queries and :meth:`warped_positions`,
    ``fused={"full": False}``, shapes outside :meth:`fused_supported` and a frozen warp keep the composed chain (DESIGN.md,
    "Fused T-NeRF field: training")."""

    def __init__(self, dtype: torch.dtype = torch.float16, generator: Optional[torch.Generator] = None, fused: Union[bool, dict] = True,
                 fused_training: bool = False):
        super().__init__()
        self.fused_training = bool(fused_training)
        self.posi_encoder = SinusoidalEncoding(3, 0, 4, True, out_dtype=dtype)
        self.time_encoder = SinusoidalEncoding(1, 0, 4, True, out_dtype=dtype)
        self.warp = reference_mlp(self.posi_encoder.latent_dim + self.time_encoder.latent_dim, 3, 4, 64, 2, dtype=dtype,
                                  out_dtype=torch.float32, generator=generator)
        with torch.no_grad():   # output_init=functools.partial(torch.nn.init.uniform_, b=1e-4); the bias is zero already
            out = self.warp.weight(self.warp.n_hidden_layers)
            out.copy_(torch.rand(out.shape, generator=generator or torch.Generator().manual_seed(1337)) * 1e-4)
        self.nerf = VanillaNeRFRadianceField(dtype=dtype, generator=generator, fused=fused)
        self.dtype = dtype
        self.fused = dict(self.nerf.fused)

    # ---------------------------------------------------------------- the fused launch

    def fused_supported(self, full: bool = True) -> bool:
        """The shapes csrc/nerf_field.hip serves with a warp stage: the warp network (36, 3, 64, 1..4 hidden layers, biases,
        any skip) in front of what :meth:`VanillaNeRFRadianceField.fused_supported` lists."""
        w = self.warp
        trunk, head = self.nerf._descs()
        return tnerf_field_limits_error((*w._shape, int(w.bias_enabled), w.skip_mask), trunk, head if full else None) is None

    def _use_fused(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        if not (self.fused["full" if full else "density"] and self.fused_supported(full)):
            return False
        ts = [t for t in tensors if t is not None]
        dev = self.warp.params.device
        if not (all(t.is_cuda and t.device == dev for t in ts) and all(t.dtype == torch.float32 for t in ts if t.is_floating_point())):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in [*self.parameters(), *ts]))

    def _use_train(self, *tensors: Tensor) -> bool:
        """The fused training pass serves this full query: grad is on, wanted by parameters only, the warp's among them."""
        if not (self.fused_training and self.fused["full"] and torch.is_grad_enabled() and self.fused_supported(True)):
            return False
        dev = self.warp.params.device
        if not (all(t.is_cuda and t.device == dev for t in tensors) and all(t.dtype == torch.float32 for t in tensors if t.is_floating_point())):
            return False
        return self.warp.params.requires_grad and not any(t.requires_grad for t in tensors)

    def _train(self, activated: bool, n: int, rgb_dtype=None, sigma_dtype=None, **inputs):
        """``(rgb [n, 3], sigma [n])`` of one training launch, raw or activated, differentiable towards the parameters."""
        m = self.nerf.mlp
        with torch.autocast("cuda", enabled=False):
            return _TNerfTrainFn.apply(self.warp.params, m.trunk.params, m.head.params, self, activated, n, inputs, rgb_dtype, sigma_dtype)

    def _launch(self, kind: str, n: int, activated: bool = False, positions=None, times=None, dirs=None, rays=None, warped: bool = False,
                rgb_dtype=None, sigma_dtype=None, save: Optional[List[Tensor]] = None):
        """One fused launch.  ``kind``: ``"full"``: ``(rgb [n, 3], sigma [n], warped [n, 3] or None)``; ``"density"``:
        ``(None, sigma, warped or None)``; ``"warp"``: ``(None, None, warped)``.  ``times``: [n] with ``positions``, [n_rays]
        with ``rays``.  ``save``: the training forward, which fills these six buffers (struct nfa_nerf_saved, then ``warp_in`` and
        ``warp_hidden`` of struct nfa_tnerf_saved, whose third member is ``warped``)."""
        full = kind == "full"
        w, t, h = self.warp, self.nerf.mlp.trunk, self.nerf.mlp.head
        dev = w.params.device
        sigma = torch.empty(n, dtype=sigma_dtype or self.dtype, device=dev) if kind != "warp" else None
        rgb = torch.empty(n, 3, dtype=rgb_dtype or self.dtype, device=dev) if full else None
        xw = torch.empty(n, 3, dtype=torch.float32, device=dev) if warped or kind == "warp" else None
        if n == 0:
            return rgb, sigma, xw
        keep = [x.contiguous() for x in (rays[:5] if rays is not None else (positions, dirs)) if x is not None]
        times = times.contiguous()
        if rays is not None:
            keep[4] = keep[4] if keep[4].dtype == torch.int64 else keep[4].to(torch.int64)
            inp = B.NGPInput(None, None, *[B.ptr(x) for x in keep], keep[0].shape[0])
        else:
            inp = B.NGPInput(B.ptr(keep[0]), B.ptr(keep[1]) if full else None, None, None, None, None, None, 0)
        elem = B.ELEM_CODES[self.dtype]
        with torch.cuda.device(dev):
            wp, tp = w.params, t.params
            wimg = w._images(wp)[0]
            if kind == "warp":
                B.call("nfa_tnerf_warp", elem, w._desc, B.ptr(wimg), w._bias_ptr(wp), ctypes.byref(inp), B.ptr(times), n, B.ptr(xw),
                       B.stream())
                return rgb, sigma, xw
            timg = t._images(tp)[0]
            if save is not None:
                hp = h.params
                sv, wsv = B.NerfSaved(*[B.ptr(b) for b in save[:4]]), B.TNerfSaved(B.ptr(save[4]), B.ptr(save[5]), B.ptr(xw))
                B.call("nfa_tnerf_train_fwd", elem, w._desc, t._desc, h._desc, B.ptr(wimg), B.ptr(timg), B.ptr(self.nerf._head_image()),
                       w._bias_ptr(wp), t._bias_ptr(tp), h._bias_ptr(hp), ctypes.byref(inp), B.ptr(times), n, int(activated),
                       ctypes.byref(sv), ctypes.byref(wsv), B.ptr(sigma), B.ELEM_CODES[sigma.dtype], B.ptr(rgb), B.ELEM_CODES[rgb.dtype],
                       B.stream())
            elif full:
                hp = h.params
                B.call("nfa_tnerf_field", elem, w._desc, t._desc, h._desc, B.ptr(wimg), B.ptr(timg), B.ptr(self.nerf._head_image()),
                       w._bias_ptr(wp), t._bias_ptr(tp), h._bias_ptr(hp), ctypes.byref(inp), B.ptr(times), n, int(activated), B.ptr(sigma),
                       B.ELEM_CODES[sigma.dtype], B.ptr(rgb), B.ELEM_CODES[rgb.dtype], B.ptr(xw) if xw is not None else None, B.stream())
            else:
                B.call("nfa_tnerf_density", elem, w._desc, t._desc, B.ptr(wimg), B.ptr(timg), w._bias_ptr(wp), t._bias_ptr(tp),
                       ctypes.byref(inp), B.ptr(times), n, int(activated), B.ptr(sigma), B.ELEM_CODES[sigma.dtype],
                       B.ptr(xw) if xw is not None else None, B.stream())
        return rgb, sigma, xw

    @staticmethod
    def _point_times(x: Tensor, t: Tensor) -> bool:
        """One timestamp per point: ``t`` is ``x``'s shape with a last dimension of 1."""
        return t.shape == (*x.shape[:-1], 1)

    # ---------------------------------------------------------------- the reference's methods

    def warped_positions(self, x: Tensor, t: Tensor) -> Tensor:
        """``x + warp(cat(posi_encoder(x), time_encoder(t)))``, float32, in ``x``'s shape."""
        if self._point_times(x, t) and self._use_fused(False, x, t):
            return self._launch("warp", x.numel() // 3, positions=x.reshape(-1, 3), times=t.reshape(-1))[2].view(x.shape)
        enc = torch.cat([self.posi_encoder(x), self.time_encoder(t)], dim=-1)
        return x + self.warp(enc.reshape(-1, enc.shape[-1])).view(x.shape)

    def query_density(self, x: Tensor, t: Tensor) -> Tensor:
        if self._point_times(x, t) and self._use_fused(False, x, t):
            sigma = self._launch("density", x.numel() // 3, True, positions=x.reshape(-1, 3), times=t.reshape(-1))[1]
            return sigma.view(*x.shape[:-1], 1)
        return self.nerf.query_density(self.warped_positions(x, t))

    def query_opacity(self, x: Tensor, timestamps: Tensor, step_size) -> Tensor:
        idxs = torch.randint(0, len(timestamps), (x.shape[0],), device=x.device)
        return self.query_density(x, timestamps[idxs]) * step_size   # (small densities: 1 - exp(-density * step_size) is the same)

    def forward(self, x: Tensor, t: Tensor, condition: Optional[Tensor] = None):
        if condition is not None and condition.shape == x.shape and self._point_times(x, t) and self._use_train(x, t, condition):
            rgb, sigma = self._train(True, x.numel() // 3, positions=x.reshape(-1, 3), times=t.reshape(-1), dirs=condition.reshape(-1, 3))
            return rgb.view(*x.shape[:-1], 3), sigma.view(*x.shape[:-1], 1)
        if condition is not None and condition.shape == x.shape and self._point_times(x, t) and self._use_fused(True, x, t, condition):
            rgb, sigma, _ = self._launch("full", x.numel() // 3, True, positions=x.reshape(-1, 3), times=t.reshape(-1),
                                         dirs=condition.reshape(-1, 3))
            return rgb.view(*x.shape[:-1], 3), sigma.view(*x.shape[:-1], 1)
        return self.nerf(self.warped_positions(x, t), condition=condition)

    # ---------------------------------------------------------------- the methods in the other fields' shape

    def query_raw(self, positions: Tensor, t: Tensor, directions: Tensor):
        """``(raw_rgbs [..., 3], raw_sigmas [...])`` at world positions and times ``[..., 1]``, before any activation."""
        if positions.shape == directions.shape and self._point_times(positions, t) and self._use_train(positions, t, directions):
            rgb, sigma = self._train(False, positions.numel() // 3, positions=positions.reshape(-1, 3), times=t.reshape(-1),
                                     dirs=directions.reshape(-1, 3))
            return rgb.view(*positions.shape[:-1], 3), sigma.view(positions.shape[:-1])
        if positions.shape == directions.shape and self._point_times(positions, t) and self._use_fused(True, positions, t, directions):
            rgb, sigma, _ = self._launch("full", positions.numel() // 3, False, positions=positions.reshape(-1, 3), times=t.reshape(-1),
                                         dirs=directions.reshape(-1, 3))
            return rgb.view(*positions.shape[:-1], 3), sigma.view(positions.shape[:-1])
        return self.nerf.query_raw(self.warped_positions(positions, t), directions)

    def _ray_times(self, rays_o: Tensor, timestamps: Tensor) -> bool:
        return timestamps.numel() == rays_o.shape[0]

    def density_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor,
                        timestamps: Tensor) -> Tensor:
        """Densities ``[n]`` at the midpoints of packed ray samples, each at its ray's time (``timestamps`` ``[n_rays, 1]``): a
        trainer's ``sigma_fn``."""
        if self._ray_times(rays_o, timestamps) and self._use_fused(False, rays_o, rays_d, t_starts, t_ends, timestamps, ray_indices):
            return self._launch("density", t_starts.numel(), True, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices),
                                times=timestamps.reshape(-1))[1]
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices)
        return self.query_density(s.positions, timestamps.reshape(-1, 1)[ray_indices]).squeeze(-1)

    def query_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, timestamps: Tensor,
                      raw: bool = True):
        """The field at the midpoints of packed ray samples, each at its ray's time.  ``raw=True``: ``(raw_rgbs [n, 3],
        raw_sigmas [n])``, what :func:`nerfacc_amd.rendering_from_raw` takes; otherwise ``(rgbs [n, 3], sigmas [n])`` activated."""
        if self._ray_times(rays_o, timestamps) and self._use_train(rays_o, rays_d, t_starts, t_ends, timestamps, ray_indices):
            return self._train(not raw, t_starts.numel(), rays=(rays_o, rays_d, t_starts, t_ends, ray_indices), times=timestamps.reshape(-1))
        if self._ray_times(rays_o, timestamps) and self._use_fused(True, rays_o, rays_d, t_starts, t_ends, timestamps, ray_indices):
            return self._launch("full", t_starts.numel(), not raw, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices),
                                times=timestamps.reshape(-1))[:2]
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="raw")
        t = timestamps.reshape(-1, 1)[ray_indices]
        if raw:
            return self.query_raw(s.positions, t, s.dirs)
        rgb, sigma = self.forward(s.positions, t, s.dirs)
        return rgb, sigma.squeeze(-1)

    def load_reference_state_dict(self, sd: dict) -> None:
        """Takes the reference module's state dict: ``warp.hidden_layers.N.*`` and ``warp.output_layer.*`` (through
        :meth:`FusedMLP.load_reference_state_dict`), ``nerf.*`` (through :meth:`VanillaNeRFRadianceField.load_reference_state_dict`)
        and the encoders' ``scales`` buffers, which must be the reference's ``2^k``.  Any other key, a missing key and a wrong
        shape raise ``ValueError``."""
        sd = dict(sd)
        for name, enc in (("posi_encoder", self.posi_encoder), ("time_encoder", self.time_encoder)):
            scales = sd.pop(name + ".scales", None)
            if scales is not None:
                want = torch.tensor([2.0 ** k for k in range(enc.min_deg, enc.max_deg)], dtype=torch.float64)
                if scales.numel() != want.numel() or not torch.equal(scales.detach().cpu().double().reshape(-1), want):
                    raise ValueError(f"TNeRFRadianceField: load_reference_state_dict: '{name}.scales' is not 2^k for k in "
                                     f"{enc.min_deg} .. {enc.max_deg - 1}")
        other = sorted(k for k in sd if not k.startswith(("warp.", "nerf.")))
        if other:
            raise ValueError(f"TNeRFRadianceField: load_reference_state_dict: unexpected keys {other}")
        warp_sd = {k[len("warp."):]: v for k, v in sd.items() if k.startswith("warp.")}
        nerf_sd = {k[len("nerf."):]: v for k, v in sd.items() if k.startswith("nerf.")}
        self.warp.load_reference_state_dict(warp_sd)
        self.nerf.load_reference_state_dict(nerf_sd)


# ---------------------------------------------------------------- the NDR T-NeRF field (csrc/ndr_warp.h, nerf_field.hip WARP == 2)

NDR_BLOCKS, NDR_TIME_DIMS, NDR_TIME_WIDTH = 3, 9, 64
NDR_NET1, NDR_NET2 = (82, 1, 128, 2, 1, 0), (73, 3, 128, 1, 1, 0)   # struct nfa_mlp_desc of warp_layers_1[i] and warp_layers_2[i]
NDR_IMAGE_ELEMS, NDR_BIAS_FLOATS = 3 * 49152, 3 * 576             # include/nerfacc_hip.h: nfa_ndr_field's warp_image and warp_bias


def ndr_field_limits_error(nets1: List[tuple], nets2: List[tuple], times: List[tuple], trunk: Optional[tuple],
                           head: Optional[tuple]) -> Optional[str]:
    """None for a field the fused NDR query holds: exactly the reference's warp (three blocks; ``nets1`` / ``nets2`` the
    descriptors of ``warp_layers_1`` / ``warp_layers_2``, ``times`` the shapes of the twelve time-layer tensors) in front of
    what :func:`nerf_field_limits_error` accepts."""
    if len(nets1) != NDR_BLOCKS or len(nets2) != NDR_BLOCKS:
        return f"{len(nets1)} and {len(nets2)} warp networks: {NDR_BLOCKS} coupling blocks are supported"
    for name, descs, want in (("warp_layers_1", nets1, NDR_NET1), ("warp_layers_2", nets2, NDR_NET2)):
        for i, d in enumerate(descs):
            if tuple(d) != want:
                return f"{name}[{i}] {tuple(d)}: (n_in, n_out, width, n_hidden, bias, skip_mask) = {want} is supported"
    want_t = [(NDR_TIME_WIDTH, NDR_TIME_DIMS), (NDR_TIME_WIDTH,)] * (2 * NDR_BLOCKS)
    if [tuple(s) for s in times] != want_t:
        return f"time layers {[tuple(s) for s in times]}: {2 * NDR_BLOCKS} layers of {NDR_TIME_DIMS} -> {NDR_TIME_WIDTH} with biases are supported"
    return nerf_field_limits_error(trunk, head)


class _NdrTimeFn(torch.autograd.Function):
    """The six time layers on ``t [n]`` as one native pass (``nfa_ndr_time_features``): ``[n, 6, 64]`` of the networks' type, the
    bits the fused launch forms in registers.  Backward towards the six matrices and biases: torch matmuls of the gradient
    ``[n, 64]`` against the encoded time ``[n, 9]``.  No gradient towards ``t``."""

    @staticmethod
    def forward(ctx, t: Tensor, t_enc: Tensor, field: "NDRTNeRFRadianceField", *wb: Tensor):
        if t.requires_grad:
            raise NotImplementedError("NDRTNeRFRadianceField: no gradient towards the times is implemented")
        n, dev = t.numel(), t.device
        out = torch.empty(n, 2 * NDR_BLOCKS, NDR_TIME_WIDTH, dtype=field.dtype, device=dev)
        if n:
            img, bias = field._time_image()
            with torch.cuda.device(dev):
                B.call("nfa_ndr_time_features", B.ELEM_CODES[field.dtype], B.ptr(img), B.ptr(bias), B.ptr(t), n, B.ptr(out), B.stream())
        ctx.save_for_backward(t_enc)
        return out

    @staticmethod
    def backward(ctx, g):
        (t_enc,) = ctx.saved_tensors
        G = g.float().reshape(g.shape[0], -1)                                  # [n, 6 * 64]
        dW = (G.t() @ t_enc.float()).view(2 * NDR_BLOCKS, NDR_TIME_WIDTH, NDR_TIME_DIMS)
        db = G.sum(0).view(2 * NDR_BLOCKS, NDR_TIME_WIDTH)
        grads = [v for j in range(2 * NDR_BLOCKS) for v in (dW[j], db[j])]
        return (None, None, None, *[v if need else None for v, need in zip(grads, ctx.needs_input_grad[3:])])


class NDRTNeRFRadianceField(nn.Module):
    """The reference's dynamic-scene field with the invertible warp of Neural Deformable Radiance fields (ref:
    examples/radiance_fields/mlp.py: ``NDRTNeRFRadianceField``; arXiv 2206.15258).  ``time_encoder``, ``posi_encoder_1`` and
    ``posi_encoder_2`` are :class:`SinusoidalEncoding` (1, 0, 4), (2, 0, 4) and (1, 0, 4) with identity, ``out_dtype=dtype``;
    ``warp_layers_1[i]`` is :func:`reference_mlp` (82, 1, 2, 128) and ``warp_layers_2[i]`` (73, 3, 1, 128), float32 outputs, output
    layers initialised ``uniform_(0, 1e-4)`` with zero bias; ``time_layers_1[i]`` and ``time_layers_2[i]`` hold the reference's
    ``DenseLayer(9, 64)`` as float32 ``weight [64, 9]`` and ``bias [64]``; ``nerf`` is :class:`VanillaNeRFRadianceField`.  Three
    coupling blocks move ``x = (u, v, w)``::

        dw = warp_layers_1[i](cat[posi_encoder_1(u, v), time_layers_1[i](time_encoder(t))]);   w = w + dw
        theta, tu, tv = warp_layers_2[i](cat[posi_encoder_2(w), time_layers_2[i](time_encoder(t))])
        u, v = cos(theta) (u - tu) + sin(theta) (v - tv),  cos(theta) (v - tv) - sin(theta) (u - tu)

    with the axes rolled ``[1, 2, 0]`` behind block 0 and ``[2, 0, 1]`` behind block 1, and ``nerf`` is queried at the result.
    ``dw``, ``theta``, the translation, the sums and the rotation are float32 and never rounded to the half type; a time layer
    rounds once to ``dtype``; ``sin`` and ``cos`` of ``theta`` are a float32 :class:`SinusoidalEncoding` (1, 0, 1).

    With grad enabled and something that requires it, on CPU tensors, with ``fused=False`` and for a shape outside
    :meth:`fused_supported` a query runs the native passes in their order (the *composed chain*), which trains every parameter;
    the six time layers are one native pass there (``nfa_ndr_time_features``).  Under ``torch.no_grad()``, or when nothing
    requires grad, a supported field takes ONE launch (``nfa_ndr_field``, ``nfa_ndr_density``, ``nfa_ndr_warp``): the warp's
    288 KiB of weights stream through the trunk's LDS ring in front of the trunk's own, and nothing between ``(x, t, dir)``, or a
    ray sample and its ray's timestamp, and the outputs exists in memory.  The warped positions and sigma are the composed
    chain's bits; the raw colour carries the vanilla field's one last-bit difference.

    ``fused`` is a bool or ``{"density": bool, "full": bool}`` (:meth:`warp` follows ``"density"``), handed to ``nerf`` as well;
    DESIGN.md, "Fused NDR field", has the measurements.  There is no fused training pass, no gradient towards ``x``, ``t`` or
    the rays through the fused launch, and no inverse warp."""

    def __init__(self, dtype: torch.dtype = torch.float16, generator: Optional[torch.Generator] = None, fused: Union[bool, dict] = True):
        super().__init__()
        self.time_encoder = SinusoidalEncoding(1, 0, 4, True, out_dtype=dtype)
        self.posi_encoder_1 = SinusoidalEncoding(2, 0, 4, True, out_dtype=dtype)
        self.posi_encoder_2 = SinusoidalEncoding(1, 0, 4, True, out_dtype=dtype)
        self._rot_encoder = SinusoidalEncoding(1, 0, 1, False)   # (sin theta, cos theta) in float32
        gen = generator or torch.Generator().manual_seed(1337)
        self.warp_layers_1, self.warp_layers_2 = nn.ModuleList(), nn.ModuleList()
        self.time_layers_1, self.time_layers_2 = nn.ModuleList(), nn.ModuleList()
        for _ in range(NDR_BLOCKS):
            for nets, (n_in, n_out, width, depth, _, _) in ((self.warp_layers_1, NDR_NET1), (self.warp_layers_2, NDR_NET2)):
                net = reference_mlp(n_in, n_out, depth, width, None, dtype=dtype, out_dtype=torch.float32, generator=generator)
                with torch.no_grad():   # output_init=functools.partial(torch.nn.init.uniform_, b=1e-4); the bias is zero already
                    out = net.weight(depth)
                    out.copy_(torch.rand(out.shape, generator=gen) * 1e-4)
                nets.append(net)
            for layers in (self.time_layers_1, self.time_layers_2):
                lin = nn.Linear(NDR_TIME_DIMS, NDR_TIME_WIDTH)   # a holder of weight and bias in nn.Linear layout; never called
                with torch.no_grad():                            # DenseLayer: xavier_uniform_, zero bias
                    bound = math.sqrt(6.0 / (NDR_TIME_DIMS + NDR_TIME_WIDTH))
                    lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen) * 2 - 1) * bound)
                    lin.bias.zero_()
                layers.append(lin)
        self.nerf = VanillaNeRFRadianceField(dtype=dtype, generator=generator, fused=fused)
        self.dtype = dtype
        self.fused = dict(self.nerf.fused)
        self._time_packed = None   # (key, image, bias)
        self._warp_packed = None   # (key, image, bias)

    # ---------------------------------------------------------------- the packed warp

    def _time_tensors(self) -> List[Tensor]:
        return [v for i in range(len(self.time_layers_1)) for lin in (self.time_layers_1[i], self.time_layers_2[i]) for v in (lin.weight, lin.bias)]

    @staticmethod
    def _key(ts: List[Tensor]):
        return tuple((t.data_ptr(), t._version, t.device) for t in ts)

    def _time_image(self):
        """``(image [6, 1024] of dtype, bias [6, 64] float32)`` of the six time layers in ``nfa_ndr_time_features``' layout, rebuilt
        when a master changes."""
        ts = self._time_tensors()
        key = self._key(ts)
        if self._time_packed is None or self._time_packed[0] != key:
            with torch.no_grad():
                w = torch.stack([v.detach() for v in ts[0::2]])                               # [6, 64, 9]
                w = torch.nn.functional.pad(w, (0, 16 - NDR_TIME_DIMS)).to(self.dtype)       # [6, 64, 16]: (m, r) rows, (h, j) columns
                img = w.view(-1, 2, 32, 2, 8).permute(0, 1, 3, 2, 4).reshape(-1, 1024).contiguous()
                bias = torch.stack([v.detach().float() for v in ts[1::2]]).contiguous()
            self._time_packed = (key, img, bias)
        return self._time_packed[1], self._time_packed[2]

    def _warp_image(self):
        """``(image, bias)`` of the whole warp as ``nfa_ndr_field`` takes them: the nets' :class:`FusedMLP` forward images and
        the time layers' in one buffer, one float32 bias block (the way ``_head_image()`` is kept)."""
        nets = [n for i in range(NDR_BLOCKS) for n in (self.warp_layers_1[i], self.warp_layers_2[i])]
        key = self._key([n.params for n in nets] + self._time_tensors())
        if self._warp_packed is None or self._warp_packed[0] != key:
            with torch.no_grad():
                timg, tbias = self._time_image()
                parts, biases = [], []
                for j, net in enumerate(nets):
                    p = net.params
                    parts += [timg[j], net._images(p)[0]]
                    biases.append(tbias[j])
                    for b in net._bias_views(p.detach()):
                        biases.append(torch.nn.functional.pad(b.float(), (0, -b.numel() % 32)))
                img, bias = torch.cat(parts).contiguous(), torch.cat(biases).contiguous()
            assert img.numel() == NDR_IMAGE_ELEMS and bias.numel() == NDR_BIAS_FLOATS
            self._warp_packed = (key, img, bias)
        return self._warp_packed[1], self._warp_packed[2]

    # ---------------------------------------------------------------- the fused launch

    def fused_supported(self, full: bool = True) -> bool:
        """Exactly the reference's warp (three blocks of (82, 1, 2 x 128) and (73, 3, 1 x 128) networks with biases and without a
        skip, twelve ``[64, 9]`` / ``[64]`` time-layer tensors) in front of what :meth:`VanillaNeRFRadianceField.fused_supported`
        lists."""
        desc = lambda nets: [(*n._shape, int(n.bias_enabled), n.skip_mask) for n in nets]
        trunk, head = self.nerf._descs()
        return ndr_field_limits_error(desc(self.warp_layers_1), desc(self.warp_layers_2), [t.shape for t in self._time_tensors()],
                                      trunk, head if full else None) is None

    def _use_fused(self, full: bool, *tensors: Optional[Tensor]) -> bool:
        if not (self.fused["full" if full else "density"] and self.fused_supported(full)):
            return False
        ts = [t for t in tensors if t is not None]
        dev = self.warp_layers_1[0].params.device
        if not (all(t.is_cuda and t.device == dev for t in ts) and all(t.dtype == torch.float32 for t in ts if t.is_floating_point())):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in [*self.parameters(), *ts]))

    def _launch(self, kind: str, n: int, activated: bool = False, positions=None, times=None, dirs=None, rays=None, warped: bool = False,
                rgb_dtype=None, sigma_dtype=None):
        """One fused launch.  ``kind``: ``"full"``: ``(rgb [n, 3], sigma [n], warped [n, 3] or None)``; ``"density"``:
        ``(None, sigma, warped or None)``; ``"warp"``: ``(None, None, warped)``.  ``times``: [n] with ``positions``, [n_rays]
        with ``rays``."""
        full = kind == "full"
        t, h = self.nerf.mlp.trunk, self.nerf.mlp.head
        dev = t.params.device
        sigma = torch.empty(n, dtype=sigma_dtype or self.dtype, device=dev) if kind != "warp" else None
        rgb = torch.empty(n, 3, dtype=rgb_dtype or self.dtype, device=dev) if full else None
        xw = torch.empty(n, 3, dtype=torch.float32, device=dev) if warped or kind == "warp" else None
        if n == 0:
            return rgb, sigma, xw
        keep = [x.contiguous() for x in (rays[:5] if rays is not None else (positions, dirs)) if x is not None]
        times = times.contiguous()
        if rays is not None:
            keep[4] = keep[4] if keep[4].dtype == torch.int64 else keep[4].to(torch.int64)
            inp = B.NGPInput(None, None, *[B.ptr(x) for x in keep], keep[0].shape[0])
        else:
            inp = B.NGPInput(B.ptr(keep[0]), B.ptr(keep[1]) if full else None, None, None, None, None, None, 0)
        elem = B.ELEM_CODES[self.dtype]
        with torch.cuda.device(dev):
            wimg, wbias = self._warp_image()
            if kind == "warp":
                B.call("nfa_ndr_warp", elem, B.ptr(wimg), wimg.numel(), B.ptr(wbias), wbias.numel(), ctypes.byref(inp), B.ptr(times), n,
                       B.ptr(xw), B.stream())
                return rgb, sigma, xw
            tp = t.params
            timg = t._images(tp)[0]
            if full:
                B.call("nfa_ndr_field", elem, t._desc, h._desc, B.ptr(wimg), wimg.numel(), B.ptr(timg), B.ptr(self.nerf._head_image()),
                       B.ptr(wbias), wbias.numel(), t._bias_ptr(tp), h._bias_ptr(h.params), ctypes.byref(inp), B.ptr(times), n, int(activated),
                       B.ptr(sigma), B.ELEM_CODES[sigma.dtype], B.ptr(rgb), B.ELEM_CODES[rgb.dtype], B.ptr(xw) if xw is not None else None,
                       B.stream())
            else:
                B.call("nfa_ndr_density", elem, t._desc, B.ptr(wimg), wimg.numel(), B.ptr(timg), B.ptr(wbias), wbias.numel(), t._bias_ptr(tp),
                       ctypes.byref(inp), B.ptr(times), n, int(activated), B.ptr(sigma), B.ELEM_CODES[sigma.dtype],
                       B.ptr(xw) if xw is not None else None, B.stream())
        return rgb, sigma, xw

    _point_times = staticmethod(TNeRFRadianceField._point_times)

    # ---------------------------------------------------------------- the composed chain

    def _time_features(self, t: Tensor, t_enc: Tensor) -> Tensor:
        """``[n, 6, 64]`` of ``dtype``: row ``2 i + s`` is ``time_layers_{s+1}[i](t_enc)``, FusedMLP's layer arithmetic without an
        activation (half operands, a float32 sum that starts from the bias, one rounding)."""
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("NDRTNeRFRadianceField: no gradient towards the times is implemented")
        ts = self._time_tensors()
        if t.is_cuda and t.dtype == torch.float32:
            with torch.autocast("cuda", enabled=False):
                return _NdrTimeFn.apply(t.contiguous(), t_enc, self, *ts)
        x = t_enc.to(self.dtype).float()
        return torch.stack([(x @ w.to(self.dtype).float().t() + b.float()).to(self.dtype) for w, b in zip(ts[0::2], ts[1::2])], 1)

    def _block(self, x: Tensor, feat: Tensor, i: int) -> Tensor:
        uv, w = x[:, :2], x[:, 2:]
        w = w + self.warp_layers_1[i](torch.cat([self.posi_encoder_1(uv), feat[:, 2 * i]], -1))
        rt = self.warp_layers_2[i](torch.cat([self.posi_encoder_2(w), feat[:, 2 * i + 1]], -1))
        sc = self._rot_encoder(rt[:, :1])
        s, c = sc[:, :1], sc[:, 1:]
        d = uv - rt[:, 1:]
        du, dv = d[:, :1], d[:, 1:]
        return torch.cat([c * du + s * dv, c * dv - s * du, w], -1)

    # ---------------------------------------------------------------- the reference's methods

    def warp(self, x: Tensor, t: Tensor) -> Tensor:
        """The warped positions, float32, in ``x``'s shape (``t``: ``x``'s shape with a last dimension of 1)."""
        if self._point_times(x, t) and self._use_fused(False, x, t):
            return self._launch("warp", x.numel() // 3, positions=x.reshape(-1, 3), times=t.reshape(-1))[2].view(x.shape)
        if not self._point_times(x, t):
            raise ValueError(f"NDRTNeRFRadianceField: t must be {(*x.shape[:-1], 1)} for x {tuple(x.shape)} (got {tuple(t.shape)})")
        p, t1 = x.reshape(-1, 3), t.reshape(-1)
        feat = self._time_features(t1, self.time_encoder(t1.view(-1, 1)))
        p = self._block(p, feat, 0)[:, [1, 2, 0]]
        p = self._block(p, feat, 1)[:, [2, 0, 1]]
        return self._block(p, feat, 2).view(x.shape)

    def query_density(self, x: Tensor, t: Tensor) -> Tensor:
        if self._point_times(x, t) and self._use_fused(False, x, t):
            sigma = self._launch("density", x.numel() // 3, True, positions=x.reshape(-1, 3), times=t.reshape(-1))[1]
            return sigma.view(*x.shape[:-1], 1)
        return self.nerf.query_density(self.warp(x, t))

    def query_opacity(self, x: Tensor, timestamps: Tensor, step_size) -> Tensor:
        idxs = torch.randint(0, len(timestamps), (x.shape[0],), device=x.device)
        return self.query_density(x, timestamps[idxs]) * step_size   # (small densities: 1 - exp(-density * step_size) is the same)

    def forward(self, x: Tensor, t: Tensor, condition: Optional[Tensor] = None):
        if condition is not None and condition.shape == x.shape and self._point_times(x, t) and self._use_fused(True, x, t, condition):
            rgb, sigma, _ = self._launch("full", x.numel() // 3, True, positions=x.reshape(-1, 3), times=t.reshape(-1),
                                         dirs=condition.reshape(-1, 3))
            return rgb.view(*x.shape[:-1], 3), sigma.view(*x.shape[:-1], 1)
        return self.nerf(self.warp(x, t), condition=condition)

    # ---------------------------------------------------------------- the methods in the other fields' shape

    def query_raw(self, positions: Tensor, t: Tensor, directions: Tensor):
        """``(raw_rgbs [..., 3], raw_sigmas [...])`` at world positions and times ``[..., 1]``, before any activation."""
        if positions.shape == directions.shape and self._point_times(positions, t) and self._use_fused(True, positions, t, directions):
            rgb, sigma, _ = self._launch("full", positions.numel() // 3, False, positions=positions.reshape(-1, 3), times=t.reshape(-1),
                                         dirs=directions.reshape(-1, 3))
            return rgb.view(*positions.shape[:-1], 3), sigma.view(positions.shape[:-1])
        return self.nerf.query_raw(self.warp(positions, t), directions)

    def density_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor,
                        timestamps: Tensor) -> Tensor:
        """Densities ``[n]`` at the midpoints of packed ray samples, each at its ray's time (``timestamps`` ``[n_rays, 1]``): a
        trainer's ``sigma_fn``."""
        if timestamps.numel() == rays_o.shape[0] and self._use_fused(False, rays_o, rays_d, t_starts, t_ends, timestamps, ray_indices):
            return self._launch("density", t_starts.numel(), True, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices),
                                times=timestamps.reshape(-1))[1]
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices)
        return self.query_density(s.positions, timestamps.reshape(-1, 1)[ray_indices]).squeeze(-1)

    def query_on_rays(self, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, timestamps: Tensor,
                      raw: bool = True):
        """The field at the midpoints of packed ray samples, each at its ray's time.  ``raw=True``: ``(raw_rgbs [n, 3],
        raw_sigmas [n])``, what :func:`nerfacc_amd.rendering_from_raw` takes; otherwise ``(rgbs [n, 3], sigmas [n])`` activated."""
        if timestamps.numel() == rays_o.shape[0] and self._use_fused(True, rays_o, rays_d, t_starts, t_ends, timestamps, ray_indices):
            return self._launch("full", t_starts.numel(), not raw, rays=(rays_o, rays_d, t_starts, t_ends, ray_indices),
                                times=timestamps.reshape(-1))[:2]
        s = sample_positions(rays_o, rays_d, t_starts, t_ends, ray_indices, dirs="raw")
        t = timestamps.reshape(-1, 1)[ray_indices]
        if raw:
            return self.query_raw(s.positions, t, s.dirs)
        rgb, sigma = self.forward(s.positions, t, s.dirs)
        return rgb, sigma.squeeze(-1)

    def load_reference_state_dict(self, sd: dict) -> None:
        """Takes the reference module's state dict: ``warp_layers_{1,2}.N.hidden_layers.M.*`` and ``.output_layer.*`` (through
        :meth:`FusedMLP.load_reference_state_dict`), ``time_layers_{1,2}.N.output_layer.*``, ``nerf.*`` (through
        :meth:`VanillaNeRFRadianceField.load_reference_state_dict`) and the three encoders' ``scales`` buffers, which must be the
        reference's ``2^k``.  Any other key, a missing key and a wrong shape raise ``ValueError``."""
        who = "NDRTNeRFRadianceField: load_reference_state_dict"
        sd = dict(sd)
        for name in ("time_encoder", "posi_encoder_1", "posi_encoder_2"):
            enc, scales = getattr(self, name), sd.pop(name + ".scales", None)
            if scales is not None:
                want = torch.tensor([2.0 ** k for k in range(enc.min_deg, enc.max_deg)], dtype=torch.float64)
                if scales.numel() != want.numel() or not torch.equal(scales.detach().cpu().double().reshape(-1), want):
                    raise ValueError(f"{who}: '{name}.scales' is not 2^k for k in {enc.min_deg} .. {enc.max_deg - 1}")
        groups = {f"{g}.{i}.": m for g in ("warp_layers_1", "warp_layers_2", "time_layers_1", "time_layers_2")
                  for i, m in enumerate(getattr(self, g))}
        groups["nerf."] = self.nerf
        other = sorted(k for k in sd if not k.startswith(tuple(groups)))
        if other:
            raise ValueError(f"{who}: unexpected keys {other}")
        for prefix, m in groups.items():
            part = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            if not prefix.startswith("time_layers"):
                m.load_reference_state_dict(part)
                continue
            want = {"output_layer.weight": m.weight, "output_layer.bias": m.bias}
            if set(part) != set(want):
                raise ValueError(f"{who}: '{prefix}': missing keys {sorted(set(want) - set(part))}, unexpected keys {sorted(set(part) - set(want))}")
            for k, dst in want.items():
                if tuple(part[k].shape) != tuple(dst.shape):
                    raise ValueError(f"{who}: '{prefix}{k}' is {tuple(part[k].shape)}, expected {tuple(dst.shape)}")
            with torch.no_grad():
                for k, dst in want.items():
                    dst.copy_(part[k])
