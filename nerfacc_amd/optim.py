"""The end of a training step, native: a fused multi-tensor Adam / AdamW with the loss scale and the LR schedule on the device.

The reference's trainers end every step in ``torch.optim.Adam`` under ``GradScaler(2**10)`` and a chained ``LinearLR`` /
``MultiStepLR`` scheduler.  Here the update of ALL parameters of a field -- a hash table of millions of values and a handful of
small MLP tensors alike -- is at most three launches (``csrc/optim.hip``, the ``nfa_optim_*`` entries of
``include/nerfacc_hip.h``), the overflow check of the loss scale never reaches the host, and the schedule is a closed form
evaluated on the device: a step with its update has no host read and replays as one graph (``nerfacc_amd.CapturedStep``).

    scaler = DeviceGradScaler()                                   # torch GradScaler's policy, state on the device
    sched = WarmupMultiStepLR(0.01, 100, (10000, 15000, 18000), 0.33)
    opt = FusedAdam(field.parameters(), lr=1e-2, eps=1e-15, scaler=scaler, schedule=sched, zero_grad=True)
    ...
    scaler.scale(loss).backward()
    opt.step()                                                    # scan, decide, update: no scaler.step / scaler.update

On CPU parameters ``step()`` runs the same formulas as float32 torch ops in the kernel's order, the square root through numpy
(bit for bit the kernel's results: ``tests/optim_reference.py`` restates both).  Not in ``nerfacc_amd.__all__``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _backend as B

CHUNK = 4096                      # include/nerfacc_hip.h: NFA_OPTIM_CHUNK
MAX_GROUPS, MAX_MILESTONES = B.OPTIM_MAX_GROUPS, B.OPTIM_MAX_MILESTONES
FLAG_DECOUPLED, FLAG_SKIP_ZERO_GRAD = 1, 2   # NFA_OPTIM_DECOUPLED, NFA_OPTIM_SKIP_ZERO_GRAD

# The device structs of include/nerfacc_hip.h as numpy record types (the CPU path works on the same buffers through them).
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("n", "<i8"), ("group", "<i4"),
                         ("reserved", "<i4")])
CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("chunk", "<i4")])
SCALER_DTYPE = np.dtype([("scale", "<f4"), ("tracker", "<i4"), ("found", "<i4"), ("reserved", "<i4"), ("skipped", "<i8"),
                         ("reserved2", "<i8")])
GROUP_SCALARS_DTYPE = np.dtype([("step_size", "<f4"), ("bc2_sqrt", "<f4"), ("decay", "<f4"), ("one_minus_beta1", "<f4"), ("beta2", "<f4"),
                                ("one_minus_beta2", "<f4"), ("eps", "<f4"), ("weight_decay", "<f4"), ("flags", "<i4"),
                                ("reserved", "<i4", (3,))])
STATE_DTYPE = np.dtype([("calls", "<i8"), ("step", "<i8"), ("beta1_pow", "<f8", (MAX_GROUPS,)), ("beta2_pow", "<f8", (MAX_GROUPS,)),
                        ("inv_scale", "<f4"), ("skip", "<i4"), ("factor", "<f4"), ("reserved", "<i4"),
                        ("group", GROUP_SCALARS_DTYPE, (MAX_GROUPS,))])
assert TENSOR_DTYPE.itemsize == 48 and SCALER_DTYPE.itemsize == 32 and STATE_DTYPE.itemsize == 1056


def build_work_list(sizes: Sequence[int], chunk: int = CHUNK) -> np.ndarray:
    """The work list of tensors of ``sizes`` elements: records ``(tensor, chunk)`` (``CHUNK_DTYPE``), entry ``(i, c)`` standing
    for elements ``[c * chunk, min(sizes[i], (c + 1) * chunk))`` of tensor ``i``.  Every element of every tensor is in exactly
    one entry and no entry crosses a tensor; an empty tensor has none."""
    parts = []
    for i, n in enumerate(sizes):
        if n < 0:
            raise ValueError(f"build_work_list: tensor {i} has {n} elements")
        k = (int(n) + chunk - 1) // chunk
        if k >= 2 ** 31:
            raise ValueError(f"build_work_list: tensor {i} has {n} elements: more than 2^31 chunks of {chunk}")
        part = np.empty(k, dtype=CHUNK_DTYPE)
        part["tensor"] = i
        part["chunk"] = np.arange(k, dtype=np.int64)
        parts.append(part)
    return np.concatenate(parts) if parts else np.empty(0, dtype=CHUNK_DTYPE)


def _f32(x: float) -> float:
    """x rounded once to float32, as a Python float."""
    return float(np.float32(x))


class WarmupMultiStepLR:
    """The reference trainers' ``ChainedScheduler([LinearLR(start_factor, total_iters=warmup_iters), MultiStepLR(milestones,
    gamma)])`` as a closed form of the number ``t`` of ``step()`` calls made so far (the reference calls ``scheduler.step()``
    once per iteration): ``factor(t) = (start_factor + (1 - start_factor) * min(t, warmup_iters) / warmup_iters) *
    gamma ** #{m in milestones: m <= t}``, the power as repeated multiplication, in double.  Handed to
    ``FusedAdam(schedule=...)`` it is evaluated on the device and multiplies each group's ``lr``.  ``warmup_iters=0``: no
    warm-up.  At most 8 milestones."""

    def __init__(self, start_factor: float = 0.01, warmup_iters: int = 100, milestones: Sequence[int] = (), gamma: float = 0.33):
        if not 0.0 < start_factor <= 1.0:
            raise ValueError(f"WarmupMultiStepLR: start_factor {start_factor}: in (0, 1]")
        if warmup_iters < 0 or int(warmup_iters) != warmup_iters:
            raise ValueError(f"WarmupMultiStepLR: warmup_iters {warmup_iters}: a non-negative integer")
        ms = sorted(int(m) for m in milestones)
        if len(ms) > MAX_MILESTONES:
            raise ValueError(f"WarmupMultiStepLR: {len(ms)} milestones: at most {MAX_MILESTONES}")
        if ms and ms[0] < 0:
            raise ValueError("WarmupMultiStepLR: negative milestone")
        self.start_factor, self.warmup_iters, self.milestones, self.gamma = float(start_factor), int(warmup_iters), tuple(ms), float(gamma)

    def _factor(self, t: int) -> float:
        """The double the device forms (csrc/optim.hip: optim_decide_kernel), operation for operation."""
        f = 1.0
        if self.warmup_iters > 0:
            f = self.start_factor + (1.0 - self.start_factor) * float(min(t, self.warmup_iters)) / float(self.warmup_iters)
        for m in self.milestones:
            if m <= t:
                f = f * self.gamma
        return f

    def factor_at(self, t: int) -> float:
        """The factor at call ``t`` (0-based), rounded once to float32: what the device reports for that step."""
        return _f32(self._factor(int(t)))


class DeviceGradScaler:
    """torch ``GradScaler``'s policy with every piece of its state on the device and no host read: on a non-finite gradient
    the scale backs off (``* backoff_factor``), the tracker resets and the optimiser's step is skipped; otherwise the tracker
    counts and after ``growth_interval`` clean steps the scale grows (``* growth_factor``, kept if finite).
    ``growth_interval=None`` keeps the scale fixed on clean steps (the reference's ``GradScaler(2**10)`` never checks at all).

    ``scale(loss)`` multiplies by the device scale; the scaler is handed to ``FusedAdam(scaler=...)`` (one optimiser per
    scaler), whose ``step()`` does the check, the unscaling and the update of the scale: there is no ``step`` / ``update``
    here.  ``get_scale()`` and ``skipped_steps()`` read the device and are the only calls that do."""

    def __init__(self, init_scale: float = 2.0 ** 10, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: Optional[int] = 2000):
        if not (init_scale > 0 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0):
            raise ValueError("DeviceGradScaler: needs init_scale > 0, growth_factor > 1 and 0 < backoff_factor < 1")
        if growth_interval is not None and growth_interval < 1:
            raise ValueError(f"DeviceGradScaler: growth_interval {growth_interval}: a positive integer or None")
        self.init_scale, self.growth_factor, self.backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self.growth_interval = None if growth_interval is None else int(growth_interval)
        self._buf: Optional[Tensor] = None   # struct nfa_optim_scaler as 4 int64, made on first use
        self._loaded: Optional[np.ndarray] = None   # a state dict loaded before that
        self._owner = None

    def _initial(self) -> np.ndarray:
        if self._loaded is not None:
            return self._loaded.copy()
        rec = np.zeros(1, dtype=SCALER_DTYPE)
        rec["scale"] = self.init_scale
        return rec

    def _buffer(self, device) -> Tensor:
        device = torch.device(device)
        if self._buf is None:
            self._buf = torch.from_numpy(self._initial().view(np.int64).copy()).to(device)
        elif self._buf.device != device:
            raise RuntimeError(f"DeviceGradScaler: its state is on {self._buf.device}, asked for {device}")
        return self._buf

    def _record(self) -> np.ndarray:
        """A host copy of the state (a device read), or the initial state."""
        if self._buf is None:
            return self._initial()
        return self._buf.cpu().numpy().view(SCALER_DTYPE)

    def scale_tensor(self, device) -> Tensor:
        """The float32 ``[1]`` view of the scale on ``device`` (it changes in place as the optimiser steps)."""
        return self._buffer(device).view(torch.float32)[0:1]

    def scale(self, loss: Tensor) -> Tensor:
        return loss * self.scale_tensor(loss.device).to(loss.dtype)[0]

    def get_scale(self) -> float:
        """The current scale (reads the device)."""
        return float(self._record()["scale"][0])

    def growth_tracker(self) -> int:
        """Clean steps since the last change of the scale (reads the device)."""
        return int(self._record()["tracker"][0])

    def skipped_steps(self) -> int:
        """How many optimiser steps were skipped for a non-finite gradient (reads the device)."""
        return int(self._record()["skipped"][0])

    def state_dict(self) -> dict:
        r = self._record()
        return {"scale": float(r["scale"][0]), "growth_tracker": int(r["tracker"][0]), "skipped_steps": int(r["skipped"][0]),
                "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval}

    def load_state_dict(self, sd: dict) -> None:
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = sd["growth_interval"]
        rec = np.zeros(1, dtype=SCALER_DTYPE)
        rec["scale"], rec["tracker"], rec["skipped"] = sd["scale"], sd["growth_tracker"], sd.get("skipped_steps", 0)
        if self._buf is None:
            self._loaded = rec
        else:
            self._buf.copy_(torch.from_numpy(rec.view(np.int64).copy()))   # in place: a captured graph keeps its pointer


def _decide_host(args: B.OptimArgs, state: np.ndarray, scaler: Optional[np.ndarray]) -> None:
    """optim_decide_kernel (csrc/optim.hip) on host records, operation for operation."""
    st = state[0]
    calls, step = int(st["calls"]), int(st["step"])
    found = scaler is not None and int(scaler[0]["found"]) != 0
    scale = np.float32(scaler[0]["scale"]) if scaler is not None else np.float32(1.0)
    factor = 1.0
    if args.warmup_iters > 0:
        factor = args.start_factor + (1.0 - args.start_factor) * float(min(calls, args.warmup_iters)) / float(args.warmup_iters)
    for k in range(args.n_milestones):
        if args.milestones[k] <= calls:
            factor = factor * args.gamma
    if not found:
        for gi in range(args.n_groups):
            g = args.groups[gi]
            b1p, b2p = float(st["beta1_pow"][gi]) * g.beta1, float(st["beta2_pow"][gi]) * g.beta2
            lr = g.lr * factor
            s = st["group"][gi]
            s["step_size"] = np.float32(lr / (1.0 - b1p))
            s["bc2_sqrt"] = np.float32(np.sqrt(1.0 - b2p))
            s["decay"] = np.float32(1.0 - lr * g.weight_decay)
            s["one_minus_beta1"], s["beta2"], s["one_minus_beta2"] = np.float32(1.0 - g.beta1), np.float32(g.beta2), np.float32(1.0 - g.beta2)
            s["eps"], s["weight_decay"], s["flags"] = np.float32(g.eps), np.float32(g.weight_decay), g.flags
            st["beta1_pow"][gi], st["beta2_pow"][gi] = b1p, b2p
    st["calls"] = calls + 1
    st["step"] = step if found else step + 1
    st["inv_scale"] = np.float32(1.0 / float(scale))
    st["skip"] = 1 if found else 0
    st["factor"] = np.float32(factor)
    if scaler is not None:
        sc = scaler[0]
        tracker = int(sc["tracker"])
        if found:
            sc["scale"], sc["tracker"] = scale * np.float32(args.backoff_factor), 0
            sc["skipped"] = int(sc["skipped"]) + 1
        elif args.growth_interval > 0:
            tracker += 1
            if tracker == args.growth_interval:
                with np.errstate(over="ignore"):
                    grown = scale * np.float32(args.growth_factor)
                if np.isfinite(grown):
                    sc["scale"] = grown
                tracker = 0
            sc["tracker"] = tracker
        sc["found"] = 0


def _update_host(p: Tensor, grad: Tensor, m: Tensor, v: Tensor, s, inv_scale: float) -> None:
    """adam_element (csrc/optim.hip) on whole CPU tensors: one float32 torch op per kernel operation, in its order (one of
    them, the square root, numpy's)."""
    S = {k: float(s[k]) for k in ("step_size", "bc2_sqrt", "decay", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "weight_decay")}
    flags = int(s["flags"])
    g = grad.mul(inv_scale)
    pn = p
    if flags & FLAG_DECOUPLED:
        pn = p.mul(S["decay"])
    elif S["weight_decay"] != 0.0:
        g = g.add(p.mul(S["weight_decay"]))
    mn = m.add(g.sub(m).mul(S["one_minus_beta1"]))
    vn = v.mul(S["beta2"]).add(g.mul(g).mul(S["one_minus_beta2"]))
    # (the square root through numpy: torch's CPU sqrt is a vector-library routine that is not correctly rounded -- on random
    # float32 values 0.7 % to 17 % of the results are an ulp off, depending on the host CPU; the kernel's and numpy's are IEEE)
    root = torch.from_numpy(np.sqrt(vn.contiguous().numpy()))
    den = root.div(torch.full_like(vn, S["bc2_sqrt"])).add(S["eps"])
    pn = pn.sub(mn.mul(S["step_size"]).div(den))
    if flags & FLAG_SKIP_ZERO_GRAD:
        keep = grad.mul(inv_scale) == 0
        pn, mn, vn = torch.where(keep, p, pn), torch.where(keep, m, mn), torch.where(keep, v, vn)
    p.copy_(pn)
    m.copy_(mn)
    v.copy_(vn)


class FusedAdam(torch.optim.Optimizer):
    """torch's ``Adam`` (``decoupled_weight_decay=True``: ``AdamW``), non-amsgrad, over all parameters in at most three
    launches per ``step()``: a non-finite scan of the gradients (only with a ``scaler``), a one-wave launch that forms the
    step's scalars on the device, and the update.  Float32 arithmetic, every operation rounded on its own, no atomics: the
    same bits on every run, and on CPU parameters the same bits from torch ops.

    Per group: ``lr`` (read on the host at each ``step()``, so torch's LR schedulers work in eager mode; a captured graph
    keeps the value it was captured with -- use ``schedule`` there), ``betas``, ``eps``, ``weight_decay``,
    ``decoupled_weight_decay`` and ``skip_zero_grad``: an element whose unscaled gradient is exactly 0 keeps its value and
    its moments and is not decayed -- tiny-cuda-nn's rule for hash tables, most of whose fine-level entries no sample of a
    batch touches; 16 bytes of zeros cost their gradient read only.  At most 16 groups.

    Per optimiser: ``zero_grad=True`` makes the update write 0 over each gradient it has used (on a skipped step too); the
    ``.grad`` tensors stay allocated, as graph capture needs, so do not call ``zero_grad(set_to_none=True)`` between steps.
    ``scaler``: a :class:`DeviceGradScaler`; the gradients are unscaled inside the update, and a step with a non-finite
    gradient changes no parameter, moment or counter.  ``schedule``: a :class:`WarmupMultiStepLR`, evaluated on the device
    from the number of ``step()`` calls; its factor multiplies every group's ``lr``.

    Parameters must be float32, contiguous leaf tensors with float32 contiguous gradients, all on one device.  A parameter
    whose ``.grad`` is ``None`` is left out of that step.  There is ONE update counter per optimiser (the bias corrections
    use the count of performed updates): this is torch's per-parameter ``step`` whenever every parameter has a gradient in
    every step, and differs for a parameter that joins later.  ``state_dict()`` / ``load_state_dict()`` use torch Adam's
    layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), so a run moves between ``torch.optim.Adam`` and this class
    both ways; per-parameter steps that differ cannot be loaded.  The device tables are rebuilt (one small copy) only when
    the set of pointers or sizes changes (a parameter, a gradient or a moment tensor replaced, by hand too), so do that
    before a capture: ``CapturedStep``'s warm-up does.

    In a captured graph: the update writes ``params`` in place and ``step()`` bumps their version counters on the host, which
    a replay does not repeat.  A module that caches something derived from its parameters under that counter --
    ``FusedMLP``'s packed weight images -- therefore follows the updates inside a graph only if the rebuild itself was
    captured, i.e. if the cache was stale when the capture ran.  That holds when the captured function ends in ``step()``
    (every warm-up run leaves the cache stale for the next one, the capture included; ``tests/test_optim_gpu.py`` checks
    this case against eager steps bit for bit).  A graph of forward + backward ALONE, with ``step()`` called behind each
    replay, captures the rebuild only if the counter is bumped inside the captured function before the forward
    (``torch.autograd.graph.increment_version(mlp.params)``: a host action, it makes the capture see a stale cache);
    without that the replays keep computing on the images of the capture and the updates never reach the forward.  The
    other way round, EAGER use of such a module after replays of a graph that holds the update (an evaluation pass between
    training steps) needs the same bump first, for the same reason: the replays moved the parameters, not the counter.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, skip_zero_grad: bool = False, zero_grad: bool = False,
                 scaler: Optional[DeviceGradScaler] = None, schedule: Optional[WarmupMultiStepLR] = None):
        if isinstance(lr, Tensor):
            raise TypeError("FusedAdam: lr is a tensor: a Python float (it is read on the host at each step)")
        if not lr >= 0.0:
            raise ValueError(f"FusedAdam: lr {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: betas {betas}")
        if not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError(f"FusedAdam: eps {eps}, weight_decay {weight_decay}")
        if scaler is not None and not isinstance(scaler, DeviceGradScaler):
            raise TypeError("FusedAdam: scaler must be a nerfacc_amd.optim.DeviceGradScaler (torch's GradScaler reads the device)")
        if schedule is not None and not isinstance(schedule, WarmupMultiStepLR):
            raise TypeError("FusedAdam: schedule must be a nerfacc_amd.optim.WarmupMultiStepLR")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay),
                        skip_zero_grad=bool(skip_zero_grad))
        self._state_buf: Optional[Tensor] = None   # struct nfa_optim_state as int64 words
        self._list_key = self._args_key = None   # what the cached plan / argument struct were made from
        self._table = self._work = self._cached_plan = self._args_struct = None
        self._plan_states = []   # (a parameter's state dict, exp_avg, exp_avg_sq, their addresses) of the cached plan
        super().__init__(params, defaults)
        self.fused_zero_grad = bool(zero_grad)
        self.scaler, self.schedule = scaler, schedule
        if scaler is not None:
            if scaler._owner is not None:
                raise ValueError("FusedAdam: this DeviceGradScaler already belongs to another optimiser (each step() advances it)")
            scaler._owner = self

    # ------------------------------------------------------------------ parameters
    def add_param_group(self, param_group) -> None:
        ps = param_group["params"]
        for j, p in enumerate([ps] if isinstance(ps, Tensor) else list(ps)):
            p = p[1] if isinstance(p, tuple) else p
            if isinstance(p, Tensor) and not p.is_leaf:
                raise ValueError(f"FusedAdam: parameter {j} of group {len(self.param_groups)} (shape {tuple(p.shape)}) is not a leaf tensor")
        super().add_param_group(param_group)
        self._list_key = None
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"FusedAdam: {len(self.param_groups)} param groups: at most {MAX_GROUPS}")
        gi = len(self.param_groups) - 1
        for j, p in enumerate(self.param_groups[gi]["params"]):
            self._check_param(p, gi, j)

    def _name(self, gi: int, j: int, p: Tensor) -> str:
        names = self.param_groups[gi].get("param_names")
        return (f"parameter '{names[j]}'" if names else f"parameter {j} of group {gi}") + f" (shape {tuple(p.shape)})"

    def _check_param(self, p: Tensor, gi: int, j: int) -> None:
        if p.dtype != torch.float32:
            raise TypeError(f"FusedAdam: {self._name(gi, j, p)} is {p.dtype}: float32 parameters only")
        if not p.is_contiguous():
            raise ValueError(f"FusedAdam: {self._name(gi, j, p)} is not contiguous")

    def _check_grad(self, p: Tensor, gi: int, j: int) -> None:
        g = p.grad
        if g.is_sparse or g.dtype != torch.float32:
            raise TypeError(f"FusedAdam: the gradient of {self._name(gi, j, p)} is {'sparse' if g.is_sparse else g.dtype}: dense float32 only")
        if not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
            raise ValueError(f"FusedAdam: the gradient of {self._name(gi, j, p)} must be contiguous, of the parameter's shape, on its device")
        self._check_param(p, gi, j)

    def _device(self) -> torch.device:
        devs = {p.device for g in self.param_groups for p in g["params"]}
        if len(devs) != 1:
            raise ValueError(f"FusedAdam: the parameters must be on one device, got {sorted(map(str, devs))}")
        return next(iter(devs))

    # ------------------------------------------------------------------ device state
    def _state_buffer(self, device) -> Tensor:
        if self._state_buf is None or self._state_buf.device != device:
            rec = np.zeros(1, dtype=STATE_DTYPE) if self._state_buf is None else self._state_buf.cpu().numpy().view(STATE_DTYPE).copy()
            if self._state_buf is None:
                rec["beta1_pow"], rec["beta2_pow"] = 1.0, 1.0
            self._state_buf = torch.from_numpy(rec.view(np.int64).copy()).to(device)
        return self._state_buf

    def _state_record(self) -> np.ndarray:
        """A host copy of struct nfa_optim_state (a device read)."""
        return self._state_buffer(self._device()).cpu().numpy().view(STATE_DTYPE)

    def performed_steps(self) -> int:
        """Updates performed so far: ``step()`` calls minus the skipped ones (reads the device)."""
        return int(self._state_record()["step"][0])

    def schedule_calls(self) -> int:
        """``step()`` calls so far, the schedule's ``t`` (reads the device)."""
        return int(self._state_record()["calls"][0])

    def last_factor(self) -> float:
        """The schedule factor of the last ``step()`` (reads the device)."""
        return float(self._state_record()["factor"][0])

    def _args(self) -> B.OptimArgs:
        a = B.OptimArgs()
        a.n_groups = len(self.param_groups)
        for gi, g in enumerate(self.param_groups):
            if isinstance(g["lr"], Tensor):
                raise TypeError("FusedAdam: a group's lr is a tensor: a Python float (it is read on the host at each step)")
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam: amsgrad and maximize are not implemented")
            flags = (FLAG_DECOUPLED if g["decoupled_weight_decay"] else 0) | (FLAG_SKIP_ZERO_GRAD if g["skip_zero_grad"] else 0)
            a.groups[gi] = B.OptimGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                                        flags, 0)
        sch = self.schedule
        a.start_factor, a.gamma, a.warmup_iters = (sch.start_factor, sch.gamma, sch.warmup_iters) if sch else (1.0, 1.0, 0)
        a.n_milestones = len(sch.milestones) if sch else 0
        for k in range(a.n_milestones):
            a.milestones[k] = sch.milestones[k]
        sc = self.scaler
        if sc is not None:
            a.growth_factor, a.backoff_factor, a.growth_interval = sc.growth_factor, sc.backoff_factor, sc.growth_interval or 0
        return a

    # ------------------------------------------------------------------ the step
    def _entries(self):
        """(p, exp_avg, exp_avg_sq, group) of every parameter with a gradient, checked, its state made on first use."""
        out = []
        for gi, group in enumerate(self.param_groups):
            for j, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                self._check_grad(p, gi, j)
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)   # torch Adam's key; the live count is on the device
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if p.numel():
                    out.append((p, st["exp_avg"], st["exp_avg_sq"], gi))
        return out

    def _lists(self, entries, device) -> None:
        """The device table and work list of ``entries`` (one small host-to-device copy each)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam: the set of parameter, gradient or state tensors changed inside a graph capture; run "
                               "step() once before capturing (CapturedStep's warm-up does)")
        table = np.zeros(len(entries), dtype=TENSOR_DTYPE)
        for i, (p, m, v, gi) in enumerate(entries):
            table[i] = (p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi, 0)
        work = build_work_list([p.numel() for p, _, _, _ in entries])
        self._table = torch.from_numpy(table.view(np.int64).reshape(-1).copy()).to(device)
        self._work = torch.from_numpy(work.view(np.int64).reshape(-1).copy()).to(device)

    def _plan(self):
        """(device, entries) of this step.  The checks, the state look-ups and the device lists are redone only when a
        parameter or gradient tensor changed (address, size, dtype, layout), a group was added or a state dict loaded: a
        step is a few microseconds of host work otherwise.  A moment tensor put into ``self.state`` by hand, or moved to
        other memory, is seen too: the plan remembers each parameter's state dict, its two tensors and their addresses
        (replacing a whole ``self.state[p]`` dict is what ``load_state_dict`` is for).
        (Nothing here keeps a gradient tensor alive.)"""
        key = tuple((p.data_ptr(), g.data_ptr(), g.numel(), g.dtype, g.is_contiguous())
                    for group in self.param_groups for p in group["params"] for g in (p.grad,) if g is not None)
        state = self.state
        if key != self._list_key or any(st.get("exp_avg") is not m or st.get("exp_avg_sq") is not v or m.data_ptr() != mp
                                        or v.data_ptr() != vp for st, m, v, mp, vp in self._plan_states):
            device = self._device()
            entries = self._entries()
            if device.type != "cpu":
                B.require_device(*(p for p, _, _, _ in entries))
                self._lists(entries, device)
            self._cached_plan = (device, entries)
            self._plan_states = [(state[p], m, v, m.data_ptr(), v.data_ptr()) for p, m, v, _ in entries]
            self._list_key = key
        return self._cached_plan

    def _cached_args(self) -> B.OptimArgs:
        sc = self.scaler
        key = (tuple((g["lr"], g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"], g["skip_zero_grad"])
                     for g in self.param_groups),
               None if (sch := self.schedule) is None else (sch.start_factor, sch.warmup_iters, sch.milestones, sch.gamma),
               None if sc is None else (sc.growth_factor, sc.backoff_factor, sc.growth_interval))
        if key != self._args_key:
            self._args_struct, self._args_key = self._args(), key
        return self._args_struct

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        device, entries = self._plan()
        state = self._state_buffer(device)
        scaler = None if self.scaler is None else self.scaler._buffer(device)
        args = self._cached_args()
        if device.type == "cpu":
            srec = None if scaler is None else scaler.numpy().view(SCALER_DTYPE)
            rec = state.numpy().view(STATE_DTYPE)
            if srec is not None and any(not bool(torch.isfinite(p.grad).all()) for p, _, _, _ in entries):
                srec["found"] = 1
            _decide_host(args, rec, srec)
            for p, m, v, gi in entries:
                if not rec["skip"][0]:
                    _update_host(p, p.grad, m, v, rec["group"][0][gi], float(rec["inv_scale"][0]))
                if self.fused_zero_grad:
                    p.grad.zero_()
            return loss
        n, table, work, f32 = len(entries), B.ptr(self._table), B.ptr(self._work), B.ELEM_CODES[torch.float32]
        n_chunks = self._work.numel()

        def launch():
            s = B.stream()
            if scaler is not None:
                B.call("nfa_optim_scan", f32, table, n, work, n_chunks, B.ptr(scaler), s)
            B.call("nfa_optim_decide", C.byref(args), B.ptr(state), B.ptr(scaler), s)
            B.call("nfa_optim_update", f32, table, n, work, n_chunks, B.ptr(state), int(self.fused_zero_grad), s)

        if torch.cuda.current_device() == device.index:
            launch()
        else:
            with torch.cuda.device(device):
                launch()
        # the kernels wrote behind torch's back: FusedMLP keys its packed images on the version counter
        torch.autograd.graph.increment_version([p for p, _, _, _ in entries])
        return loss

    # ------------------------------------------------------------------ torch Adam's state dict
    def state_dict(self) -> dict:
        rec = self._state_record()
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(float(rec["step"][0]), dtype=torch.float32)
        sd = super().state_dict()
        sd["schedule_calls"] = int(rec["calls"][0])
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam: a state dict with amsgrad or maximize cannot be loaded")
        steps = {float(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam: the per-parameter steps differ ({sorted(steps)}): this optimiser keeps one update counter")
        step = int(steps.pop()) if steps else 0
        device = self._device()
        rec = np.zeros(1, dtype=STATE_DTYPE)
        rec["step"], rec["calls"] = step, int(state_dict.get("schedule_calls", step))
        for gi, g in enumerate(self.param_groups):
            b1p = b2p = 1.0
            for _ in range(step):   # the device's running products
                b1p, b2p = b1p * float(g["betas"][0]), b2p * float(g["betas"][1])
            rec["beta1_pow"][0][gi], rec["beta2_pow"][0][gi] = b1p, b2p
        rec["beta1_pow"][0][len(self.param_groups):] = 1.0
        rec["beta2_pow"][0][len(self.param_groups):] = 1.0
        new = torch.from_numpy(rec.view(np.int64).copy())
        if self._state_buf is None or self._state_buf.device != device:
            self._state_buf = new.to(device)
        else:
            self._state_buf.copy_(new)   # in place: a captured graph keeps its pointer
        for p, st in self.state.items():
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st and (st[k].dtype != torch.float32 or not st[k].is_contiguous() or st[k].shape != p.shape):
                    st[k] = st[k].to(torch.float32).reshape(p.shape).contiguous()
        self._list_key = None
