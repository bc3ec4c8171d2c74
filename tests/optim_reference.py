"""The fused optimiser's step restated in numpy: THE written-down operation order of csrc/optim.hip (include/nerfacc_hip.h lists
it too).  Everything per element is float32 with one rounding per operation; the step's scalars are double expressions rounded
to float32 once; beta^t are running products in double.  The tests hold the CPU torch path and the kernels to these bits.

    ref = RefAdam([p0, p1, ...], groups=[dict(lr=, betas=, eps=, weight_decay=, decoupled=, skip_zero_grad=, params=[0, 1])],
                  scaler=RefScaler(...), schedule=dict(start_factor=, warmup_iters=, milestones=, gamma=), zero_grad=False)
    ref.step([g0, None, ...])      # gradients as float32 arrays (None: the parameter sits this step out); updates ref.p / m / v
"""
import numpy as np

f32 = np.float32


def schedule_factor(t, start_factor=1.0, warmup_iters=0, milestones=(), gamma=1.0):
    """The schedule's factor at call t, in double (the caller rounds)."""
    f = 1.0
    if warmup_iters > 0:
        f = start_factor + (1.0 - start_factor) * float(min(t, warmup_iters)) / float(warmup_iters)
    for m in sorted(milestones):
        if m <= t:
            f = f * gamma
    return f


class RefScaler:
    """torch.amp.GradScaler's policy on float32 / int values."""

    def __init__(self, init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale, self.tracker, self.skipped = f32(init_scale), 0, 0
        self.growth_factor, self.backoff_factor, self.growth_interval = f32(growth_factor), f32(backoff_factor), growth_interval

    def advance(self, found):
        if found:
            self.scale, self.tracker, self.skipped = f32(self.scale * self.backoff_factor), 0, self.skipped + 1
        elif self.growth_interval:
            self.tracker += 1
            if self.tracker == self.growth_interval:
                with np.errstate(over="ignore"):
                    grown = f32(self.scale * self.growth_factor)
                if np.isfinite(grown):
                    self.scale = grown
                self.tracker = 0


def adam_elements(p, grad, m, v, *, inv_scale, step_size, bc2_sqrt, decay, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay,
                  decoupled, skip_zero_grad):
    """adam_element of csrc/optim.hip on float32 arrays; returns the new (p, m, v).  All scalars are float32."""
    assert all(a.dtype == f32 for a in (p, grad, m, v))
    with np.errstate(all="ignore"):
        g = grad * inv_scale
        g0 = g
        pn = p
        if decoupled:
            pn = p * decay
        elif weight_decay != 0:
            g = g + weight_decay * p
        mn = m + one_minus_beta1 * (g - m)
        vn = beta2 * v + one_minus_beta2 * (g * g)
        pn = pn - (step_size * mn) / (np.sqrt(vn) / bc2_sqrt + eps)
    assert pn.dtype == f32 and mn.dtype == f32 and vn.dtype == f32
    if skip_zero_grad:
        keep = g0 == 0
        pn, mn, vn = np.where(keep, p, pn), np.where(keep, m, mn), np.where(keep, v, vn)
    return pn, mn, vn


class RefAdam:
    def __init__(self, params, groups, scaler=None, schedule=None, zero_grad=False):
        self.p = [np.array(p, dtype=f32) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.groups = groups
        self.scaler, self.schedule, self.zero_grad = scaler, schedule or {}, zero_grad
        self.calls = self.step_count = 0
        self.pow = [[1.0, 1.0] for _ in groups]   # beta1^step, beta2^step: running products in double
        self.last_factor = self.last_skip = None

    def step(self, grads):
        """grads: one float32 array or None per parameter; with zero_grad the arrays are zeroed in place."""
        live = [g for g in grads if g is not None]
        found = self.scaler is not None and any(not np.isfinite(g).all() for g in live)
        factor = schedule_factor(self.calls, **self.schedule)
        inv_scale = f32(1.0 / float(self.scaler.scale)) if self.scaler is not None else f32(1.0)
        self.calls += 1
        self.last_factor, self.last_skip = f32(factor), found
        if self.scaler is not None:
            self.scaler.advance(found)
        if not found:
            self.step_count += 1
            for gi, G in enumerate(self.groups):
                b1, b2 = float(G["betas"][0]), float(G["betas"][1])
                self.pow[gi][0] *= b1
                self.pow[gi][1] *= b2
                lr = float(G["lr"]) * factor
                wd = float(G.get("weight_decay", 0.0))
                s = dict(inv_scale=inv_scale, step_size=f32(lr / (1.0 - self.pow[gi][0])), bc2_sqrt=f32(np.sqrt(1.0 - self.pow[gi][1])),
                         decay=f32(1.0 - lr * wd), one_minus_beta1=f32(1.0 - b1), beta2=f32(b2), one_minus_beta2=f32(1.0 - b2),
                         eps=f32(G["eps"]), weight_decay=f32(wd), decoupled=bool(G.get("decoupled", False)),
                         skip_zero_grad=bool(G.get("skip_zero_grad", False)))
                for i in G["params"]:
                    if grads[i] is None or grads[i].size == 0:
                        continue
                    self.p[i], self.m[i], self.v[i] = adam_elements(self.p[i], grads[i], self.m[i], self.v[i], **s)
        if self.zero_grad:
            for g in live:
                g[...] = 0
