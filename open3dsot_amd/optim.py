"""Adam for the trackers on flat buffers: one kernel launch per step.

`MatchingBaseModel.configure_optimizers` (models/base_model.py:28-36) builds `torch.optim.Adam(betas=(0.5, 0.999),
eps=1e-6)`.  On this model -- 76 small parameter tensors, 1.48 M values -- torch's fused multi-tensor Adam takes three
launches and 0.13 ms per step.  `FlatAdam` is the same update rule with every parameter and both moments as views of
flat buffers and the gradients read where autograd left them (device job table, csrc/heads.hip::adam_step_kernel):
one ~10 us launch.  `state_dict()` has torch.optim.Adam's layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so
checkpoints are interchangeable with the reference's optimizer.

`FlatSGD` is the reference's other optimizer (`optimizer: sgd`, models/base_model.py:29-31: momentum 0.9) on the same layout
(csrc/optim.hip::sgd_step_kernel), with torch.optim.SGD's `state_dict()` (`momentum_buffer` per parameter).

Both take `grad_clip` (main.py:85 `gradient_clip_val`, norm clipping): when it is a positive number, `step()` first runs the two
launches of `o3d_grad_norm` over the same job table and then the update on g * coefficient, the coefficient read from device
memory (`o3d_adam_step_scaled`, `o3d_sgd_step`): no host synchronisation.  UNLIKE `torch.nn.utils.clip_grad_norm_`, `p.grad`
is left unclipped -- only the update sees the scale -- so a caller that reads the gradients after the step reads the raw ones.
With `grad_clip` None or 0 the step is the unclipped one: no norm launch, no allocation.
"""
import torch
from torch.autograd.graph import increment_version

from . import capi


class _FlatClip:
    """what the flat optimizers share: the re-homing check, the cached device job table and the clipping launches"""

    grad_clip = None
    _norm = None            # (partials, out) of o3d_grad_norm, allocated at the first clipped step
    _norm_ran = False
    _all_key, _all_table = None, None

    def _check_homed(self):
        base = self._flat.data_ptr()
        name = type(self).__name__
        for p, (off, _) in self._offsets.items():
            # every parameter must still be a view of the flat buffer: a second optimizer built on the same model,
            # module.to(dtype) or any `p.data = ...` re-homes it and this update would silently go nowhere
            if p.data_ptr() != base + 4 * off:
                raise RuntimeError("%s: a parameter no longer lives in this optimizer's flat buffer (re-homed by "
                                   "another %s, module.to(...) or a p.data assignment); rebuild the optimizer"
                                   % (name, name))

    def _job_table(self, gi, live, grads):
        key = (gi,) + tuple(g.data_ptr() for g in grads)
        if self._key is None or self._key.get(gi) != key:
            # (eager autograd hands out new gradient tensors every step: one small upload; a replayed HIP graph
            # writes the same buffers every step: the table is built once)
            rows = [[g.data_ptr(), self._offsets[p][0], self._offsets[p][1]] for p, g in zip(live, grads)]
            self._key = dict(self._key or {})
            self._key[gi] = key
            self._table = dict(self._table or {})
            self._table[gi] = torch.tensor(rows, dtype=torch.int64, device=self._flat.device)
        return self._table[gi]

    def _live(self):
        """[(group index, group, live parameters, their contiguous gradients, job table)] of the groups with a gradient"""
        out = []
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]
            if live:
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in live]
                out.append((gi, group, live, grads, self._job_table(gi, live, grads)))
        return out

    def _clip_scale(self, lib, work, stream):
        """grad_clip set: launch o3d_grad_norm over the gradients of ALL groups (clip_grad_norm_'s one total norm) -> the
        device address of the coefficient; else None"""
        if not self.grad_clip:
            self._norm_ran = False
            return None
        if not float(self.grad_clip) > 0.0:
            raise ValueError("%s: grad_clip must be None, 0 or a positive number, got %r" % (type(self).__name__, self.grad_clip))
        if len(work) == 1:
            tab = work[0][4]
        else:
            key = tuple(self._key[w[0]] for w in work)
            if self._all_key != key:
                self._all_key, self._all_table = key, torch.cat([w[4] for w in work])
            tab = self._all_table
        slices = capi.CONSTANTS["O3D_NORM_SLICES"]
        dev = self._flat.device
        if self._norm is None or self._norm[0].numel() < tab.shape[0] * slices:
            self._norm = (torch.empty(tab.shape[0] * slices, dtype=torch.float64, device=dev),
                          torch.zeros(2, dtype=torch.float32, device=dev))
        partials, out = self._norm
        capi.check(lib.o3d_grad_norm(tab.data_ptr(), tab.shape[0], float(self.grad_clip), partials.data_ptr(),
                                     out.data_ptr(), stream), "grad_norm")
        self._norm_ran = True
        return out.data_ptr() + 4

    def last_grad_norm(self):
        """the total gradient norm the last step() clipped by, BEFORE clipping: a 0-d device tensor (a view of the buffer
        the next clipped step overwrites; no synchronisation) -- or None when that step did not clip"""
        return self._norm[1][0] if self._norm_ran else None

    def last_clip_coef(self):
        """min(1, grad_clip / (norm + 1e-6)) of the last step(), like last_grad_norm()"""
        return self._norm[1][1] if self._norm_ran else None


class FlatAdam(_FlatClip, torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_clip=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        ps = [p for g in self.param_groups for p in g["params"]]
        if not ps or not all(p.is_cuda and p.dtype == torch.float32 for p in ps):
            raise ValueError("FlatAdam: fp32 CUDA parameters only (use torch.optim.Adam elsewhere)")
        dev = ps[0].device
        total = sum(p.numel() for p in ps)
        self._flat = torch.empty(total, device=dev, dtype=torch.float32)
        self._m = torch.zeros(total, device=dev, dtype=torch.float32)
        self._v = torch.zeros(total, device=dev, dtype=torch.float32)
        self._step = torch.zeros((), dtype=torch.float32)          # shared by every parameter (torch keeps one each)
        self._offsets = {}
        off = 0
        with torch.no_grad():
            for p in ps:
                n = p.numel()
                view = self._flat[off:off + n].view_as(p)
                view.copy_(p)
                p.data = view                       # the parameter now lives in the flat buffer
                self.state[p] = {"step": self._step, "exp_avg": self._m[off:off + n].view_as(p),
                                 "exp_avg_sq": self._v[off:off + n].view_as(p)}
                self._offsets[p] = (off, n)
                off += n
        self._key, self._table = None, None
        self.grad_clip = grad_clip

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lib = capi.load()
        self._check_homed()
        self._step += 1
        t = float(self._step)
        dev = self._flat.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            work = self._live()
            scale = self._clip_scale(lib, work, stream) if work else None
            keep = []
            for gi, group, live, grads, tab in work:
                b1, b2 = group["betas"]
                args = (tab.data_ptr(), tab.shape[0], self._flat.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                        float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                        1.0 - b1 ** t, 1.0 - b2 ** t)
                if scale is None:
                    capi.check(lib.o3d_adam_step(*args, stream), "adam_step")
                else:
                    capi.check(lib.o3d_adam_step_scaled(*args, scale, stream), "adam_step_scaled")
                keep.append(grads)
                # the kernel wrote the parameters through the flat buffer: bump their version counters like an in-place
                # torch op would, so the forward/backward guards of the fused operators and the eval-constant cache see it
                increment_version(live)
            if keep:
                self._keep = keep                   # the launches read them: alive until the next step
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        missing = [p for p in self._offsets if not self.state.get(p)]
        if missing and len(missing) < len(self._offsets):
            # torch.optim.Adam omits parameters that never received a gradient and would start them at step 0 on their first
            # update; FlatAdam keeps ONE step counter for all parameters, so their bias correction continues at the
            # checkpoint's step -- the updates of exactly those parameters differ from the reference optimizer's after resume
            import warnings
            warnings.warn("FlatAdam.load_state_dict: the checkpoint holds state for %d of %d parameters; the others get zero "
                          "moments but share the checkpoint's step counter (torch.optim.Adam would restart them at step 0)"
                          % (len(self._offsets) - len(missing), len(self._offsets)), RuntimeWarning, stacklevel=2)
        with torch.no_grad():                       # back into the flat buffers (the base class swapped in copies)
            step = None
            for p, (off, n) in self._offsets.items():
                st = self.state.get(p)
                if not st:          # e.g. a torch.optim.Adam checkpoint taken before its first step: fresh moments
                    self._m[off:off + n].zero_()
                    self._v[off:off + n].zero_()
                    self.state[p] = {"step": self._step, "exp_avg": self._m[off:off + n].view_as(p),
                                     "exp_avg_sq": self._v[off:off + n].view_as(p)}
                    continue
                self._m[off:off + n].view_as(p).copy_(st["exp_avg"])
                self._v[off:off + n].view_as(p).copy_(st["exp_avg_sq"])
                step = float(st["step"]) if step is None else step
                st["exp_avg"], st["exp_avg_sq"] = self._m[off:off + n].view_as(p), self._v[off:off + n].view_as(p)
            self._step.fill_(step if step is not None else 0.0)
            for st in self.state.values():
                st["step"] = self._step
        self._key = self._table = None


class FlatSGD(_FlatClip, torch.optim.Optimizer):
    """torch.optim.SGD with momentum (dampening 0, no Nesterov, no maximize) on flat buffers: one launch per step.  The
    param_groups carry torch.optim.SGD's keys, so a state_dict goes either way between the two."""

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0, grad_clip=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None))
        ps = [p for g in self.param_groups for p in g["params"]]
        if not ps or not all(p.is_cuda and p.dtype == torch.float32 for p in ps):
            raise ValueError("FlatSGD: fp32 CUDA parameters only (use torch.optim.SGD elsewhere)")
        dev = ps[0].device
        total = sum(p.numel() for p in ps)
        self._flat = torch.empty(total, device=dev, dtype=torch.float32)
        self._buf = torch.zeros(total, device=dev, dtype=torch.float32)
        self._offsets = {}
        off = 0
        with torch.no_grad():
            for p in ps:
                n = p.numel()
                view = self._flat[off:off + n].view_as(p)
                view.copy_(p)
                p.data = view                       # the parameter now lives in the flat buffer
                self.state[p] = {"momentum_buffer": self._buf[off:off + n].view_as(p)}
                self._offsets[p] = (off, n)
                off += n
        self._key, self._table = None, None
        self.grad_clip = grad_clip

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lib = capi.load()
        self._check_homed()
        dev = self._flat.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            work = self._live()
            scale = self._clip_scale(lib, work, stream) if work else None
            keep = []
            for gi, group, live, grads, tab in work:
                if group.get("dampening", 0) != 0 or group.get("nesterov") or group.get("maximize"):
                    raise ValueError("FlatSGD: dampening, nesterov and maximize are not implemented (the reference uses none)")
                capi.check(lib.o3d_sgd_step(tab.data_ptr(), tab.shape[0], self._flat.data_ptr(), self._buf.data_ptr(),
                                            float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]),
                                            scale, stream), "sgd_step")
                keep.append(grads)
                increment_version(live)             # as in FlatAdam.step
            if keep:
                self._keep = keep                   # the launches read them: alive until the next step
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        with torch.no_grad():                       # back into the flat buffer (the base class swapped in copies)
            for p, (off, n) in self._offsets.items():
                view = self._buf[off:off + n].view_as(p)
                buf = (self.state.get(p) or {}).get("momentum_buffer")
                if buf is None:     # torch.optim.SGD before the parameter's first step: its first step sets buf = g
                    view.zero_()
                else:
                    view.copy_(buf)
                self.state[p] = {"momentum_buffer": view}
        self._key = self._table = None


def make_adam(params, lr, weight_decay, betas=(0.5, 0.999), eps=1e-6):
    """the reference's Adam (models/base_model.py:32-33): FlatAdam when every parameter is an fp32 GPU tensor, else
    torch.optim.Adam (the CPU mirror used by the tests)"""
    params = list(params)
    if params and all(q.is_cuda and q.dtype == torch.float32 for q in params) and _ON["on"]:
        return FlatAdam(params, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
    return torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps,
                            fused=True if params and all(q.is_cuda for q in params) else None)


def make_sgd(params, lr, weight_decay, momentum=0.9):
    """the reference's SGD (models/base_model.py:29-31): FlatSGD when every parameter is an fp32 GPU tensor, else
    torch.optim.SGD (the CPU mirror used by the tests)"""
    params = list(params)
    if params and all(q.is_cuda and q.dtype == torch.float32 for q in params) and _ON["on"]:
        return FlatSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)


_ON = {"on": True}      # set_flat_adam(False): torch.optim.Adam / SGD, for the tests that compare the update rules


def set_flat_adam(enabled):
    _ON["on"] = bool(enabled)
