"""``FusedAdam``: ``torch.optim.Adam`` (L2 weight decay added to the gradient, the only form the reference's trainer uses,
gnn/trainer.py:70) whose step is ONE kernel launch for every parameter of the model (csrc/optim.hip) instead of torch's seven
``multi_tensor_apply`` launches.

Drop-in for the optimizer of a training loop: constructor arguments, ``param_groups`` and the per-parameter state (``exp_avg``,
``exp_avg_sq``, ``step``) are torch's, so torch's learning-rate schedulers drive it by writing ``group['lr']`` and
``state_dict()`` / ``load_state_dict()`` exchange checkpoints with ``torch.optim.Adam`` in both directions.

The kernel writes the parameters through raw pointers; every weight-derived cache of this package (bf16 / f16 weight planes, the
layers' operand images, magnitude bounds) is keyed on a tensor's version counter, so ``step()`` bumps the counter of every
parameter it updated."""
from __future__ import annotations

import torch

from . import ops

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a Python number (a tensor lr would be read back from the device every step)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # torch.optim.Adam's keys in its order: a state_dict of either optimizer loads into the other.  foreach / fused select
        # between torch's own implementations and mean nothing here; they are kept for the layout only.
        defaults = {"lr": lr, "betas": tuple(float(b) for b in betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": amsgrad,
                    "maximize": maximize, "foreach": foreach, "capturable": capturable, "differentiable": differentiable,
                    "fused": fused, "decoupled_weight_decay": decoupled_weight_decay}
        super().__init__(params, defaults)
        self._check_groups()
        self.launches_last_step = 0

    def _check_groups(self) -> None:
        for group in self.param_groups:
            for flag in _UNSUPPORTED:
                if group.get(flag, False):
                    raise ValueError(f"FusedAdam does not implement {flag}=True (plain Adam with L2 weight decay only)")

    def __setstate__(self, state):
        super().__setstate__(state)
        defaults = getattr(self, "defaults", {})
        for group in self.param_groups:
            for key in ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
                group.setdefault(key, defaults.get(key))
            for p in group["params"]:
                st = self.state.get(p)
                if st and not isinstance(st["step"], int):       # torch.optim.Adam keeps the count as a float32 tensor
                    st["step"] = int(round(float(st["step"])))
        self._check_groups()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # tensors that share (device, betas, eps) share launches; lr and weight decay travel per tensor
        buckets = {}
        for group in self.param_groups:
            for flag in _UNSUPPORTED:
                if group[flag]:
                    raise ValueError(f"FusedAdam does not implement {flag}=True (plain Adam with L2 weight decay only)")
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise ValueError("FusedAdam: lr must be a Python number")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue                                     # torch: no moment decay and no step increment either
                if g.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError(f"FusedAdam updates contiguous float32 parameters on the GPU (got {ops._describe(p)})")
                if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                    raise TypeError(f"FusedAdam needs a contiguous float32 gradient next to its parameter (got {ops._describe(g)} "
                                    f"for {ops._describe(p)})")
                key = (p.device.index, float(beta1), float(beta2), float(group["eps"]))
                buckets.setdefault(key, []).append((p, g, float(lr), float(group["weight_decay"])))
        # nothing has been changed up to here: a refused tensor leaves every step count and moment as it was
        self.launches_last_step = 0
        for (index, beta1, beta2, eps), items in buckets.items():
            ps, gs, ms, vs, steps, lrs, wds = [], [], [], [], [], [], []
            for p, g, lr, wd in items:
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                ps.append(p); gs.append(g); ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"])
                steps.append(st["step"]); lrs.append(lr); wds.append(wd)
            if index == torch.cuda.current_device():
                self.launches_last_step += ops.adam_step(ps, gs, ms, vs, steps, lrs, wds, beta1, beta2, eps)
            else:
                with torch.cuda.device(index):
                    self.launches_last_step += ops.adam_step(ps, gs, ms, vs, steps, lrs, wds, beta1, beta2, eps)
            # the kernel wrote through raw pointers: caches keyed on Tensor._version must see these parameters as changed
            torch.autograd.graph.increment_version(ps)
        return loss
