"""The parameter update of a training iteration on the device: ``SplatAdam`` is ``torch.optim.Adam`` (reference
scene/gaussian_model.py:130-139 builds ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` over six tensors, train.py:314-322 steps it)
with the step itself as ONE kernel launch for every tensor that has a gradient (``sr_adam_step``, csrc/adam.hip).

``param_groups`` and ``state`` have exactly torch.optim.Adam's layout -- per parameter ``step`` (a float32 scalar on the
host), ``exp_avg`` and ``exp_avg_sq``, created on the first step in which the parameter has a gradient -- so the reference's
optimizer surgery (``replace_tensor_to_optimizer``, ``_prune_optimizer``, ``cat_tensors_to_optimizer``),
``splatfields_amd.densify.densify_and_prune`` and ``update_learning_rate`` work on it unchanged, and ``state_dict()`` goes to
and from ``torch.optim.Adam``.  The bias corrections are computed on the host in double from ``step``, as torch does with
``capturable=False``; nothing waits for the device and nothing is copied from it.

``step(visible=mask)`` (opt-in, never the default: the reference's Adam decays the moments of invisible splats too) leaves
parameter and both moments of the rows whose mask byte is 0 bit-for-bit untouched -- upstream 3DGS's sparse Adam, with the
global step count in the bias corrections.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import inspect
from typing import Optional

import torch

from . import _lib

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def _adam_defaults() -> dict:
    """torch.optim.Adam's own option names and defaults (they differ between torch versions): a state_dict of either optimizer
    then loads into the other."""
    sig = inspect.signature(torch.optim.Adam.__init__)
    return {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params") and v.default is not inspect.Parameter.empty}


class SplatAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **options):
        defaults = _adam_defaults()
        unknown = sorted(set(options) - set(defaults))
        if unknown:
            raise TypeError(f"SplatAdam: unknown option(s) {unknown}")
        defaults.update(options)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                self._check_param(p)
        except Exception:
            self.param_groups.pop()
            raise

    @staticmethod
    def _check_group(group):
        if group.get("weight_decay", 0) != 0:
            raise ValueError("SplatAdam: weight_decay is not supported (the reference's optimizer has none)")
        for name in _UNSUPPORTED:
            if group.get(name, False):
                raise ValueError(f"SplatAdam: {name} is not supported")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("SplatAdam: lr must be a number (a tensor lr belongs to capturable=True, which is not supported)")
        b1, b2 = group["betas"]
        if not 0.0 <= group["lr"] or not 0.0 <= group["eps"] or not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
            raise ValueError(f"SplatAdam: invalid lr / eps / betas: {group['lr']}, {group['eps']}, {group['betas']}")

    @staticmethod
    def _check_param(p):
        if p.dtype is not torch.float32:
            raise ValueError(f"SplatAdam: parameters must be float32, got {p.dtype}")
        if not p.is_contiguous():
            raise ValueError("SplatAdam: parameters must be contiguous")
        if not p.is_cuda:
            raise ValueError("SplatAdam has no CPU path: parameters must be on a HIP ('cuda') device")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        for st in self.state.values():        # torch's fused / capturable Adam keeps `step` on the device: here it lives on the host
            if torch.is_tensor(st.get("step")) and st["step"].device.type != "cpu":
                st["step"] = st["step"].to(device="cpu", dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None, *, visible: Optional[torch.Tensor] = None):
        """One Adam step of every parameter that has a gradient.  `visible`: [rows] bool or uint8 on the parameters' device;
        every parameter with a gradient must then have `rows` rows, and rows whose byte is 0 are left untouched."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows = 0
        if visible is not None:
            if not isinstance(visible, torch.Tensor) or visible.dtype not in (torch.bool, torch.uint8) or visible.dim() != 1:
                raise ValueError("SplatAdam: visible must be a one-dimensional bool or uint8 tensor")
            if not visible.is_cuda:
                raise ValueError("SplatAdam has no CPU path: visible must be on the parameters' HIP ('cuda') device")
            visible = visible.contiguous()
            rows = visible.shape[0]
        todo = []    # everything is checked before any state changes: a refused step leaves the optimizer as it was
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check_param(p)
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("SplatAdam does not support sparse gradients")
                if g.device != p.device:
                    raise RuntimeError("SplatAdam: a gradient must be on its parameter's device")
                if visible is not None and (visible.device != p.device or p.dim() == 0 or p.shape[0] != rows):
                    raise ValueError(f"SplatAdam: visible has {rows} rows on {visible.device}, a parameter with a gradient has shape "
                                     f"{tuple(p.shape)} on {p.device}")
                st = self.state[p]
                for name in ("exp_avg", "exp_avg_sq") if len(st) else ():
                    t = st[name]
                    if t.dtype is not torch.float32 or not t.is_contiguous() or t.device != p.device or t.numel() != p.numel():
                        raise RuntimeError(f"SplatAdam: state['{name}'] must be a contiguous float32 tensor of the parameter's size on its device")
                todo.append((group, p, g))
        jobs = {}    # device -> [(SrAdamJob fields, the gradient: kept alive until the launch is enqueued)]
        for group, p, g in todo:
            lr, eps = float(group["lr"]), float(group["eps"])
            beta1, beta2 = (float(b) for b in group["betas"])
            if g.dtype is not torch.float32 or not g.is_contiguous():
                g = g.to(torch.float32).contiguous()
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            t = float(st["step"])                       # a host scalar: no device is asked
            bias1, bias2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
            row = p.numel() // p.shape[0] if p.dim() > 0 and p.shape[0] > 0 else 1
            fields = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), row, lr / bias1,
                      bias2 ** 0.5, 1.0 - beta1, 1.0 - beta2, eps)
            jobs.setdefault(p.device, []).append((fields, g))
        if not jobs:
            return loss
        lib = _lib.load()
        for dev, items in jobs.items():
            with torch.cuda.device(dev):
                stream = _lib.stream(dev)
                mask = _lib.ptr(visible)
                for first in range(0, len(items), _lib.ADAM_MAX_TENSORS):
                    part = items[first:first + _lib.ADAM_MAX_TENSORS]
                    table = (_lib.SrAdamJob * len(part))(*[_lib.SrAdamJob(*fields) for fields, _ in part])
                    _lib.check(lib.sr_adam_step(len(part), table, mask, rows, stream))
        return loss
