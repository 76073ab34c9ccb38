"""The parameter update of the deform network on the device: ``NetworkAdam`` is ``torch.optim.Adam`` (reference
scene/deform_model.py:23-34 builds ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` over every parameter of the network, train.py:318
steps it) with the step as ONE kernel launch per ``SR_NET_ADAM_MAX_GRADS`` tensors (``sr_net_adam_step``, csrc/network_adam.hip):
one launch for the 71 and 137 tensors of the static and the 4-D network, two for the 502 of the network with the plane generator.

``SplatAdam`` (optim.py) builds its job table per step and passes it as the kernel argument, 32 jobs at a time: right for six
large tensors, wrong for five hundred small ones.  Here the table is a PLAN: the addresses of a network's parameters and moments
do not change from step to step, so the table is written once, lives on the device, and a step passes only the gradient
pointers and one set of scalars.  The plan is rebuilt when a parameter's or a moment's address, an element count or the list of
parameters changes (``p.data = ...``, ``module.to(...)``, ``add_param_group``, ``load_state_dict``, a first gradient);
``plans_built`` counts the builds.  Writing ``group["lr"]`` needs no new plan.

``param_groups`` and ``state`` have exactly torch.optim.Adam's layout -- per parameter ``step`` (a float32 scalar on the host),
``exp_avg`` and ``exp_avg_sq``, created on the first step in which the parameter has a gradient -- so ``state_dict()`` goes to and
from ``torch.optim.Adam`` and ``SplatAdam``.  The moments this optimizer creates are views into two flat buffers (two fills instead
of two per tensor), each at its parameter's offset modulo 16 bytes, which is what the kernel's 16-byte path needs.  The arithmetic
is ``SplatAdam``'s, bit for bit; the bias corrections are computed on the host in double from the step count.  Nothing waits for
the device and nothing is copied from it.  There is no CPU path and no row mask."""
from __future__ import annotations

import ctypes as C
import os
from itertools import repeat
from operator import attrgetter, is_
from typing import Optional

import torch

from . import _lib
from .optim import SplatAdam, _adam_defaults

_check_group, _check_param = SplatAdam._check_group, SplatAdam._check_param

NETWORK_OPTIMIZERS = ("torch", "fused")


def checked_network_optimizer(name) -> str:
    if name not in NETWORK_OPTIMIZERS:
        raise ValueError(f"unknown network optimizer {name!r}: expected one of {NETWORK_OPTIMIZERS}")
    return name


# process default of the deform network's optimizer, read once: SPLATFIELDS_NETWORK_OPTIMIZER=fused gives every
# SplatFieldsModel.train_setting that does not name one itself a NetworkAdam
_NETWORK_OPTIMIZER = checked_network_optimizer(os.environ.get("SPLATFIELDS_NETWORK_OPTIMIZER") or "torch")


def set_network_optimizer(name: str) -> str:
    """Process default of the deform network's optimizer: "torch" (torch.optim.Adam) or "fused" (NetworkAdam).  Returns the
    previous setting."""
    global _NETWORK_OPTIMIZER
    prev, _NETWORK_OPTIMIZER = _NETWORK_OPTIMIZER, checked_network_optimizer(name)
    return prev


def network_optimizer() -> str:
    return _NETWORK_OPTIMIZER


def resolve_network_optimizer(name: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _NETWORK_OPTIMIZER if name is None else checked_network_optimizer(name)


_data_ptr, _numel, _is_contiguous, _get_device = torch.Tensor.data_ptr, torch.Tensor.numel, torch.Tensor.is_contiguous, torch.Tensor.get_device
_grad_of, _dtype_of = attrgetter("grad"), attrgetter("dtype")
_FLOAT32 = {torch.float32}


def _hyper(group):
    """what one launch's scalars are made of, besides the step count"""
    return float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])


class _Plan:
    """The table of one list of parameters (host and device copy), what it was built from -- the addresses and counts a step
    compares against --, and what a step fills: the gradient pointers."""

    def __init__(self, groups, state):
        self.params = [p for group in groups for p in group["params"]]
        self.group_sizes = [len(group["params"]) for group in groups]
        self.group_of = [gi for gi, group in enumerate(groups) for _ in group["params"]]
        n = self.length = len(self.params)
        self.all = list(range(n))
        self.device = self.params[0].device if n else None
        self.device_index = {self.device.index} if n else None
        self.table = (_lib.SrNetAdamSlot * max(n, 1))()
        self.param_ptrs, self.numels, self.m_ptrs, self.v_ptrs, self.steps, self.counts = [], [], [], [], [], []
        for i, p in enumerate(self.params):
            st = state.get(p)
            m, v = (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) if st else (0, 0)
            slot = self.table[i]
            slot.param, slot.exp_avg, slot.exp_avg_sq, slot.count = p.data_ptr(), m, v, p.numel()
            self.param_ptrs.append(p.data_ptr()); self.numels.append(p.numel()); self.m_ptrs.append(m); self.v_ptrs.append(v)
            self.counts.append(int(st["step"]) if st else 0)           # a host scalar, read once per plan
        # the step counts of the plan's tensors become views into ONE host buffer: a step in which all of them have a gradient
        # increments them with one add (a foreach add over 500 host scalars costs more than the launch)
        self.flat_steps = torch.tensor([float(c) for c in self.counts], dtype=torch.float32)
        self.with_state = 0
        for i, p in enumerate(self.params):
            st = state.get(p)
            if st:
                st["step"] = self.flat_steps[i]
                self.with_state += 1
            self.steps.append(st["step"] if st else None)
        lib = _lib.load()
        _lib.check(lib.sr_net_adam_plan(self.table, n))                # fills chunk_end: one owner of the chunking
        if n:
            self.table_dev = torch.frombuffer(self.table, dtype=torch.uint8).to(self.device)      # uploaded once
            self.table_dev_ptr = C.cast(C.c_void_p(self.table_dev.data_ptr()), C.POINTER(_lib.SrNetAdamSlot))
        self.grads = (C.c_void_p * max(n, 1))()                       # what a step fills
        width = C.sizeof(C.c_void_p)
        self.ranges = [(first, min(_lib.NET_ADAM_MAX_GRADS, n - first),
                        (C.c_void_p * min(_lib.NET_ADAM_MAX_GRADS, n - first)).from_buffer(self.grads, first * width))
                       for first in range(0, n, _lib.NET_ADAM_MAX_GRADS)]

    @staticmethod
    def check(groups, state):
        """what a plan cannot be built from: parameters on several devices, state that is not what this optimizer creates"""
        device = None
        for group in groups:
            for p in group["params"]:
                device = p.device if device is None else device
                if p.device != device:
                    raise ValueError(f"NetworkAdam: all parameters must be on one device, got {device} and {p.device}")
                st = state.get(p)
                if not st:
                    continue
                for name in ("exp_avg", "exp_avg_sq"):
                    t = st[name]
                    if t.dtype is not torch.float32 or not t.is_contiguous() or t.device != p.device or t.numel() != p.numel():
                        raise RuntimeError(f"NetworkAdam: state['{name}'] must be a contiguous float32 tensor of the parameter's size on its device")
                if not torch.is_tensor(st.get("step")) or st["step"].device.type != "cpu":
                    raise RuntimeError("NetworkAdam: state['step'] must be a tensor on the host")

    def describes(self, groups, state, stepped):
        """the plan was built from these groups, and from the addresses, counts and state tensors that the parameters (and, of
        the tensors `stepped`, the state) have now"""
        if [len(group["params"]) for group in groups] != self.group_sizes:
            return False
        k = 0
        for group in groups:
            size = len(group["params"])
            if not all(map(is_, group["params"], self.params[k:k + size])):
                return False
            k += size
        if list(map(_data_ptr, self.params)) != self.param_ptrs or list(map(_numel, self.params)) != self.numels:
            return False
        whole = len(stepped) == self.length
        try:
            states = [state.get(self.params[i]) for i in stepped] if not whole else list(map(state.get, self.params))
            return ([st["exp_avg"].data_ptr() for st in states] == (self.m_ptrs if whole else [self.m_ptrs[i] for i in stepped])
                    and [st["exp_avg_sq"].data_ptr() for st in states] == (self.v_ptrs if whole else [self.v_ptrs[i] for i in stepped])
                    and all(map(is_, [st["step"] for st in states], self.steps if whole else [self.steps[i] for i in stepped])))
        except (KeyError, TypeError):                                  # a tensor with a first gradient has no state yet
            return False


class NetworkAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **options):
        defaults = _adam_defaults()
        unknown = sorted(set(options) - set(defaults))
        if unknown:
            raise TypeError(f"NetworkAdam: unknown option(s) {unknown}")
        defaults.update(options)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self._plan, self.plans_built = None, 0
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_group(group)
            for p in group["params"]:
                _check_param(p)
        except Exception:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plan, self.plans_built = None, 0                         # a plan holds addresses: it never travels

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None                                              # the loaded moments are other tensors
        for group in self.param_groups:
            _check_group(group)
        for st in self.state.values():        # torch's fused / capturable Adam keeps `step` on the device: here it lives on the host
            if torch.is_tensor(st.get("step")) and st["step"].device.type != "cpu":
                st["step"] = st["step"].to(device="cpu", dtype=torch.float32)

    def _create_state(self, fresh):
        """`step`, `exp_avg`, `exp_avg_sq` of parameters that have their first gradient: the moments are views into two flat
        buffers, each at its parameter's offset modulo 16 bytes."""
        offsets, total = [], 0
        for p in fresh:
            total = (total + 3) // 4 * 4 + ((p.data_ptr() >> 2) & 3)
            offsets.append(total)
            total += p.numel()
        flat_m, flat_v = (torch.zeros(total + 4, dtype=torch.float32, device=fresh[0].device) for _ in range(2))
        for p, off in zip(fresh, offsets):
            st = self.state[p]
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = flat_m.narrow(0, off, p.numel()).view(p.shape)
            st["exp_avg_sq"] = flat_v.narrow(0, off, p.numel()).view(p.shape)

    def _gather(self):
        """-> (the gradient of every parameter of the plan, or None; converted gradients to keep alive until the launch).  The
        steady state: every gradient is dense float32, contiguous and on the device, and the plan still describes the tensors --
        a handful of passes over the lists, no per-tensor Python.  Anything else goes through `_gather_checked`."""
        plan = self._plan
        if plan is None:
            return self._gather_checked()
        grads = list(map(_grad_of, plan.params))
        missing = sum(map(is_, grads, repeat(None)))
        stepped = plan.all if not missing else [i for i, g in enumerate(grads) if g is not None]
        have = grads if not missing else [grads[i] for i in stepped]
        try:
            pointers = list(map(_data_ptr, have))
            plain = (not have or (set(map(_dtype_of, have)) == _FLOAT32 and all(map(_is_contiguous, have))
                                  and set(map(_get_device, have)) == plan.device_index))
        except RuntimeError:                                           # a sparse gradient has no data pointer
            plain = False
        if not plain or not plan.describes(self.param_groups, self.state, stepped):
            return self._gather_checked()
        for group in self.param_groups:
            _check_group(group)
        if missing:
            full = [0] * plan.length
            for i, pointer in zip(stepped, pointers):
                full[i] = pointer
            pointers = full
        plan.grads[:plan.length] = pointers
        return stepped, {}

    def _gather_checked(self):
        """The same with every check spelled out: everything is checked before any state changes, so a refused step leaves the
        optimizer as it was; gradients of another dtype or layout are converted; parameters with a first gradient get their
        state; the plan is built again when it does not describe the tensors."""
        converted, fresh, grads = {}, [], []
        for group in self.param_groups:
            _check_group(group)
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    _check_param(p)
                    if g.is_sparse:
                        raise RuntimeError("NetworkAdam does not support sparse gradients")
                    if g.device != p.device:
                        raise RuntimeError("NetworkAdam: a gradient must be on its parameter's device")
                    if g.dtype is not torch.float32 or not g.is_contiguous():
                        g = converted[p] = g.to(torch.float32).contiguous()
                    if not self.state.get(p):
                        fresh.append(p)
                grads.append(g)
        stepped = [i for i, g in enumerate(grads) if g is not None]
        plan = self._plan
        if fresh or plan is None or not plan.describes(self.param_groups, self.state, stepped):
            _Plan.check(self.param_groups, self.state)                 # the last check: from here on the state changes
            if fresh:
                self._create_state(fresh)
            plan = self._plan = _Plan(self.param_groups, self.state)
            self.plans_built += 1
        plan.grads[:plan.length] = [0 if g is None else g.data_ptr() for g in grads]
        return stepped, converted

    @torch.no_grad()
    def step(self, closure=None):
        """One Adam step of every parameter that has a gradient."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        stepped, keep = self._gather()
        if not stepped:
            return loss
        plan = self._plan
        counts, group_of = plan.counts, plan.group_of
        for i in stepped:
            counts[i] += 1
        if len(stepped) == plan.with_state:                            # the tensors that have a state are the ones with a gradient
            plan.flat_steps.add_(1)
        else:
            torch._foreach_add_([plan.steps[i] for i in stepped], 1)
        hypers = {}        # (lr, beta1, beta2, eps) -> its index: groups that share all four share a launch
        of_group = [hypers.setdefault(_hyper(group), len(hypers)) for group in self.param_groups]
        hypers = list(hypers)
        if len(stepped) == plan.length:
            active = [of_group[gi] for gi in group_of]
        else:
            active = [-1] * plan.length
            for i in stepped:
                active[i] = of_group[group_of[i]]
        lib = _lib.load()
        with torch.cuda.device(plan.device):
            stream = _lib.stream(plan.device)
            for first, n, pointers in plan.ranges:
                # one launch carries one set of scalars: the tensors of the range that share lr, betas, eps and step count
                shares = sorted(s for s in set(zip(active[first:first + n], counts[first:first + n])) if s[0] >= 0)
                for hi, t in shares:
                    lr, beta1, beta2, eps = hypers[hi]
                    bias1, bias2 = 1.0 - beta1 ** float(t), 1.0 - beta2 ** float(t)
                    scalars = _lib.SrNetAdamScalars(lr / bias1, bias2 ** 0.5, 1.0 - beta1, 1.0 - beta2, eps)
                    if len(shares) > 1:    # the other tensors of the range are skipped in this launch: their pointers are null
                        mine = (C.c_void_p * n)()
                        for j in range(n):
                            if active[first + j] == hi and counts[first + j] == t:
                                mine[j] = pointers[j]
                    else:
                        mine = pointers
                    _lib.check(lib.sr_net_adam_step(plan.table, plan.table_dev_ptr, plan.length, first, n, mine, C.byref(scalars), stream))
        del keep
        return loss
