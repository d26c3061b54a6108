"""build_optimizer (code/optimizer.py:29-53) for the native model, its three opt_func values, each
one HBM sweep per step over the flat parameter buffer, optionally fused with the EMA update:
  'adam'   Adam(betas=(0.9, 0.999), eps=1e-8, weight_decay=0)                    es_adam_ema_step
  'adamw'  AdamW(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)                es_adamw_ema_step
  'sgd'    SGD(momentum=0.9, nesterov=True, weight_decay=0.05)                   es_sgd_ema_step
TRAIN.WEIGHT_DECAY is ignored, as in the reference.  AdamW and SGD decay
the first param group only (the second is forced to 0, code/optimizer.py:26-27) and read each group's
own lr / weight_decay from param_groups at every step; the sweep finds an element's group in a class
map (class_map: one byte per 64 floats; 0 = frozen parameter or padding, skipped by the sweep, so
weight decay cannot move a frozen weight), rebuilt whenever the optimizer is built (the trainers
build it in get_config, after IS_FREEZE is applied).  state_dict() is torch.optim.AdamW's / SGD's
own; loading another kind's state raises a ValueError that names both.

Checkpoints use torch.optim.Adam's own state_dict format, so a native checkpoint resumes in the
reference and the other way round: the two param groups of set_weight_decay (code/optimizer.py:
13-27: trainable parameters only, in named_parameters order; 1-D tensors, `.bias` and the model's
no_weight_decay() names go to the second group), parameter indices numbered group by group, and
per-index state {'step', 'exp_avg', 'exp_avg_sq'} shaped like the parameter.  On the device the
moments stay two flat buffers in the parameter layout; frozen parameters (IS_FREEZE) get a zero
gradient and zero moments, so the fused sweep leaves them bit-for-bit unchanged.
"""
import math

import torch

from . import _lib
from ._lib import call, ptr


def _in_keywords(name, keywords):
    return any(k in name for k in keywords)


def weight_decay_groups(model):
    """(decay, no_decay) lists of parameter names, as set_weight_decay (code/optimizer.py:13-27)
    splits model.named_parameters()."""
    skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else set()
    skip_kw = model.no_weight_decay_keywords() if hasattr(model, "no_weight_decay_keywords") else set()
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if len(p.shape) == 1 or name.endswith(".bias") or name in skip or _in_keywords(name, skip_kw):
            no_decay.append(name)
        else:
            decay.append(name)
    return decay, no_decay


class NativeAdam:
    _GROUP_DEFAULTS = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                       "differentiable": False, "fused": None}

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.model = model
        self.betas, self.eps = betas, eps
        decay, no_decay = weight_decay_groups(model)
        self._group_names = [decay, no_decay]
        common = dict(lr=lr, betas=tuple(betas), eps=eps, **self._GROUP_DEFAULTS)
        self.param_groups = [dict(common, weight_decay=0), dict(common, weight_decay=0.0)]
        self.exp_avg = torch.zeros_like(model.flat)
        self.exp_avg_sq = torch.zeros_like(model.flat)
        self.step_count = 0

    def _slice(self, buf, name):
        o = self.model.offs[name]
        shape = self.model.get_parameter(name).shape
        return buf[o:o + math.prod(shape)].view(shape)

    def zero_grad(self, set_to_none=False):
        self.model.flat_grad.zero_()

    def frozen_ranges(self):
        """Flat [lo, hi) ranges of the parameters outside both groups (requires_grad False)."""
        trainable = set(self._group_names[0]) | set(self._group_names[1])
        out = []
        for name, p in self.model.named_parameters():
            if name not in trainable:
                o = self.model.offs[name]
                out.append((o, o + p.numel()))
        return out

    def step(self, ema_flat=None, ema_decay=0.999, grad_scale=1.0):
        """One Adam update from model.flat_grad (x grad_scale); fused EMA if ema_flat is given."""
        if self.exp_avg.device != self.model.flat.device:
            self.exp_avg = self.exp_avg.to(self.model.flat.device)
            self.exp_avg_sq = self.exp_avg_sq.to(self.model.flat.device)
        self.step_count += 1
        b1, b2 = self.betas
        lr = self.param_groups[0]["lr"]
        # torch.optim.Adam (single-tensor): step_size = lr / bias_correction1, computed in double
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        step_size = lr / bc1
        bc2_sqrt = math.sqrt(bc2)
        p, g = self.model.flat, self.model.flat_grad
        call("es_adam_ema_step", ptr(p), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(ema_flat), p.numel(),
             float(b1), float(b2), float(self.eps), float(-step_size), float(bc2_sqrt), float(ema_decay),
             float(1.0 - ema_decay), float(grad_scale), _lib.stream())
        self.model.mark_updated()

    # -------------------------------------------------------------- torch.optim.Adam format
    def state_dict(self):
        state, groups, idx = {}, [], 0
        for g, names in zip(self.param_groups, self._group_names):
            ids = []
            for name in names:
                if self.step_count > 0:
                    state[idx] = {"step": torch.tensor(float(self.step_count)),
                                  "exp_avg": self._slice(self.exp_avg, name).detach().cpu().clone(),
                                  "exp_avg_sq": self._slice(self.exp_avg_sq, name).detach().cpu().clone()}
                ids.append(idx)
                idx += 1
            groups.append(dict(g, params=ids))
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != len(self._group_names):
            raise ValueError(f"optimizer state has {len(groups)} param groups, the model {len(self._group_names)}")
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = set()
        for g, mine, names in zip(groups, self.param_groups, self._group_names):
            if len(g["params"]) != len(names):
                raise ValueError(f"param group sizes differ: checkpoint {len(g['params'])}, model {len(names)}")
            for idx, name in zip(g["params"], names):
                st = sd["state"].get(idx)
                if st is None:
                    continue
                self._slice(self.exp_avg, name).copy_(st["exp_avg"].reshape(self._slice(self.exp_avg, name).shape))
                self._slice(self.exp_avg_sq, name).copy_(
                    st["exp_avg_sq"].reshape(self._slice(self.exp_avg_sq, name).shape))
                steps.add(int(st["step"].item() if torch.is_tensor(st["step"]) else st["step"]))
            mine.update({k: v for k, v in g.items() if k != "params"})
        if len(steps) > 1:
            raise ValueError(f"per-parameter Adam step counts differ ({sorted(steps)}): the fused sweep keeps one")
        self.step_count = steps.pop() if steps else 0
        self.betas = tuple(self.param_groups[0]["betas"])
        self.eps = self.param_groups[0]["eps"]


GRANULE = 64  # floats per class-map byte: every native model lays its parameters at multiples of 64 floats


def class_map(model):
    """The sweeps' class map: a uint8 CPU tensor with one entry per 64 floats of model.flat -- 1 for the
    granules of a param-group-0 (decay) parameter, 2 for group 1 (no decay), 0 for frozen parameters and for
    the alignment padding behind each tensor (a parameter's last, partly filled granule carries its class:
    the padding in it has zero gradient and starts at zero, so every rule leaves it zero)."""
    assert model.numel % GRANULE == 0, f"flat buffer of {model.numel} floats is no multiple of {GRANULE}"
    cls = torch.zeros(model.numel // GRANULE, dtype=torch.uint8)
    params = dict(model.named_parameters())
    for c, names in enumerate(weight_decay_groups(model), 1):
        for name in names:
            o = model.offs[name]
            assert o % GRANULE == 0, f"{name} starts at float {o}, not a multiple of {GRANULE}"
            cls[o // GRANULE:(o + params[name].numel() + GRANULE - 1) // GRANULE] = c
    return cls


def _state_kind(sd):
    """Which torch optimizer wrote the state_dict `sd`, from its param-group keys."""
    g = sd["param_groups"][0] if sd.get("param_groups") else {}
    if "momentum" in g:
        return "SGD"
    if "betas" in g:
        return "AdamW" if g.get("decoupled_weight_decay", True) else "Adam"
    return "unknown"


class _FlatOptimizer:
    """What the class-mapped sweeps share: the two param groups with their own lr / weight_decay (read at
    every step: the LR scheduler and a loaded checkpoint write them), flat state buffers in the parameter
    layout, and torch's state_dict format sliced per parameter.  Subclasses name their torch class (KIND),
    their per-parameter state tensors (BUFFERS) and launch the sweep (_launch)."""
    KIND = None
    BUFFERS = ()

    def __init__(self, model, torch_defaults, weight_decay):
        if not hasattr(model, "flat"):
            raise NotImplementedError(f"native {self.KIND} needs a native model (flat parameter buffer)")
        self.model = model
        decay, no_decay = weight_decay_groups(model)
        self._group_names = [decay, no_decay]
        common = {k: v for k, v in torch_defaults.items() if k != "params"}
        # set_weight_decay (code/optimizer.py:26-27): the second group's weight decay is forced to 0.
        self.param_groups = [dict(common, weight_decay=weight_decay), dict(common, weight_decay=0.0)]
        self.cls = class_map(model)
        for b in self.BUFFERS:
            setattr(self, b, torch.zeros_like(model.flat))
        self.step_count = 0

    _slice = NativeAdam._slice
    zero_grad = NativeAdam.zero_grad
    frozen_ranges = NativeAdam.frozen_ranges

    def _to_device(self):
        dev = self.model.flat.device
        if self.cls.device != dev:
            self.cls = self.cls.to(dev)
        for b in self.BUFFERS:
            if getattr(self, b).device != dev:
                setattr(self, b, getattr(self, b).to(dev))

    def step(self, ema_flat=None, ema_decay=0.999, grad_scale=1.0):
        """One update from model.flat_grad (x grad_scale); fused EMA if ema_flat is given."""
        self._to_device()
        self.step_count += 1
        self._launch(ema_flat, float(ema_decay), float(grad_scale))
        self.model.mark_updated()

    def _state(self, name):
        raise NotImplementedError

    def state_dict(self):
        state, groups, idx = {}, [], 0
        for g, names in zip(self.param_groups, self._group_names):
            ids = []
            for name in names:
                if self.step_count > 0:
                    state[idx] = self._state(name)
                ids.append(idx)
                idx += 1
            groups.append(dict(g, params=ids))
        return {"state": state, "param_groups": groups}

    def _check_kind(self, sd):
        kind = _state_kind(sd)
        if kind != self.KIND:
            raise ValueError(f"optimizer state is torch.optim.{kind}'s, this optimizer is {self.KIND}: "
                             f"build the trainer with opt_func={kind!r} to resume it")

    def _load_groups(self, sd):
        """Checks the layout, zeroes the buffers, copies the group settings; yields (name, state or None)."""
        self._check_kind(sd)
        groups = sd["param_groups"]
        if len(groups) != len(self._group_names):
            raise ValueError(f"optimizer state has {len(groups)} param groups, the model {len(self._group_names)}")
        for g, names in zip(groups, self._group_names):
            if len(g["params"]) != len(names):
                raise ValueError(f"param group sizes differ: checkpoint {len(g['params'])}, model {len(names)}")
        for b in self.BUFFERS:
            getattr(self, b).zero_()
        out = []
        for g, mine, names in zip(groups, self.param_groups, self._group_names):
            out += [(name, sd["state"].get(idx)) for idx, name in zip(g["params"], names)]
            mine.update({k: v for k, v in g.items() if k != "params"})
        return out

    def _copy_in(self, buf, name, t):
        dst = self._slice(getattr(self, buf), name)
        dst.copy_(t.reshape(dst.shape))


class NativeAdamW(_FlatOptimizer):
    """torch.optim.AdamW over the flat buffer: es_adamw_ema_step, one sweep fused with the EMA."""
    KIND = "AdamW"
    BUFFERS = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05):
        ref = torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(model, ref.param_groups[0], weight_decay)

    def _launch(self, ema_flat, ema_decay, grad_scale):
        g0 = self.param_groups[0]
        (b1, b2), eps = g0["betas"], g0["eps"]
        if any(g.get("amsgrad") or g.get("maximize") for g in self.param_groups):
            raise NotImplementedError("native AdamW: amsgrad / maximize are not built")
        # torch.optim.AdamW (single-tensor): param.mul_(1 - lr * wd); step_size = lr / bias_correction1, in double
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        neg_step = [-(g["lr"] / bc1) for g in self.param_groups]
        decay_mul = [1 - g["lr"] * g["weight_decay"] for g in self.param_groups]
        p = self.model.flat
        call("es_adamw_ema_step", ptr(p), ptr(self.model.flat_grad), ptr(self.exp_avg), ptr(self.exp_avg_sq),
             ptr(ema_flat), ptr(self.cls), p.numel(), float(b1), float(b2), float(1 - b1), float(1 - b2), float(eps),
             float(math.sqrt(bc2)),
             float(neg_step[0]), float(neg_step[1]), float(decay_mul[0]), float(decay_mul[1]), ema_decay,
             float(1.0 - ema_decay), grad_scale, _lib.stream())

    def _state(self, name):
        return {"step": torch.tensor(float(self.step_count)),
                "exp_avg": self._slice(self.exp_avg, name).detach().cpu().clone(),
                "exp_avg_sq": self._slice(self.exp_avg_sq, name).detach().cpu().clone()}

    def load_state_dict(self, sd):
        steps = set()
        for name, st in self._load_groups(sd):
            if st is None:
                continue
            self._copy_in("exp_avg", name, st["exp_avg"])
            self._copy_in("exp_avg_sq", name, st["exp_avg_sq"])
            steps.add(int(st["step"].item() if torch.is_tensor(st["step"]) else st["step"]))
        if len(steps) > 1:
            raise ValueError(f"per-parameter AdamW step counts differ ({sorted(steps)}): the fused sweep keeps one")
        self.step_count = steps.pop() if steps else 0
        for g in self.param_groups:
            g["decoupled_weight_decay"] = True


class NativeSGD(_FlatOptimizer):
    """torch.optim.SGD (momentum, Nesterov, dampening 0) over the flat buffer: es_sgd_ema_step."""
    KIND = "SGD"
    BUFFERS = ("momentum_buffer",)

    def __init__(self, model, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=0.05):
        ref = torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, nesterov=nesterov,
                              weight_decay=weight_decay)
        super().__init__(model, ref.param_groups[0], weight_decay)

    def _launch(self, ema_flat, ema_decay, grad_scale):
        g0 = self.param_groups[0]
        if any(g.get("dampening") or g.get("maximize") for g in self.param_groups):
            raise NotImplementedError("native SGD: dampening / maximize are not built")
        p = self.model.flat
        call("es_sgd_ema_step", ptr(p), ptr(self.model.flat_grad), ptr(self.momentum_buffer), ptr(ema_flat),
             ptr(self.cls), p.numel(), float(g0["momentum"]), float(-self.param_groups[0]["lr"]),
             float(-self.param_groups[1]["lr"]), float(self.param_groups[0]["weight_decay"]),
             float(self.param_groups[1]["weight_decay"]), int(bool(g0["nesterov"])), ema_decay,
             float(1.0 - ema_decay), grad_scale, _lib.stream())

    def _state(self, name):
        return {"momentum_buffer": self._slice(self.momentum_buffer, name).detach().cpu().clone()}

    def load_state_dict(self, sd):
        seen = False
        for name, st in self._load_groups(sd):
            if st is None or st.get("momentum_buffer") is None:
                continue  # torch's first step clones the gradient: a zero buffer does the same
            self._copy_in("momentum_buffer", name, st["momentum_buffer"])
            seen = True
        # torch's SGD state holds no step count: 1 marks "has stepped" (buffers go into state_dict)
        self.step_count = 1 if seen else 0


def build_optimizer(model, opt_func='Adam', lr=1e-3):
    opt_lower = opt_func.lower()
    if opt_lower == 'adam':
        if not hasattr(model, "flat"):
            raise NotImplementedError("native Adam needs a native model (flat parameter buffer)")
        return NativeAdam(model, lr=lr)
    if opt_lower == 'adamw':
        return NativeAdamW(model, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    if opt_lower == 'sgd':
        return NativeSGD(model, lr=lr, momentum=0.9, nesterov=True, weight_decay=0.05)
    raise NotImplementedError(f"optimizer {opt_func!r}: Adam, AdamW and SGD are native (code/optimizer.py:43-51)")
