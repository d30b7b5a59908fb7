"""The grounding solver: what the reference's fine-grained trainer does between the loss dict and the next batch.

  make_optimizer(cfg, model)       solver/build.py:8-55   one AdamW group per trainable parameter with the reference's lr / weight-decay
                                                          rule, full-model gradient clipping around the step
  make_lr_scheduler(cfg, opt)      solver/build.py:58-119, solver/lr_scheduler.py:11-91   warm-up + multi-step / cosine, closed forms
  ModelEma(model, decay)           utils/ema.py:6-45      the averaged copy of the model the reference checkpoints and evaluates
  GroundingSolver(cfg, model)      engine/trainer.py:131-224 without AMP: sum the losses, zero a NaN total, zero_grad, backward,
                                                          optimizer step, scheduler step, weight-decay schedule, EMA update

On a HIP model the optimizer is optim.FiberTorchAdamW (csrc/solver.hip): clip_grad_norm_, AdamW over all groups and the EMA of every
updated parameter are three launches, and nothing in GroundingSolver.step() waits for the device.  On a host model everything is plain
torch (torch.optim.AdamW with the clipping wrapped around it), as optim.HFAdamW serves host tensors for the coarse-grained path.

cfg is the reference's configuration tree (attribute access); a SOLVER field that is absent takes the default of the reference's
config/defaults.py, except OPTIMIZER, which defaults to "ADAMW" (every grounding yaml sets it; SGD is not implemented)."""
import bisect
import copy
import math

import torch

from . import lib
from .optim import FiberTorchAdamW

_DEFAULTS = dict(OPTIMIZER="ADAMW", BASE_LR=0.001, LANG_LR=0.00001, BACKBONE_BODY_LR_FACTOR=1.0, BIAS_LR_FACTOR=2, WEIGHT_DECAY=0.0005,
                 WEIGHT_DECAY_BIAS=0.0, WEIGHT_DECAY_NORM_FACTOR=1.0, MODEL_EMA=0.0, MAX_ITER=40000, MULTI_MAX_EPOCH=(), USE_COSINE=False,
                 MIN_LR=0.000001, GAMMA=0.1, STEPS=(30000,), USE_AUTOSTEP=False, WARMUP_FACTOR=1.0 / 3, WARMUP_ITERS=500,
                 WARMUP_METHOD="linear", WEIGHT_DECAY_SCHEDULE=False, WEIGHT_DECAY_SCHEDULE_RATIO=0.667)
_CLIP_DEFAULTS = dict(ENABLED=False, CLIP_VALUE=0.0, CLIP_TYPE="full_model", NORM_TYPE=2.0)


def _solver(cfg, name):
    return getattr(cfg.SOLVER, name, _DEFAULTS[name])


def _clip(cfg, name):
    return getattr(getattr(cfg.SOLVER, "CLIP_GRADIENTS", None), name, _CLIP_DEFAULTS[name])


# ---- optimizer -------------------------------------------------------------------------------------------------------------------------
def group_hyper(cfg, key):
    """(lr, weight_decay) of the parameter named `key`: the reference's rule with its substring tests as they are -- "bias" also matches
    `relative_position_bias_table`, "norm" / "Norm" match any module so named."""
    lr, wd = _solver(cfg, "BASE_LR"), _solver(cfg, "WEIGHT_DECAY")
    if "language_backbone" in key:
        lr = _solver(cfg, "LANG_LR")
    if "backbone.body" in key and "language_backbone.body" not in key:
        lr = _solver(cfg, "BASE_LR") * _solver(cfg, "BACKBONE_BODY_LR_FACTOR")
    if "bias" in key:
        lr = lr * _solver(cfg, "BIAS_LR_FACTOR")
        wd = _solver(cfg, "WEIGHT_DECAY_BIAS")
    if "norm" in key or "Norm" in key:
        wd = wd * _solver(cfg, "WEIGHT_DECAY_NORM_FACTOR")
    return lr, wd


def clip_value(cfg):
    """max_norm of the full-model clipping, or None when the configuration switches it off"""
    if _clip(cfg, "ENABLED") and _clip(cfg, "CLIP_TYPE") != "full_model":
        raise NotImplementedError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE = {_clip(cfg, 'CLIP_TYPE')!r}: only \"full_model\" clipping (one norm over "
                                  "every parameter) is implemented")
    if _clip(cfg, "ENABLED") and float(_clip(cfg, "NORM_TYPE")) != 2.0:
        raise NotImplementedError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE = {_clip(cfg, 'NORM_TYPE')}: the norm kernel computes the 2-norm only")
    on = _clip(cfg, "ENABLED") and _clip(cfg, "CLIP_VALUE") > 0.0
    return float(_clip(cfg, "CLIP_VALUE")) if on else None


class ClippedAdamW(torch.optim.AdamW):
    """torch.optim.AdamW with clip_grad_norm_ over all its parameters in front of every step: the host form of FiberTorchAdamW"""

    def __init__(self, params, lr, max_grad_norm=None):
        super().__init__(params, lr)
        self.max_grad_norm = max_grad_norm

    def step(self, closure=None):
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"]], self.max_grad_norm)
        return super().step(closure)


def make_optimizer(cfg, model):
    if _solver(cfg, "OPTIMIZER") != "ADAMW":
        raise NotImplementedError(f"SOLVER.OPTIMIZER = {_solver(cfg, 'OPTIMIZER')!r}: only \"ADAMW\" is implemented (the grounding configurations "
                                  "use nothing else)")
    max_norm = clip_value(cfg)
    groups = []
    for key, p in model.named_parameters():
        if p.requires_grad:
            lr, wd = group_hyper(cfg, key)
            groups.append({"params": [p], "lr": lr, "weight_decay": wd})
    if not groups:
        raise ValueError("make_optimizer: the model has no trainable parameter")
    if groups[0]["params"][0].is_cuda:
        return FiberTorchAdamW(groups, lr=_solver(cfg, "BASE_LR"), max_grad_norm=max_norm)
    return ClippedAdamW(groups, _solver(cfg, "BASE_LR"), max_grad_norm=max_norm)


# ---- learning-rate schedules --------------------------------------------------------------------------------------------------------------
def _warmup(it, iters, factor, method):
    """the factor on the base lr at iteration `it` of a warm-up of `iters` iterations: `factor` throughout ("constant") or the line from
    `factor` at 0 to 1 at `iters` ("linear"); 1 afterwards"""
    if it >= iters:
        return 1.0
    if method == "constant":
        return factor
    a = it / iters
    return factor * (1.0 - a) + a


class _Warmup(torch.optim.lr_scheduler.LRScheduler):
    def __init__(self, optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch):
        if warmup_method not in ("constant", "linear"):
            raise ValueError(f"warmup_method must be 'constant' or 'linear', got {warmup_method!r}")
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        super().__init__(optimizer, last_epoch)


class WarmupMultiStepLR(_Warmup):
    """lr_i(it) = base_i warmup(it) gamma^(number of milestones <= it)"""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method="linear", last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError(f"milestones must be increasing, got {milestones}")
        self.milestones, self.gamma = list(milestones), gamma
        super().__init__(optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch)

    def get_lr(self):
        it = self.last_epoch
        f = _warmup(it, self.warmup_iters, self.warmup_factor, self.warmup_method) * self.gamma ** bisect.bisect_right(self.milestones, it)
        return [b * f for b in self.base_lrs]


class WarmupCosineAnnealingLR(_Warmup):
    """lr_i(it) = base_i warmup(it) during the warm-up, then eta_min + (base_i - eta_min) (1 + cos(pi (it - warmup_iters) / max_iters)) / 2"""

    def __init__(self, optimizer, max_iters, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method="linear", eta_min=0, last_epoch=-1):
        self.max_iters, self.gamma, self.eta_min = max_iters, gamma, eta_min
        super().__init__(optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch)

    def get_lr(self):
        it = self.last_epoch
        if it < self.warmup_iters:
            f = _warmup(it, self.warmup_iters, self.warmup_factor, self.warmup_method)
            return [b * f for b in self.base_lrs]
        c = (1.0 + math.cos(math.pi * (it - self.warmup_iters) / self.max_iters)) / 2.0
        return [self.eta_min + (b - self.eta_min) * c for b in self.base_lrs]


def make_lr_scheduler(cfg, optimizer):
    if _solver(cfg, "MULTI_MAX_EPOCH"):
        raise NotImplementedError("SOLVER.MULTI_MAX_EPOCH: the multi-stage schedule (a list of schedulers) is not implemented")
    warm = dict(warmup_factor=_solver(cfg, "WARMUP_FACTOR"), warmup_iters=_solver(cfg, "WARMUP_ITERS"), warmup_method=_solver(cfg, "WARMUP_METHOD"))
    if _solver(cfg, "USE_COSINE"):
        return WarmupCosineAnnealingLR(optimizer, _solver(cfg, "MAX_ITER"), _solver(cfg, "GAMMA"), eta_min=_solver(cfg, "MIN_LR"), **warm)
    if _solver(cfg, "USE_AUTOSTEP"):
        raise NotImplementedError("SOLVER.USE_AUTOSTEP: the reduce-on-plateau schedule needs evaluation during training, which is not implemented")
    milestones = [round(s * _solver(cfg, "MAX_ITER")) if s < 1 else s for s in _solver(cfg, "STEPS")]
    return WarmupMultiStepLR(optimizer, milestones, _solver(cfg, "GAMMA"), **warm)


# ---- model EMA ----------------------------------------------------------------------------------------------------------------------------
def _unwrap(model):
    return model.module if hasattr(model, "module") else model


class ModelEma:
    """Exponential moving average of a model's state dict, ema = decay ema + (1 - decay) value after every step: `.ema` is a deep copy of
    the (unwrapped) model in eval mode with nothing trainable, the weights the reference checkpoints and evaluates.

    Entries that are not floating point (`relative_position_index`, `position_ids`) are COPIED, not averaged: the reference averages
    them in fp32 and truncates back to integers, which can move an index down by one.

    On a HIP model the average is taken by csrc/solver.hip.  Attached to a FiberTorchAdamW (`optimizer.attach_ema(self)`), the
    optimizer's own launch writes the EMA of every parameter it updates and `update()` handles only what is left -- trainable
    parameters without a gradient, frozen parameters, buffers -- in one fiber_ema_multi_f32 launch; unattached, that launch covers
    every floating entry.  On the host it is plain torch."""

    def __init__(self, model, decay=0.9999, device=""):
        src = _unwrap(model)
        self.ema = copy.deepcopy(src)
        self.ema.eval()
        self.decay = decay
        self.device = device
        if device:
            self.ema.to(device=device)
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._by_id = {id(p): e for (_, p), (_, e) in zip(src.named_parameters(), self.ema.named_parameters())}
        self._attached = None                    # the FiberTorchAdamW that writes the EMA of the parameters it steps
        self._tab = None
        self._chunk = None

    def ema_of(self, p):
        """the EMA copy of the model's parameter `p` (None: not a parameter of the model this was built from)"""
        return self._by_id.get(id(p))

    def state_dict(self):
        return self.ema.state_dict()

    def load_checkpoint(self, checkpoint):
        """checkpoint: a path or a dict; its "model_ema" entry (keys with or without a "module." prefix) is loaded into `.ema`"""
        if isinstance(checkpoint, str):
            checkpoint = torch.load(checkpoint, map_location="cpu")
        if not isinstance(checkpoint, dict):
            raise TypeError("ModelEma.load_checkpoint: a path or a dict is expected")
        if "model_ema" in checkpoint:
            self.ema.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in checkpoint["model_ema"].items()})

    @torch.no_grad()
    def update(self, model):
        src = _unwrap(model)
        msd, esd = src.state_dict(), self.ema.state_dict()
        done = self._attached.take_ema_done() if self._attached is not None else frozenset()
        skip = {k for k, p in src.named_parameters() if id(p) in done} if done else ()
        d = float(self.decay)
        rest, ints = [], []
        for k, e in esd.items():
            v = msd[k]
            if not e.is_floating_point():
                ints.append((e, v))
            elif k not in skip:
                rest.append((e, v))
        if ints:
            torch._foreach_copy_([e for e, _ in ints], [v.to(e.device) for e, v in ints])
        if not rest:
            return
        if not rest[0][0].is_cuda:
            for e, v in rest:
                e.mul_(d).add_(v.to(e.device), alpha=1.0 - d)
            return
        for e, v in rest:
            if e.dtype != torch.float32 or v.dtype != torch.float32 or not e.is_contiguous() or not v.is_contiguous() or v.device != e.device:
                raise lib.FiberHipError("ModelEma.update: floating entries must be contiguous fp32 tensors on the EMA's device")
        key = tuple((v.data_ptr(), e.data_ptr()) for e, v in rest)
        tab = self._tab
        if tab is None or tab["key"] != key:
            if self._chunk is None:
                self._chunk = lib.plain("fiber_adamw_chunk")
            dev = rest[0][0].device
            sizes = [e.numel() for e, _ in rest]
            chunks = [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // self._chunk))]
            up = lambda host: torch.empty(tuple(host.shape), dtype=host.dtype, device=dev).copy_(host, non_blocking=True)   # noqa: E731
            tab = self._tab = {"key": key, "n": len(chunks), "table": up(torch.tensor(key, dtype=torch.int64)),
                               "numel": up(torch.tensor(sizes, dtype=torch.int64)), "chunks": up(torch.tensor(chunks, dtype=torch.int32))}
        with torch.cuda.device(rest[0][0].device):
            lib.call("fiber_ema_multi_f32", lib.ptr(tab["table"]), lib.ptr(tab["numel"]), lib.ptr(tab["chunks"]), tab["n"], d)
        # the kernel wrote these tensors behind autograd's back: bump their version counters, so that cached bf16 working copies of the
        # EMA model's weights (ops.bf16_weight) are seen to be stale
        torch.autograd.graph.increment_version([e for e, _ in rest])


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
class GroundingSolver:
    """Optimizer, schedule and EMA of the grounding model, and the body of the reference's training iteration after the forward pass.
    No GradScaler: the HIP path computes in bf16, whose range is fp32's."""

    def __init__(self, cfg, model):
        self.cfg, self.model = cfg, model
        self.optimizer = make_optimizer(cfg, model)
        self.scheduler = make_lr_scheduler(cfg, self.optimizer)
        decay = _solver(cfg, "MODEL_EMA")
        self.model_ema = ModelEma(model, decay) if decay > 0 else None
        if self.model_ema is not None and isinstance(self.optimizer, FiberTorchAdamW):
            self.optimizer.attach_ema(self.model_ema)
        self.milestone_target = 0                # the next milestone the weight-decay schedule waits for

    def step(self, loss_dict):
        """One iteration from the loss dict the model returned.  -> the loss dict, detached.  Nothing here reads from the device."""
        total = sum(loss_dict.values())
        total = torch.where(torch.isnan(total), torch.zeros_like(total), total)      # a NaN total contributes no gradient
        self.optimizer.zero_grad()
        total.backward()
        self.optimizer.step()
        self.scheduler.step()
        if _solver(self.cfg, "WEIGHT_DECAY_SCHEDULE") and hasattr(self.scheduler, "milestones"):
            ms = self.scheduler.milestones
            nxt = ms[self.milestone_target] if self.milestone_target < len(ms) else math.inf
            if self.scheduler.last_epoch >= nxt * _solver(self.cfg, "WEIGHT_DECAY_SCHEDULE_RATIO"):
                for group in self.optimizer.param_groups:
                    if "weight_decay" in group:
                        group["weight_decay"] *= self.scheduler.gamma
                self.milestone_target += 1
        if self.model_ema is not None:
            self.model_ema.update(self.model)
        return {k: v.detach() for k, v in loss_dict.items()}

    def state_dict(self):
        sd = {"optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(), "milestone_target": self.milestone_target}
        if self.model_ema is not None:
            sd["model_ema"] = self.model_ema.state_dict()
        return sd

    def load_state_dict(self, sd):
        self.optimizer.load_state_dict(sd["optimizer"])
        self.scheduler.load_state_dict(sd["scheduler"])
        self.milestone_target = sd.get("milestone_target", 0)
        if self.model_ema is not None:
            self.model_ema.load_checkpoint(sd)
