"""AdamW for the fused path on the HIP kernel of csrc/optim.hip: one launch per parameter group (one per distinct step count in
a group whose members' counts differ: the rule counts steps per parameter, the kernel takes one count per launch), bf16 working
copies of the weights refreshed in the same pass.  The update rule is transformers 4.6.0 `AdamW(correct_bias=True)` (reference
fiber_utils.py:248-252) in ITS form -- eps added to the un-corrected sqrt(v), weight decay applied after the Adam update --
which differs from torch.optim.AdamW for small gradients / early steps.  `HFAdamW` is the same rule in plain torch for host
tensors (CPU wiring tests).  Parameter groups, `lr` scheduling through LambdaLR, state_dict / load_state_dict work as for
any torch optimizer.

Host side: the pointer / size / chunk tables of a group live on the device and are rebuilt only when something moved (a
gradient was re-allocated, a bf16 copy appeared); the per-step work is one pass over the parameters comparing addresses.

`FiberTorchAdamW` is torch.optim.AdamW's form of the rule (decay first, eps added to the bias-corrected sqrt(v)) for the grounding
model, on the kernels of csrc/solver.hip: full-model gradient clipping, the update of every parameter of every group and the model
EMA in three launches, the step counts and bias corrections kept on the device."""
import torch

from . import lib, ops


class HFAdamW(torch.optim.Optimizer):
    """transformers 4.6.0 AdamW(correct_bias=True), restated (optimization.py of that release): used where the HIP kernel
    cannot run (host tensors)."""

    def __init__(self, params, lr=1e-5, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                g = p.grad
                st["exp_avg"].mul_(b1).add_(g, alpha=1.0 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                step_size = group["lr"] * (1.0 - b2 ** st["step"]) ** 0.5 / (1.0 - b1 ** st["step"])
                p.addcdiv_(st["exp_avg"], st["exp_avg_sq"].sqrt().add_(group["eps"]), value=-step_size)
                if group["weight_decay"] > 0.0:
                    p.add_(p, alpha=-group["lr"] * group["weight_decay"])
        return loss


class FiberAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-5, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._chunk = None
        self._tables = {}                       # group index -> cached device tables
        self.rebuilds = 0                       # how often a table had to be rebuilt (diagnostics)
        self._hyper = None                      # graph mode: device float [groups, 2] = {lr, bias-corrected step size}

    # ---- hipGraph support ---------------------------------------------------------------------------------------------
    # A captured step bakes every by-value kernel argument.  In graph mode the two arguments that change per step -- the
    # group's learning rate and its bias-corrected step size -- live in device memory; `prepare_replay()` advances the step
    # counters on the host, recomputes them from the (scheduler-updated) param_groups and uploads them ahead of the replay.
    def enable_graph_mode(self):
        if not self._tables:
            raise lib.FiberHipError("FiberAdamW.enable_graph_mode: take one eager step first (device tables not built yet)")
        self._check_uniform_steps("enable_graph_mode")
        dev = next(p for g in self.param_groups for p in g["params"]).device
        n = len(self.param_groups)
        self._hyper = torch.zeros((n, 2), dtype=torch.float32, device=dev)

    def disable_graph_mode(self):
        self._hyper = None

    def _check_uniform_steps(self, who):
        """The device `hyper` row holds ONE bias-corrected step size per group: a group whose members have taken different numbers
        of steps (a parameter that got its first gradient later, a loaded state dict) cannot be replayed from it."""
        for gi, tab in self._tables.items():
            steps = {st["step"] for st in tab["states"]}
            if len(steps) > 1:
                raise lib.FiberHipError(f"FiberAdamW.{who}: the parameters of group {gi} have taken different numbers of steps "
                                        f"({sorted(steps)}); graph mode keeps one step count per group")

    def prepare_replay(self):
        # The host runs ahead of the GPU (replays are asynchronous), so the upload must not read host memory that a LATER
        # prepare_replay() may already have overwritten: a FRESH pageable host tensor per call -- the runtime stages a pageable
        # source before copy_() returns (as for the pointer tables in step()), so step k's graph always sees step k's values.
        self._check_uniform_steps("prepare_replay")
        dev_t = self._hyper
        host_t = torch.zeros(tuple(dev_t.shape), dtype=torch.float32)
        for gi, group in enumerate(self.param_groups):
            tab = self._tables.get(gi)
            if tab is None:
                continue
            step = tab["states"][0]["step"] + 1
            for st in tab["states"]:
                st["step"] = step
            b1, b2 = group["betas"]
            lr = float(group["lr"])
            host_t[gi, 0] = lr
            host_t[gi, 1] = lr * (1.0 - b2 ** step) ** 0.5 / (1.0 - b1 ** step)
        dev_t.copy_(host_t, non_blocking=True)

    def load_state_dict(self, state_dict):
        """Loaded moments and step counters live in NEW tensors / dicts: drop every cached device table."""
        super().load_state_dict(state_dict)
        self._tables = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}
        self.__dict__.setdefault("_chunk", None)
        self.__dict__.setdefault("rebuilds", 0)
        self.__dict__.setdefault("_hyper", None)

    def _state_of(self, p):
        st = self.state[p]
        if st and isinstance(st.get("step"), torch.Tensor):     # a state dict saved by torch.optim.AdamW keeps tensor steps
            st["step"] = int(st["step"].item())
        if not st:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise lib.FiberHipError("FiberAdamW needs contiguous fp32 parameters on a HIP device")
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _split_by_step(self, tab):
        """Members of one table whose step counts differ: one launch per distinct count, each over that count's chunks of the SAME
        pointer table.  Which members go together does not change while they step together, so the chunk lists are kept."""
        steps = [st["step"] for st in tab["states"]]
        sig = tuple(s - steps[0] for s in steps)
        if tab.get("split_sig") != sig:
            host = tab["chunks"].cpu()
            tab["split"] = []
            for d in sorted(set(sig)):
                rows = host[torch.tensor([sig[i] == d for i in host[:, 0].tolist()])]
                tab["split"].append((d, rows.contiguous().to(tab["chunks"].device), rows.shape[0]))
            tab["split_sig"] = sig
        return [(steps[0] + d, chunks, n) for d, chunks, n in tab["split"]]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._chunk is None:
            self._chunk = lib.plain("fiber_adamw_chunk")
        cached = ops.bf16_copy_if_cached
        bumped = False
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group["params"] if p.grad is not None]
            if not plist:
                continue
            grads = []
            for p in plist:
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise lib.FiberHipError("FiberAdamW needs contiguous fp32 gradients")
                grads.append(g.data_ptr())
            copies = [cached(p) for p in plist]
            # what the cached device table was built from: the parameters AND their storage AND the state dicts (a
            # load_state_dict() swaps self.state's dicts and tensors, model.to() moves storage under an unchanged id)
            members = (tuple(map(id, plist)), tuple(p.data_ptr() for p in plist), tuple(id(self.state[p]) for p in plist))
            key = (members, tuple(grads), tuple(0 if c is None else c.data_ptr() for c in copies))
            tab = self._tables.get(gi)
            if tab is None or tab["key"] is None or tab["key"][0] != key[0]:   # membership / storage / state changed: rebuild
                self.rebuilds += 1
                states = [self._state_of(p) for p in plist]
                sizes = [p.numel() for p in plist]
                chunks = [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // self._chunk))]
                dev = plist[0].device
                fixed = torch.tensor([(p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), 0)
                                      for p, st in zip(plist, states)], dtype=torch.int64)
                tab = {"key": None, "n": len(chunks), "states": states, "fixed": fixed,
                       "table": torch.empty_like(fixed, device=dev),
                       "numel": torch.tensor(sizes, dtype=torch.int64).to(dev),
                       "chunks": torch.tensor(chunks, dtype=torch.int32).to(dev)}
                self._tables[gi] = tab
            if tab["key"] != key:
                # gradients are re-allocated every step under zero_grad(set_to_none=True): re-send the (27 KB) pointer table.
                # A fresh pageable host tensor per upload: the runtime stages it before returning, so nothing the CPU does
                # later (it runs up to a step ahead of the GPU) can touch the bytes in flight.
                host = tab["fixed"].clone()
                host[:, 1] = torch.tensor(key[1], dtype=torch.int64)
                host[:, 4] = torch.tensor(key[2], dtype=torch.int64)
                tab["table"].copy_(host, non_blocking=True)
                tab["key"] = key
            b1, b2 = group["betas"]
            if self._hyper is None:
                for st in tab["states"]:           # the rule counts per parameter: only members that have a gradient advance
                    st["step"] += 1
                step = tab["states"][0]["step"]
                launches = [(step, tab["chunks"], tab["n"])]
                if any(st["step"] != step for st in tab["states"]):
                    launches = self._split_by_step(tab)
                hyper = None
            else:                                  # graph mode: prepare_replay() owns the counters and the device scalars
                if any(st["step"] != tab["states"][0]["step"] for st in tab["states"]):
                    self._check_uniform_steps("step")
                launches = [(max(1, tab["states"][0]["step"]), tab["chunks"], tab["n"])]
                hyper = self._hyper[gi].data_ptr()
            for step, chunks, n in launches:
                lib.call("fiber_adamw_multi_f32", lib.ptr(tab["table"]), lib.ptr(tab["numel"]), lib.ptr(chunks), n,
                         float(group["lr"]), float(group["weight_decay"]), float(b1), float(b2), float(group["eps"]), int(step), hyper)
            ops.restamp_bf16_copies(plist, bump=not bumped)
            bumped = True
        if bumped:
            ops.refresh_transposed_copies()            # every W^T working copy in one launch (233 strided copies per step before)
            ops.refresh_head_major_copies()            # ... and the permuted qkv copies of the window blocks (120 ATen launches per step before)
        return loss


class FiberTorchAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW with `clip_grad_norm_(all parameters, max_grad_norm)` in front of it and (after `attach_ema`) the model EMA
    behind it (reference fine_grained/maskrcnn_benchmark/solver/build.py:8-55, utils/ema.py:36-45), in three launches of
    csrc/solver.hip whatever the grouping: the sum of squares of every gradient, one workgroup that turns it into the norm, the clip
    coefficient and each tensor's {1 - lr wd, lr / (1 - b1^t), 1 / sqrt(1 - b2^t)}, and the update.  Differences from the composition
    it replaces, all deliberate: the gradients are left unscaled (the kernel multiplies as it reads), a step whose gradient norm is not
    finite is skipped (what GradScaler.step does around the reference's optimizer) and counted in `skipped_steps`, and the step counts
    live in device memory -- a skipped step does not advance them and `step()` never synchronises.  `state_dict()` is torch's layout
    (`step` a float32 host scalar, `exp_avg`, `exp_avg_sq`); a state dict of torch.optim.AdamW over the same groups loads and
    continues.  betas and eps are one value for all groups; lr and weight_decay are per group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None):
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"FiberTorchAdamW: max_grad_norm must be positive or None, got {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = max_grad_norm
        self._chunk = None
        self._tab = None                        # the cached device tables (one set for all groups)
        self._block = None                      # device int32[4]: {float norm, float clip coefficient, skip, skipped steps}
        self._ema = None
        self._ema_done = frozenset()            # ids of the parameters whose EMA the last step() wrote
        self.rebuilds = 0

    # ---- logging (device tensors: reading them synchronises, step() does not) -----------------------------------------------
    def _state_block(self):
        if self._block is None:
            dev = next(p for g in self.param_groups for p in g["params"]).device
            self._block = torch.zeros(4, dtype=torch.int32, device=dev)
        return self._block

    @property
    def grad_norm(self):
        return self._state_block()[0:1].view(torch.float32)[0]

    @property
    def clip_coef(self):
        return self._state_block()[1:2].view(torch.float32)[0]

    @property
    def skipped_steps(self):
        return self._state_block()[3]

    def attach_ema(self, model_ema):
        """From now on step() also writes `model_ema`'s copy of every parameter it updates (fiber_amd.solver.ModelEma); the rest --
        parameters without a gradient, frozen ones, buffers -- stays with `model_ema.update()`."""
        self._ema = model_ema
        self._tab = None
        if model_ema is not None:
            model_ema._attached = self

    def take_ema_done(self):
        done, self._ema_done = self._ema_done, frozenset()
        return done

    # ---- state --------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {kk: (torch.tensor(float(vv), dtype=torch.float32) if kk == "step" else vv) for kk, vv in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Loaded moments and step counts live in NEW tensors: drop the cached device tables.  `step` arrives as torch writes it (a
        host float32 scalar, or a number) and goes to the device as int32."""
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = torch.tensor(int(float(st["step"])), dtype=torch.int32).to(p.device)
        self._tab = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tab = None

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise lib.FiberHipError("FiberTorchAdamW needs contiguous fp32 parameters on a HIP device")
            st["step"] = None                  # placed in the table's count array by the rebuild
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @staticmethod
    def _upload(dev_t, host_t):
        # a FRESH pageable host tensor per upload (see FiberAdamW.step): staged before copy_() returns, no synchronisation
        dev_t.copy_(host_t, non_blocking=True)
        return dev_t

    def _rebuild(self, plist, emas):
        self.rebuilds += 1
        dev = plist[0].device
        states = [self._state_of(p) for p in plist]
        sizes = [p.numel() for p in plist]
        n = len(plist)
        chunks = [(i, c) for i, k in enumerate(sizes) for c in range(-(-k // self._chunk))]
        # the counts of all members in ONE int32 array the finalize kernel walks; each state's `step` becomes a view of its word
        zero = torch.zeros((), dtype=torch.int32, device=dev)
        steps = torch.stack([zero if st["step"] is None else st["step"].to(device=dev, dtype=torch.int32).reshape(()) for st in states])
        for i, st in enumerate(states):
            st["step"] = steps[i]
        coef = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        fixed = torch.tensor([(p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), 0, 0 if e is None else e.data_ptr(),
                               coef.data_ptr() + 16 * i) for i, (p, st, e) in enumerate(zip(plist, states, emas))], dtype=torch.int64)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
        return {"key": None, "n": n, "nchunks": len(chunks), "states": states, "fixed": fixed, "steps": steps, "coef": coef,
                "table": new(tuple(fixed.shape), torch.int64), "hyper": None, "lr_wd": new((n, 2), torch.float32),
                "numel": self._upload(new((n,), torch.int64), torch.tensor(sizes, dtype=torch.int64)),
                "chunks": self._upload(new((len(chunks), 2), torch.int32), torch.tensor(chunks, dtype=torch.int32)),
                "partial": new((len(chunks),), torch.float64)}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._chunk is None:
            self._chunk = lib.plain("fiber_adamw_chunk")
        plist, hyper = [], []
        b1, b2 = self.param_groups[0]["betas"]
        eps = self.param_groups[0]["eps"]
        for group in self.param_groups:
            if tuple(group["betas"]) != (b1, b2) or group["eps"] != eps:
                raise lib.FiberHipError("FiberTorchAdamW keeps one betas / eps for all parameter groups")
            if group.get("amsgrad") or group.get("maximize"):     # (keys a loaded torch.optim.AdamW state dict brings along)
                raise lib.FiberHipError("FiberTorchAdamW implements neither amsgrad nor maximize")
            row = (float(group["lr"]), float(group["weight_decay"]))
            for p in group["params"]:
                if p.grad is not None:
                    plist.append(p)
                    hyper.append(row)
        self._ema_done = frozenset()
        if not plist:
            return loss
        grads = []
        for p in plist:
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or not g.is_cuda:
                raise lib.FiberHipError("FiberTorchAdamW needs contiguous fp32 gradients on a HIP device")
            grads.append(g.data_ptr())
        cached = ops.bf16_copy_if_cached
        copies = [cached(p) for p in plist]
        emas = [None] * len(plist) if self._ema is None else [self._ema.ema_of(p) for p in plist]
        for p, e in zip(plist, emas):
            if e is not None and (e.dtype != torch.float32 or not e.is_contiguous() or e.device != p.device or e.shape != p.shape):
                raise lib.FiberHipError("FiberTorchAdamW: the EMA copy of a parameter must be a contiguous fp32 tensor of its shape and device")
        # what the cached tables were built from: parameters, their storage, the state dicts, the EMA tensors
        members = (tuple(map(id, plist)), tuple(p.data_ptr() for p in plist), tuple(id(self.state[p]) for p in plist),
                   tuple(0 if e is None else e.data_ptr() for e in emas))
        key = (members, tuple(grads), tuple(0 if c is None else c.data_ptr() for c in copies))
        tab = self._tab
        if tab is None or tab["members"] != members:
            tab = self._tab = self._rebuild(plist, emas)
            tab["members"] = members
        if tab["key"] != key:                      # gradients are re-allocated every step under zero_grad(set_to_none=True)
            host = tab["fixed"].clone()
            host[:, 1] = torch.tensor(key[1], dtype=torch.int64)
            host[:, 4] = torch.tensor(key[2], dtype=torch.int64)
            self._upload(tab["table"], host)
            tab["key"] = key
        if tab["hyper"] != hyper:                  # every step during warm-up, at a milestone, when the weight-decay schedule fires
            self._upload(tab["lr_wd"], torch.tensor(hyper, dtype=torch.float32))
            tab["hyper"] = hyper
        block = self._state_block()
        max_norm = float("inf") if self.max_grad_norm is None else float(self.max_grad_norm)
        decay = 0.0 if self._ema is None else float(self._ema.decay)
        P = lib.ptr
        with torch.cuda.device(plist[0].device):
            lib.call("fiber_grad_sqnorm_multi_f32", P(tab["table"]), P(tab["numel"]), P(tab["chunks"]), tab["nchunks"], P(tab["partial"]))
            lib.call("fiber_solver_finalize", P(tab["partial"]), tab["nchunks"], max_norm, P(tab["lr_wd"]), P(tab["steps"]), P(tab["coef"]),
                     tab["n"], float(b1), float(b2), P(block))
            lib.call("fiber_adamw_torch_multi_f32", P(tab["table"]), P(tab["numel"]), P(tab["chunks"]), tab["nchunks"], float(b1), float(b2),
                     float(eps), decay, P(block))
        self._ema_done = frozenset(id(p) for p, e in zip(plist, emas) if e is not None)
        # the generation bump makes every other derived copy stale -- the EMA model's own cached bf16 copies among them
        ops.restamp_bf16_copies(plist, bump=True)
        ops.refresh_transposed_copies()
        ops.refresh_head_major_copies()
        return loss
