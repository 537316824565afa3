"""Fused multi-tensor optimisers for the three cases of the reference's factory (base_trainer.py:47-73):
`torch.optim.SGD(param_groups, momentum=MOMENTUM, nesterov=OPT_NESTEROV)` (:63-66) and
`torch.optim.Adam(param_groups, betas=(BETA1, 0.999))` (:57-61) over the four groups of models/basenet.py:73-95.
Same update rules, `param_groups` and `state[p]` layouts as the torch classes (so LR schedules that poke
`param_groups[i]["lr"]` and optimiser checkpoints keep working, in both directions), but one HIP launch per step
(dasac_sgd_step / dasac_sgd_nesterov_step / dasac_adam_step) instead of a chain of foreach passes per group.

Global gradient-norm clipping, norm logging and non-finite step skipping (`max_grad_norm`, `track_grad_norm`, `skip_nonfinite`)
live here too, because with a stash `.grad` never holds the gradient that is applied: dasac_grad_norm measures stash + grad over
the update's own table on the device, and the `_ctl` updates read its verdict from device memory -- no host synchronisation,
no ATen arithmetic, three launches per step instead of one.  `track_tensor_stats` adds the per-tensor view of the same gradients
(dasac_tensor_stats: one more pass over the same table, `tensor_stats`, `last_skipped_stats`, `measure_tensor_stats()`)."""
import ctypes
import math
import numbers

import numpy as np
import torch

from . import lib as L
from . import ops

# columns of `tensor_stats` (include/dasac_hip.h, dasac_tensor_stats); g = stash + grad as the update applies it
TENSOR_STATS_COLUMNS = ("g_sumsq", "g_maxabs", "g_nonfinite", "g_first_nonfinite", "g_zeros", "p_sumsq", "p_maxabs", "s_sumsq")


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the stash of an earlier backward pass' gradients, the walk over the parameters
    that have something to apply, and the upload of the per-step pointer table."""
    MAX_GROUPS = 8
    STATE_KEY = None             # the state tensor whose squared norm the stats table reports

    def __init__(self, params, defaults, max_grad_norm=None, skip_nonfinite=False, track_grad_norm=False, track_tensor_stats=False):
        """The four keywords are attributes of the optimiser, not `param_groups` keys, and are not part of `state_dict()`
        (groups and state keep torch's layout).
        max_grad_norm: None, or a finite float > 0 -- the summed gradient of every step is scaled by
            min(max_grad_norm / (norm + 1e-6), 1), norm = the global L2 norm of stash + grad over all parameters, as
            `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` would scale `.grad` before the step.
        track_grad_norm: measure that norm on every step without clipping (`grad_norm`).
        skip_nonfinite: a step whose norm is Inf or NaN is skipped on the device.  A skipped step leaves parameters and
            moment buffers untouched (FusedSGD fills a momentum buffer that the step would have created with -0.0, which
            makes the next step exactly the first one: momentum * -0.0 + d is d for every d, where +0.0 would turn d = -0.0
            into +0.0), clears the stash as usual and counts in `skipped_steps`.  The host does not learn
            of it: version counters advance, and FusedAdam's `state[p]["step"]` advances too, so the bias corrections of later
            steps are those of one step further on than the moments have seen.  Every rank of a data-parallel run holds the
            same reduced gradients and therefore takes the same decision.
        track_tensor_stats: every step also fills `tensor_stats`, one row of TENSOR_STATS_COLUMNS per parameter, from the
            gradients, parameters and state the update is about to read; with `skip_nonfinite` the table of the last skipped
            step is kept in `last_skipped_stats`.  Read-only: the update is bit for bit what `track_grad_norm` alone gives."""
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, numbers.Real) or not math.isfinite(max_grad_norm) \
                    or not max_grad_norm > 0:
                raise ValueError("{}: max_grad_norm must be None or a finite number > 0, got {!r}".format(type(self).__name__, max_grad_norm))
            max_grad_norm = float(max_grad_norm)
        super().__init__(params, defaults)
        if len(self.param_groups) > self.MAX_GROUPS:
            raise ValueError("{}: at most {} parameter groups".format(type(self).__name__, self.MAX_GROUPS))
        self.max_grad_norm, self.skip_nonfinite, self.track_grad_norm = max_grad_norm, bool(skip_nonfinite), bool(track_grad_norm)
        self.track_tensor_stats = bool(track_tensor_stats)
        self._tables = {}            # slot -> (key, device tensor table, device chunk table, n_tensors, n_chunks, device row_of or None)
        self._stash = {}             # parameter -> gradient of an earlier backward pass, summed inside the next step()
        self._ctl = None             # device control blocks {total, coef, skip, reserved}: [0] of step(), [1] of measure_grad_norm()
        self._skipped = None         # device int64 counter of skipped steps
        self._stats = None           # device fp64 [n_params, 8] tables: [0] of the last step(), [1] of the last skipped step
        self._captured_at = None     # device int64: `skipped_steps` as it stood after the step that [1] describes

    def _controlled(self):
        return self.max_grad_norm is not None or self.skip_nonfinite or self.track_grad_norm or self.track_tensor_stats

    def _control(self):
        if self._ctl is None:
            p = self.param_groups[0]["params"][0]
            L.require_gpu(p)
            self._ctl = torch.zeros(2, 4, dtype=torch.float32, device=p.device)
            self._skipped = torch.zeros((), dtype=torch.int64, device=p.device)
        return self._ctl

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the global L2 norm of stash + grad that the last step() measured, before clipping (0 before
        the first such step; Inf / NaN on a step that `skip_nonfinite` skipped).  A view of the control block: valid until the
        next step().  Reading it does not synchronise."""
        return self._control()[0, 0]

    @property
    def skipped_steps(self):
        """0-dim int64 device tensor: how many steps `skip_nonfinite` has skipped.  Reading it does not synchronise."""
        self._control()
        return self._skipped

    def _param_rows(self):
        """{parameter: its row of the stats tables}: the flattened `param_groups` order."""
        return {p: i for i, p in enumerate(p for group in self.param_groups for p in group["params"])}

    def _stats_tables(self):
        n = sum(len(group["params"]) for group in self.param_groups)
        if self._stats is None or self._stats.shape[1] != n:
            device = self._control().device
            self._stats = torch.zeros(2, n, len(TENSOR_STATS_COLUMNS), dtype=torch.float64, device=device)
            self._captured_at = torch.zeros((), dtype=torch.int64, device=device)
        return self._stats

    @property
    def tensor_stats(self):
        """Device fp64 [n_params, 8] (TENSOR_STATS_COLUMNS; rows in the flattened `param_groups` order): what the last step() of
        a `track_tensor_stats` optimiser measured -- zeros before the first one, and in the row of a parameter that had no
        gradient.  A view: valid until the next step().  Reading it does not synchronise."""
        return self._stats_tables()[0]

    @property
    def last_skipped_stats(self):
        """(table, captured_at): `tensor_stats` of the last step that `skip_nonfinite` skipped, and `skipped_steps` as it stood
        right after that step as a 0-dim int64 device tensor (0: no step skipped yet, the table is zeros).  Filled only with
        `track_tensor_stats` and `skip_nonfinite` both on.  Reading it does not synchronise."""
        return self._stats_tables()[1], self._captured_at

    def _row_of(self, params, index):
        """row_of of dasac_tensor_stats for a table whose rows are `params`: output row -> table row, -1 where nothing is pending."""
        row_of = np.full(len(index), -1, dtype=np.int32)
        row_of[[index[p] for p in params]] = np.arange(len(params), dtype=np.int32)
        return row_of

    def _stats_pass(self, tab, row_bytes, nt, chunks, nc, row_of, table, capture):
        """dasac_tensor_stats over an uploaded table into `table`, on the current stream; capture: also keep a skipped step's."""
        lib = L.load()
        ws = L.workspace(lib.dasac_tensor_stats_workspace(nc), table.device)
        tail = (self._control()[0].data_ptr(), self._stats[1].data_ptr(), self._captured_at.data_ptr(), self._skipped.data_ptr()) \
            if capture else (0, 0, 0, 0)
        L.check(lib.dasac_tensor_stats(tab.data_ptr(), row_bytes, nt, chunks.data_ptr(), nc, row_of.data_ptr(), row_of.numel(),
                                       ws.data_ptr(), ws.numel(), table.data_ptr(), *tail, L.stream_ptr()), "dasac_tensor_stats")

    def _step_table(self, slot, key, rows, sizes, device, params):
        """The table of a step: with `track_tensor_stats` its row_of travels with it, cached under the same key."""
        if not self.track_tensor_stats:
            return self._table(slot, key, rows, sizes, device)
        index = self._param_rows()
        return self._table(slot, key + (len(index),), rows, sizes, device, self._row_of(params, index))

    def _step_stats_pass(self, tab, row_bytes, nt, chunks, nc, row_of):
        """The stats pass of a tracked step: after the norm pass (its skip verdict is in the control block), before the update."""
        self._stats_pass(tab, row_bytes, nt, chunks, nc, row_of, self._stats_tables()[0], self.skip_nonfinite)

    def measure_tensor_stats(self):
        """The table step() would fill now (TENSOR_STATS_COLUMNS per parameter, of stash + grad as it stands, the parameters and
        the state where it exists) as a new device fp64 [n_params, 8] tensor.  Updates nothing, leaves `.grad`, the stash,
        `tensor_stats`, `last_skipped_stats` and the control block alone, does not synchronise, and works whether or not
        `track_tensor_stats` is on."""
        pending = list(self._pending(peek=True))
        index = self._param_rows()
        ctl = self._control()
        if not pending:
            return torch.zeros(len(index), len(TENSOR_STATS_COLUMNS), dtype=torch.float64, device=ctl.device)
        # rows of the 48-byte table; no first-step bit: a state that does not exist yet is simply absent
        states = [self.state.get(p, {}).get(self.STATE_KEY) for _, p, _, _ in pending]
        L.require_gpu(*states)
        rows = [(p.data_ptr(), g.data_ptr(), 0 if g2 is None else g2.data_ptr(), 0 if s is None else s.data_ptr(), p.numel(), gi)
                for (gi, p, g, g2), s in zip(pending, states)]
        key = tuple(v for r in rows for v in r) + (len(index),)
        _, tab, chunks, nt, nc, row_of = self._table("measure_stats", key, np.asarray(rows, dtype=np.int64), [r[4] for r in rows], ctl.device,
                                                     self._row_of([p for _, p, _, _ in pending], index))
        table = torch.empty(len(index), len(TENSOR_STATS_COLUMNS), dtype=torch.float64, device=ctl.device)     # every row is written
        self._stats_pass(tab, 48, nt, chunks, nc, row_of, table, False)
        return table

    def measure_grad_norm(self):
        """The global L2 norm of stash + grad as it stands -- what the next step() would measure -- as a new 0-dim fp32 device
        tensor.  Updates nothing, leaves `.grad`, the stash and `grad_norm` alone, and does not synchronise: the device-side
        stand-in for `clip_grad_norm_(full_grads().values(), inf)` when logging."""
        # rows of the 48-byte table with only what the norm pass reads: g, g2 and n
        pending = list(self._pending(peek=True))
        rows = [(0, g.data_ptr(), 0 if g2 is None else g2.data_ptr(), 0, p.numel(), 0) for _, p, g, g2 in pending]
        ctl = self._control()
        if not rows:
            return torch.zeros((), dtype=torch.float32, device=ctl.device)
        key = tuple(v for r in rows for v in r)
        _, tab, chunks, nt, nc, _ = self._table("measure", key, np.asarray(rows, dtype=np.int64), [r[4] for r in rows], ctl.device)
        self._norm_pass(tab, 48, nt, chunks, nc, ctl[1], 0.0, None)
        return ctl[1, 0].clone()

    def _norm_pass(self, tab, row_bytes, nt, chunks, nc, ctl, max_norm, skipped):
        """dasac_grad_norm over an uploaded table into the control block `ctl`, on the current stream."""
        lib = L.load()
        ws = L.workspace(lib.dasac_grad_norm_workspace(nc), ctl.device)
        L.check(lib.dasac_grad_norm(tab.data_ptr(), row_bytes, nt, chunks.data_ptr(), nc, float(max_norm), ws.data_ptr(), ws.numel(),
                                    ctl.data_ptr(), L.ptr(skipped), L.stream_ptr()), "dasac_grad_norm")

    def _step_norm_pass(self, tab, row_bytes, nt, chunks, nc):
        """The norm pass of a controlled step; returns the tail of the `_ctl` update's arguments."""
        ctl = self._control()[0]
        self._norm_pass(tab, row_bytes, nt, chunks, nc, ctl, self.max_grad_norm or 0.0, self._skipped if self.skip_nonfinite else None)
        return ctl.data_ptr(), int(self.max_grad_norm is not None), int(self.skip_nonfinite), L.stream_ptr()

    def stash_grads(self):
        """Sets the current gradients aside (p.grad becomes None): the next backward pass then ASSIGNS its gradients instead
        of accumulating into the old ones (one `add_` launch per parameter), and step() applies stash + grad in the update
        kernel -- the same single fp32 addition, in AccumulateGrad's operand order."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if p in self._stash:
                        self._stash[p] = self._stash[p] + p.grad
                    else:
                        self._stash[p] = p.grad
                    p.grad = None

    def full_grads(self):
        """{parameter: stash + .grad} -- the gradient the next step() will apply, as the reference's `.grad` would hold it
        after both backward passes (for clipping / norm logging between the last backward and step())."""
        out = {}
        for group in self.param_groups:
            for p in group["params"]:
                g, g2 = p.grad, self._stash.get(p)
                if g is None and g2 is None:
                    continue
                out[p] = g if g2 is None else (g2 if g is None else g2 + g)
        return out

    def zero_grad(self, set_to_none=True):
        self._stash.clear()
        super().zero_grad(set_to_none=set_to_none)

    def _pending(self, peek=False):
        """(group index, parameter, gradient, stashed gradient or None) of every parameter the next step() updates, checked
        and made contiguous.  Nothing has been launched when this raises.  peek: leave `.grad` as it is (a parameter that only
        the stashed pass reached otherwise gets its stashed gradient back as `.grad`)."""
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g, g2 = p.grad, self._stash.get(p)
                if g is None:
                    if g2 is None:
                        continue
                    g, g2 = g2, None                 # only the stashed pass produced a gradient for this parameter
                    if not peek:
                        p.grad = g
                L.require_gpu(p, g, g2)
                if p.dtype != torch.float32 or not p.is_contiguous() or g.is_sparse:
                    raise TypeError(name + ": dense contiguous fp32 parameters only")
                if not g.is_contiguous():
                    g = g.contiguous()
                if g2 is not None and not g2.is_contiguous():
                    g2 = g2.contiguous()
                yield gi, p, g, g2

    def _table(self, slot, key, rows, sizes, device, row_of=None):
        """rows: int64 [n_tensors, k] host array; sizes: element counts -> the (tensor, chunk) list of the multi-tensor kernels;
        row_of: None, or the int32 host array of dasac_tensor_stats, uploaded with them."""
        ent = self._tables.get(slot)
        if ent is None or ent[0] != key:
            chunks = L.chunk_list(sizes, L.load().dasac_ema_chunk_elems())
            # The gradients are fresh allocations every step, so this table is rebuilt every step: upload it through pinned
            # memory without blocking.  A pageable source makes `.to(device)` wait for the WHOLE stream -- the backward pass
            # still running on the device -- and the device then idles while the host catches up (measured: ~3 ms per step).
            up = lambda a: torch.from_numpy(a).pin_memory().to(device, non_blocking=True)
            ent = (key, up(rows), chunks.pin_memory().to(device, non_blocking=True), len(sizes), len(chunks),
                   None if row_of is None else up(row_of))
            self._tables[slot] = ent
        return ent

    def _group_floats(self, name):
        return (ctypes.c_float * len(self.param_groups))(*[float(g[name]) for g in self.param_groups])


class FusedSGD(_FusedOptimizer):
    STATE_KEY = "momentum_buffer"

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, dampening=0.0, max_grad_norm=None,
                 skip_nonfinite=False, track_grad_norm=False, track_tensor_stats=False):
        if dampening != 0.0:
            raise NotImplementedError("FusedSGD: no dampening (the reference never sets it)")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=bool(nesterov))
        super().__init__(params, defaults, max_grad_norm, skip_nonfinite, track_grad_norm, track_tensor_stats)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        momentum, nesterov = self.param_groups[0]["momentum"], bool(self.param_groups[0].get("nesterov"))
        for group in self.param_groups:
            if group["momentum"] != momentum or bool(group.get("nesterov")) != nesterov or group.get("dampening", 0.0) != 0.0 \
                    or group.get("maximize"):
                raise NotImplementedError("FusedSGD: one momentum and one nesterov setting for all groups, no dampening / maximize")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        rows = {True: [], False: []}
        device, keep, touched, owners = None, [], [], {True: [], False: []}
        for gi, p, g, g2 in list(self._pending()):      # every check first: a refusal leaves no half-initialised state
            st = self.state[p]
            first = st.get("momentum_buffer") is None
            if first:
                st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
            device = p.device
            rows[first or momentum == 0.0].append((p.data_ptr(), g.data_ptr(), 0 if g2 is None else g2.data_ptr(),
                                                   st["momentum_buffer"].data_ptr(), p.numel(), gi))
            owners[first or momentum == 0.0].append(p)
            keep += [g, g2]                          # a made-contiguous copy must outlive the queued launch
            touched += [p, st["momentum_buffer"]]
        n = len(self.param_groups)
        lr, wd = self._group_floats("lr"), self._group_floats("weight_decay")
        entry, what = (lib.dasac_sgd_nesterov_step, "dasac_sgd_nesterov_step") if nesterov else (lib.dasac_sgd_step, "dasac_sgd_step")
        if self._controlled():
            # ONE table for the tensors that take their first step and those that do not (bit 32 of `group` tells them apart):
            # the norm is a fact about all of them
            both = [r[:5] + (r[5] | 1 << 32,) for r in rows[True]] + rows[False]
            if both:
                key = tuple(v for r in both for v in r)
                _, tab, chunks, nt, nc, row_of = self._step_table("ctl", key, np.asarray(both, dtype=np.int64), [r[4] for r in both], device,
                                                                  owners[True] + owners[False])
                tail = self._step_norm_pass(tab, 48, nt, chunks, nc)
                if self.track_tensor_stats:
                    self._step_stats_pass(tab, 48, nt, chunks, nc, row_of)
                entry, what = (lib.dasac_sgd_nesterov_step_ctl, "dasac_sgd_nesterov_step_ctl") if nesterov else \
                    (lib.dasac_sgd_step_ctl, "dasac_sgd_step_ctl")
                L.check(entry(tab.data_ptr(), nt, chunks.data_ptr(), nc, ctypes.cast(lr, ctypes.c_void_p),
                              ctypes.cast(wd, ctypes.c_void_p), n, float(momentum), -1, *tail), what)
            elif self.track_tensor_stats and self._stats is not None:
                self._stats[0].zero_()               # a step with nothing pending: every row is that of an absent gradient
            rows = {}
        for first in (True, False):
            if not rows.get(first):
                continue
            key = tuple(v for r in rows[first] for v in r)
            _, tab, chunks, nt, nc, _ = self._table(first, key, np.asarray(rows[first], dtype=np.int64), [r[4] for r in rows[first]], device)
            L.check(entry(tab.data_ptr(), nt, chunks.data_ptr(), nc, ctypes.cast(lr, ctypes.c_void_p),
                          ctypes.cast(wd, ctypes.c_void_p), n, float(momentum), int(first), L.stream_ptr()), what)
        ops.bump_versions(touched)       # raw-pointer writes: keep autograd's version counters (engine cache keys) honest
        self._stash.clear()
        return loss


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam as the reference builds it: L2 weight decay added to the gradient, no amsgrad.  `state[p]` holds
    `step` (a host fp32 tensor, as torch keeps it), `exp_avg` and `exp_avg_sq`; the group keys are torch.optim.Adam's.
    Under `skip_nonfinite` a skipped step leaves `exp_avg` / `exp_avg_sq` alone but still advances the host-side `step`: the
    bias corrections are then one step ahead of the moments (see _FusedOptimizer.__init__)."""
    STATE_KEY = "exp_avg"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False,
                 capturable=False, max_grad_norm=None, skip_nonfinite=False, track_grad_norm=False, track_tensor_stats=False):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("FusedAdam: lr, eps and weight_decay must not be negative")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: betas must lie in [0, 1)")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults, max_grad_norm, skip_nonfinite, track_grad_norm, track_tensor_stats)
        self._hyper()

    def _hyper(self):
        """(beta1, beta2, eps) of the one launch; refuses what the kernel does not do."""
        g0 = self.param_groups[0]
        for group in self.param_groups:
            if any(group.get(k) for k in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")):
                raise NotImplementedError("FusedAdam: no amsgrad / maximize / capturable / differentiable / decoupled weight decay")
            if tuple(group["betas"]) != tuple(g0["betas"]) or group["eps"] != g0["eps"]:
                raise NotImplementedError("FusedAdam: one betas / eps for all groups")
        return float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        beta1, beta2, eps = self._hyper()
        ptrs, scalars, device, keep, touched, steps, owners = [], [], None, [], [], [], []
        for gi, p, g, g2 in list(self._pending()):      # every check first: a refusal leaves no half-initialised state
            st = self.state[p]
            if len(st) == 0:                          # torch/optim/adam.py, _init_group
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            L.require_gpu(m, v)
            if m.dtype != torch.float32 or v.dtype != torch.float32 or not m.is_contiguous() or not v.is_contiguous():
                raise TypeError("FusedAdam: dense contiguous fp32 state only")
            device = p.device
            ptrs.append((p.data_ptr(), g.data_ptr(), 0 if g2 is None else g2.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi))
            steps.append((st, float(self.param_groups[gi]["lr"])))
            owners.append(p)
            keep += [g, g2]                          # a made-contiguous copy must outlive the queued launch
            touched += [p, m, v]
        if ptrs:
            for st, lr in steps:                     # only now: a refusal above leaves every step count as it was
                if not torch.is_tensor(st["step"]):       # a checkpoint from before torch kept `step` as a tensor
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                st["step"] += 1
                step = st["step"].item()
                # the python doubles of adam.py:772-781; each tensor has its own step count (a parameter whose first gradient
                # arrives later takes larger bias corrections than its neighbours)
                scalars.append((lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5))
            rows = np.zeros((len(ptrs), 8), dtype=np.int64)
            rows[:, :7] = np.asarray(ptrs, dtype=np.int64)
            rows.view(np.float32)[:, 14:16] = np.asarray(scalars, dtype=np.float64)         # rounded to fp32 here, once
            key = tuple(v for r in ptrs for v in r) + tuple(v for r in scalars for v in r)
            _, tab, chunks, nt, nc, row_of = self._step_table(0, key, rows, [r[5] for r in ptrs], device, owners)
            wd = self._group_floats("weight_decay")
            if self._controlled():
                tail = self._step_norm_pass(tab, 64, nt, chunks, nc)
                if self.track_tensor_stats:
                    self._step_stats_pass(tab, 64, nt, chunks, nc, row_of)
                L.check(lib.dasac_adam_step_ctl(tab.data_ptr(), nt, chunks.data_ptr(), nc, ctypes.cast(wd, ctypes.c_void_p),
                                                len(self.param_groups), beta1, beta2, eps, *tail), "dasac_adam_step_ctl")
            else:
                L.check(lib.dasac_adam_step(tab.data_ptr(), nt, chunks.data_ptr(), nc, ctypes.cast(wd, ctypes.c_void_p),
                                            len(self.param_groups), beta1, beta2, eps, L.stream_ptr()), "dasac_adam_step")
            ops.bump_versions(touched)   # raw-pointer writes: keep autograd's version counters (engine cache keys) honest
        elif self.track_tensor_stats and self._stats is not None:
            self._stats[0].zero_()                   # a step with nothing pending: every row is that of an absent gradient
        self._stash.clear()
        return loss
