"""Adam in one HIP launch per step (csrc/adam.hip), a drop-in for train.py's torch.optim.Adam.

train.py (:97-100) builds ``torch.optim.Adam(model.parameters(), lr=...)`` and steps it after every
batch.  torch's multi-tensor Adam walks the ~880 parameter tensors (145 M values of the learning
conf) in ~34 kernel launches and reaches ~2.9 TB/s: 1.39 ms of a 13.7 ms captured training step
(profiles/r5_train_step_breakdown_*.txt).  ``Adam`` keeps torch.optim.Adam's update, state names
(``exp_avg``, ``exp_avg_sq``, ``step``) and param-group options, and runs every tensor of a group
in ONE launch from a cached table of (p, grad, exp_avg, exp_avg_sq) pointers; when the gradient tensors
are new ones (zero_grad(set_to_none=True) between steps, or StaticTrainer's per-bucket gradients) only
their pointer column is rewritten (one small host-to-device copy).
Supported: fp32 CUDA parameters, amsgrad=False, maximize=False, a float lr (a Tensor lr raises: it
would need a host read per step); anything else raises (no fallback).  Parameters whose .grad is None
are skipped, as torch.optim.Adam skips them (frozen or unused parameters keep their state).

The device path (any of ``capturable=True``, ``grad_clip_mode``, ``track_grad_norm=True``) is the rest
of train.py's step (:133-152) without a host read: the step counter is a 0-d fp32 device tensor (as
torch's capturable Adam keeps it), ``lr`` may be a 0-d fp32 device tensor that a torch scheduler
refills, ``step(loss=...)`` skips the update on the device unless ``loss > 0``, the global gradient
norm is left in ``optimizer.grad_norm``, and the gradients are clipped as the update reads them
(``p.grad`` stays as the backward wrote it).  A step is kernel launches only -- sum of squares,
its ordered finish, one control kernel and one Adam launch per table -- so it can be captured:
the pointer tables are cached per set of gradient tensors and built before the capture.
``grad_norm``, ``clip_grad_norm_`` and ``clip_grad_value_`` are the same kernels as stand-alone
drop-ins for train.py's cat-and-norm and torch.nn.utils' two functions.
"""
import collections

import numpy as np
import torch

from . import _native

_MAX_GRAD_SETS = 64  # cached pointer tables per parameter set (StaticTrainer keeps <= 32 buckets)


def _chunk_table(sizes, device):
    """gasfm_adam_chunk rows (tensor index, first value) for tensors of these sizes, on the device."""
    t = np.concatenate([np.stack([np.full(-(-n // _native.ADAM_CHUNK), i, np.int64),
                                  np.arange(0, n, _native.ADAM_CHUNK, dtype=np.int64)], 1) for i, n in enumerate(sizes)])
    rows = np.zeros((t.shape[0], 2), dtype=np.int64)  # (int32 tensor | int32 reserved), int64 begin
    rows[:, 0] = t[:, 0]
    rows[:, 1] = t[:, 1]
    return torch.from_numpy(rows).to(device)


def _check_param(p):
    if not p.is_cuda or p.dtype != torch.float32 or p.is_sparse:
        raise TypeError("gasfm_amd.optim: fp32 dense CUDA parameters only")
    if not p.is_contiguous():
        raise TypeError("gasfm_amd.optim: contiguous parameters only")


def _check_grads(grads, device):
    for g in grads:
        if g is None or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.device != device:
            raise TypeError("gasfm_amd.optim: dense contiguous fp32 gradients on the parameters' device")


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


# ------------------------------------------------------------------ stand-alone norm and clipping
_GRAD_TABLES = collections.OrderedDict()  # (device, gradient pointers, sizes) -> tables; pointers, so nothing is kept alive


def _grad_tables(parameters):
    """The cached tables (gasfm_adam_tensor rows with g and numel only, chunks, the partial and total
    buffers) of the gradients of ``parameters``, or None when none has a gradient."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return None
    dev = grads[0].device
    if any(g.dtype != torch.float32 or g.device != dev for g in grads):  # every call: the key holds no dtype
        raise TypeError("gasfm_amd.optim: dense contiguous fp32 gradients on one device")
    key = (dev, tuple(g.data_ptr() for g in grads), tuple(g.numel() for g in grads))
    t = _GRAD_TABLES.get(key)
    if t is None:
        for g in grads:
            _check_param(g)
        _check_grads(grads, dev)
        chunks = _chunk_table(key[2], dev)
        t = {"tensors": torch.tensor([[0, ptr, 0, 0, n] for ptr, n in zip(*key[1:])], dtype=torch.int64).to(dev),
             "chunks": chunks, "n": chunks.shape[0], "dev": dev,
             "partial": torch.empty(max(1, chunks.shape[0]), dtype=torch.float64, device=dev),
             "total": torch.empty(1, dtype=torch.float64, device=dev)}
        _GRAD_TABLES[key] = t
        while len(_GRAD_TABLES) > _MAX_GRAD_SETS:
            _GRAD_TABLES.popitem(last=False)
    else:
        _GRAD_TABLES.move_to_end(key)
    return t


def _norm_of(t):
    norm = torch.empty((), dtype=torch.float32, device=t["dev"])
    _native.grad_sumsq(t["tensors"], t["chunks"], t["n"], t["partial"], norm)
    _native.grad_sumsq_finish(t["partial"], t["n"], t["total"], norm)
    return norm


def grad_norm(parameters):
    """The 2-norm of all gradients of ``parameters`` as a 0-d device tensor, without a host read:
    train.py's ``torch.cat([p.grad.flatten() ...]).norm()`` in two launches, fp64 accumulation in a
    fixed order (two calls are bitwise equal).  Parameters whose .grad is None are skipped."""
    t = _grad_tables(parameters)
    return torch.tensor(0.0) if t is None else _norm_of(t)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for norm_type 2 in three launches: every gradient is multiplied
    by min(1, max_norm / (norm + 1e-6)); returns the norm before clipping (0-d device tensor)."""
    if float(norm_type) != 2.0:
        raise ValueError(f"gasfm_amd.optim.clip_grad_norm_: only norm_type=2 is supported (got {norm_type})")
    if error_if_nonfinite:
        raise NotImplementedError("gasfm_amd.optim.clip_grad_norm_: error_if_nonfinite needs a host read")
    t = _grad_tables(parameters)
    if t is None:
        return torch.tensor(0.0)
    norm = _norm_of(t)
    _native.grad_clip(t["tensors"], t["chunks"], t["n"], "norm", max_norm, norm, norm)
    return norm


def clip_grad_value_(parameters, clip_value, foreach=None):
    """torch.nn.utils.clip_grad_value_ in one launch: every gradient clamped to [-clip_value, clip_value]."""
    t = _grad_tables(parameters)
    if t is not None:
        _native.grad_clip(t["tensors"], t["chunks"], t["n"], "value", clip_value, None, t["total"])


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 maximize=False, capturable=False, grad_clip_mode=None, grad_clip_th=None, track_grad_norm=False):
        if amsgrad or maximize:
            raise NotImplementedError("gasfm_amd.optim.Adam: amsgrad / maximize are not supported")
        if grad_clip_mode not in _native.CLIP_MODES:
            raise ValueError(f"gasfm_amd.optim.Adam: grad_clip_mode {grad_clip_mode!r} (None, 'norm' or 'value')")
        if (grad_clip_mode is None) != (grad_clip_th is None):
            raise ValueError("gasfm_amd.optim.Adam: grad_clip_mode and grad_clip_th go together")
        if grad_clip_th is not None and not grad_clip_th > 0.0:
            raise ValueError(f"gasfm_amd.optim.Adam: grad_clip_th={grad_clip_th}")
        self._device_path = bool(capturable or grad_clip_mode is not None or track_grad_norm)
        if torch.is_tensor(lr) and not self._device_path:
            raise TypeError("gasfm_amd.optim.Adam: a Tensor lr is not supported (pass a float)")
        if not torch.is_tensor(lr) and not 0.0 <= lr:
            raise ValueError(f"gasfm_amd.optim.Adam: lr={lr}")
        if not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"gasfm_amd.optim.Adam: lr={lr}, betas={betas}, eps={eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"gasfm_amd.optim.Adam: invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if self._device_path:
            defaults["capturable"] = True  # StaticTrainer captures the step of an optimizer that says so
        super().__init__(params, defaults)
        self._tables = {}
        self._clip_mode, self._clip_th = grad_clip_mode, grad_clip_th
        self._need_norm = grad_clip_mode == "norm" or bool(track_grad_norm)
        self._ws = None  # device path: the sum-of-squares partials, their total and the norm
        self._retired = []  # outgrown partial buffers and dropped tables that a captured graph may still use
        self.grad_norm = None  # device path with a norm: the last step's pre-clip norm (0-d device tensor)

    def _build(self, ps, grads):
        """Validate the group, create missing state, build the device tables: gasfm_adam_tensor rows as
        int64 [n, 5] (p, g, m, v, numel) and the chunk table.  A later step whose gradient tensors are
        other tensors (p.grad = None between steps) only rewrites column 1 (``_regrad``)."""
        for p, g in zip(ps, grads):
            if not p.is_cuda or p.dtype != torch.float32 or p.is_sparse:
                raise TypeError("gasfm_amd.optim.Adam: fp32 dense CUDA parameters only")
            if not p.is_contiguous():
                raise TypeError("gasfm_amd.optim.Adam: contiguous parameters only")
        steps = {int(self.state[p]["step"]) for p in ps if self.state[p]}
        if len(steps) > 1:
            raise RuntimeError("gasfm_amd.optim.Adam: the parameters of a group are at different steps")
        step = torch.tensor(float(steps.pop() if steps else 0))  # ONE step counter shared by the group
        rows = []
        for p, g in zip(ps, grads):
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] = step
            rows.append([p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()])
        dev = ps[0].device
        tensors = torch.tensor(rows, dtype=torch.int64).to(dev)
        chunks = _chunk_table([p.numel() for p in ps], dev)
        # the entry holds the tensors whose pointers it stores, so their ids stay theirs
        keep = (list(ps), [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps])
        return {"tensors": tensors, "chunks": chunks, "n": chunks.shape[0], "step": step, "keep": keep,
                "grads": None}

    @staticmethod
    def _regrad(t, grads):
        """Point the table at this step's gradient tensors (one host-to-device copy of n pointers)."""
        for g in grads:
            if g is None or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous():
                raise TypeError("gasfm_amd.optim.Adam: dense contiguous fp32 gradients for every parameter")
        ptrs = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        t["tensors"][:, 1].copy_(ptrs.pin_memory().to(t["tensors"].device, non_blocking=True))
        t["grads"] = list(grads)  # keeps them alive, and their ids for the next comparison

    def state_dict(self):
        sd = super().state_dict()
        if self._device_path:
            # one counter per parameter, as torch keeps them: loaded into torch.optim.Adam, a tensor
            # shared by the whole group would be advanced once per parameter
            sd["state"] = {k: {**v, "step": v["step"].clone()} if torch.is_tensor(v.get("step")) else v
                           for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._drop_tables(list(self._tables))  # the moment buffers were replaced

    def _drop_tables(self, keys):
        """Forget cached tables.  On the device path a table that a captured graph reads (pinned) is
        retired, not freed: a replay of that graph then still finds its table, chunks, counter, control
        struct, moments and parameters alive (it updates the state it was captured with)."""
        for k in keys:
            sets = self._tables.pop(k)
            if self._device_path:
                self._retired.extend(t for tabs in sets.values() for t in tabs if t["pinned"])

    # -------------------------------------------------------------------------------- device path
    def _build_device(self, ps, grads, step_value, sibling):
        """One table of the device path: as ``_build`` with the gradient column filled in, a 0-d fp32
        device step counter shared by these parameters and a gasfm_adam_ctl.  ``sibling``: the table of
        the same parameters over another gradient set, whose chunks, counter and control struct it shares."""
        dev = ps[0].device
        for p in ps:
            _check_param(p)
        _check_grads(grads, dev)
        if sibling is None:
            held = [self.state[p].get("step") for p in ps]
            if torch.is_tensor(held[0]) and held[0].device == dev and held[0].dtype == torch.float32 \
                    and held[0].dim() == 0 and all(s is held[0] for s in held):
                step = held[0]
            else:
                step = torch.tensor(float(step_value), dtype=torch.float32, device=dev)
            for p in ps:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] = step
            chunks = _chunk_table([p.numel() for p in ps], dev)
            ctl = torch.zeros(_native.ADAM_CTL_FLOATS, dtype=torch.float32, device=dev)
            keep = (list(ps), [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps])
        else:
            step, chunks, ctl, keep = (sibling[k] for k in ("step", "chunks", "ctl", "keep"))
        rows = [[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()]
                for p, g, m, v in zip(ps, grads, keep[1], keep[2])]
        return {"tensors": torch.tensor(rows, dtype=torch.int64).to(dev), "chunks": chunks, "n": chunks.shape[0],
                "step": step, "ctl": ctl, "keep": keep, "pinned": False}

    def _device_tables(self):
        """[(group, tables)] for the parameters that hold gradients now.  Cached per parameter set and,
        under it, per set of gradient pointers: a table is built once, outside any capture, and a step
        over known gradients copies nothing."""
        plan = []
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]  # torch skips grad-less params
            if not live:
                continue
            grads = [p.grad for p in live]
            dev = live[0].device
            pkey = (gi, tuple(map(id, live)))
            gkey = tuple(g.data_ptr() for g in grads)
            sets = self._tables.get(pkey)
            if sets is None:
                # another subset of this group has gradients now: the cached tables' shared step
                # counters no longer describe every member, so they go
                self._drop_tables([k for k in self._tables if k[0] == gi])
                sets = self._tables[pkey] = collections.OrderedDict()
            tabs = sets.get(gkey)
            if tabs is None:
                if _capturing(dev):
                    raise RuntimeError("gasfm_amd.optim.Adam: these gradient tensors have no pointer table yet; "
                                       "call prepare() or step() with them once before capturing")
                if sets:
                    tabs = [self._build_device(t["keep"][0], [p.grad for p in t["keep"][0]], None, t)
                            for t in next(iter(sets.values()))]
                else:
                    # torch keeps one counter per parameter: split by their current step (one launch each)
                    by_step, seen = {}, {}
                    for p in live:
                        s = self.state[p].get("step") if self.state[p] else None
                        if s is not None and id(s) not in seen:
                            seen[id(s)] = int(s)  # one host read per counter tensor
                        v = 0 if s is None else seen[id(s)]
                        by_step.setdefault(v, []).append(p)
                    tabs = [self._build_device(ps, [p.grad for p in ps], v, None) for v, ps in by_step.items()]
                sets[gkey] = tabs
                for k in [k for k, ts in sets.items() if not ts[0]["pinned"]][:max(0, len(sets) - _MAX_GRAD_SETS)]:
                    del sets[k]
            else:
                sets.move_to_end(gkey)
            if _capturing(dev):
                for t in tabs:
                    t["pinned"] = True  # a graph holds its address: never evicted
            plan.append((group, tabs))
        return plan

    def _workspace(self, dev, n):
        ws = self._ws
        if ws is None:
            ws = self._ws = {"partial": None, "total": torch.zeros(1, dtype=torch.float64, device=dev),
                             "norm": torch.zeros((), dtype=torch.float32, device=dev)}
        if ws["total"].device != dev:
            raise RuntimeError("gasfm_amd.optim.Adam: the device path needs every parameter on one device")
        if ws["partial"] is None or ws["partial"].numel() < n:
            if _capturing(dev):
                raise RuntimeError("gasfm_amd.optim.Adam: workspace too small inside a capture; call prepare() first")
            if ws["partial"] is not None:
                self._retired.append(ws["partial"])
            ws["partial"] = torch.empty(max(1, n), dtype=torch.float64, device=dev)
        return ws

    def prepare(self):
        """Build the tables and the workspace for the current gradient tensors without stepping: what a
        capture of ``step()`` needs to exist beforehand (one host-to-device copy per new table)."""
        if not self._device_path:
            return
        plan = self._device_tables()
        if plan:
            self._workspace(plan[0][1][0]["tensors"].device, sum(t["n"] for _, tabs in plan for t in tabs))

    def _step_device(self, loss):
        plan = self._device_tables()
        if not plan:
            return
        entries = [t for _, tabs in plan for t in tabs]
        dev = entries[0]["tensors"].device
        if loss is not None and not (torch.is_tensor(loss) and loss.device == dev and loss.dtype == torch.float32
                                     and loss.numel() == 1):
            raise TypeError("gasfm_amd.optim.Adam: loss must be a 0-d fp32 tensor on the parameters' device")
        total = None
        if self._need_norm:
            ws = self._workspace(dev, sum(t["n"] for t in entries))
            off = 0
            for t in entries:
                _native.grad_sumsq(t["tensors"], t["chunks"], t["n"], ws["partial"][off:], ws["total"])
                off += t["n"]
            _native.grad_sumsq_finish(ws["partial"], off, ws["total"], ws["norm"])
            total, self.grad_norm = ws["total"], ws["norm"]
        for group, tabs in plan:
            lr = group["lr"]
            if torch.is_tensor(lr) and not (lr.device == dev and lr.dtype == torch.float32 and lr.numel() == 1):
                raise TypeError("gasfm_amd.optim.Adam: a Tensor lr must be a 0-d fp32 tensor on the parameters' device")
            b1, b2 = group["betas"]
            for t in tabs:
                _native.adam_control(t["ctl"], total, loss, lr, t["step"], b1, b2, self._clip_mode, self._clip_th)
                if t["n"]:
                    _native.adam_step_ctl(t["tensors"], t["chunks"], t["n"], t["ctl"], b1, b2, group["eps"],
                                          group["weight_decay"], self._clip_mode, self._clip_th)
                torch.autograd.graph.increment_version(t["keep"][0])

    @torch.no_grad()
    def step(self, closure=None, *, loss=None):
        """loss (device path): a 0-d fp32 device tensor; the update and the step counter are skipped on
        the device unless ``loss > 0`` (train.py's ``if batch_loss.item() > 0``, a NaN loss included)."""
        out = None
        if closure is not None:
            with torch.enable_grad():
                out = closure()
        if self._device_path:
            self._step_device(loss)
            return out
        if loss is not None:
            raise TypeError("gasfm_amd.optim.Adam: step(loss=...) needs the device path (capturable=True)")
        for gi, group in enumerate(self.param_groups):
            if torch.is_tensor(group["lr"]):
                raise TypeError("gasfm_amd.optim.Adam: a Tensor lr is not supported (pass a float)")
            live = [p for p in group["params"] if p.grad is not None]  # torch skips grad-less params
            if not live:
                continue
            key = (gi, tuple(map(id, live)))
            tabs = self._tables.get(key)
            if tabs is None:
                # another subset of this group has gradients now: its cached tables' shared step
                # counters no longer describe every member, so they go; torch keeps one counter per
                # parameter, so the parameters are split by their current step (one launch each)
                for k in [k for k in self._tables if k[0] == gi]:
                    del self._tables[k]
                by_step = {}
                for p in live:
                    by_step.setdefault(int(self.state[p]["step"]) if self.state[p] else 0, []).append(p)
                tabs = [self._build(ps, [p.grad for p in ps]) for ps in by_step.values()]
                self._tables[key] = tabs
            for t in tabs:
                ps = t["keep"][0]
                grads = [p.grad for p in ps]
                if t["grads"] is None or any(a is not b for a, b in zip(grads, t["grads"])):
                    self._regrad(t, grads)
                t["step"] += 1  # in place: every parameter's state["step"]
                b1, b2 = group["betas"]
                _native.adam_step(t["tensors"], t["chunks"], t["n"], group["lr"], b1, b2, group["eps"],
                                  group["weight_decay"], int(t["step"]), ps[0])
                # the kernel wrote p in place behind autograd's back: bump the version counters, as an
                # in-place torch op would (version-keyed caches -- e.g. dense.weight_shadow's bf16
                # shadows -- see it)
                torch.autograd.graph.increment_version(ps)
        return out
