"""The optimizer step on the HIP kernels (csrc/optim.hip): `FusedAdamW`, a drop-in for `torch.optim.AdamW`.

ref: pointcept/utils/optimizer.py (build_optimizer: `OPTIMIZERS.build(cfg, default_args=dict(params=...))` with the
     `param_dicts` learning-rate groups, configs/scannet/CDSegNet.py:143-147) and engines/train.py:216-271 (run_step:
     `scaler.scale(loss).backward(); scaler.unscale_; clip_grad_norm_; scaler.step(optimizer); scaler.update()`).

One step is: unscale (GradScaler's `grad_scale`), skip on a non-finite gradient (`found_inf`), clip by the global 2-norm,
AdamW, and the 16-bit copies of the weights the AMP forward multiplies with - two passes of THIS optimizer over the gradients
with clipping (cdseg_grad_norm, cdseg_adamw_step), one without.  Nothing is read on the host: `step` has no `.item()` and no
synchronisation.  (Under `scaler.step`, `found_inf` is still GradScaler's: torch makes its own pass over every gradient to
produce it before it calls `step`; the non-finite flag of cdseg_grad_norm, `last_nonfinite`, is informative only.)  The update formula and the fixed summation order of the norm are written out in include/cdseg.h.

Differences from the reference's run_step, both opt-in:
  * `max_grad_norm` clips the UNSCALED gradients inside the step.  The reference's trainer calls `clip_grad_norm_` itself
    in front of `scaler.step`, on gradients that are still scaled unless `scaler.unscale_` ran; that route keeps working
    (it is torch code in front of `step`), then leave `max_grad_norm` None.
  * `shadow16` keeps a 16-bit copy of every weight matrix current, so that the AMP forward (`train_graph._Linear16` /
    `_SubMConv16`) does not cast the weights again.  A copy is used only while storage address, shape, dtype and
    `Tensor._version` of the weight are the ones recorded at the last step.  A change made through `.data` (or a raw pointer)
    does NOT move `_version` - `train._derived` has the same limitation; call `refresh_shadows()` after such a change.
    `load_state_dict` drops every recorded version (checkpoint loading rewrites weights through `.data` next to it): the
    forward casts again until the next `step` or `refresh_shadows()`.  A `step` leaves every copy current, also when
    GradScaler's `found_inf` makes the device skip it: copies that were not current going in (their weight moved, or they
    were forgotten) are cast again behind the kernel, whatever the device decided.
"""
import ctypes
import weakref

import torch

from . import _lib, ops
from ._lib import OPT_CLIP, OPT_SKIP, OptGroup, OptTensor, check

_SHADOWS = {}  # data_ptr of a weight -> [shape, 16-bit copy, recorded _version, weakref of the registered tensor object]


def _drop_shadow(key, ref):
    ent = _SHADOWS.get(key)
    if ent is not None and ent[3] is ref:  # (an entry that another, live tensor object of the same storage made stays)
        del _SHADOWS[key]


def register_shadow(weight, copy):
    """Record `copy` (16-bit, same shape) as the current 16-bit copy of the fp32 tensor `weight`, at its present `_version`.
    The entry goes when the tensor OBJECT that registered it last is collected."""
    if copy.shape != weight.shape or weight.dtype != torch.float32 or not ops.is_lp(copy.dtype):
        raise ValueError("register_shadow: an fp32 tensor and a 16-bit tensor of the same shape")
    key = weight.data_ptr()
    ent = _SHADOWS.get(key)
    if ent is not None and ent[3]() is weight:
        ent[:3] = [weight.shape, copy, weight._version]
        return
    ref = weakref.ref(weight)
    _SHADOWS[key] = [weight.shape, copy, weight._version, ref]
    weakref.finalize(weight, _drop_shadow, key, ref)


def shadow16(tensor, dtype):
    """The registered 16-bit copy of `tensor`, or None: only when the storage address, the shape, the dtype (fp32 source,
    `dtype` copy) and the recorded `_version` all match.  (`.data` writes do not move `_version`: see the module docstring.)"""
    ent = _SHADOWS.get(tensor.data_ptr())
    if ent is None or tensor.dtype != torch.float32 or ent[0] != tensor.shape or ent[1].dtype != dtype or ent[2] != tensor._version:
        return None
    return ent[1]


def _aligned_offsets(sizes, quantum):
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + quantum - 1) // quantum * quantum
    return offs, total


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's update (decoupled weight decay, bias correction, eps outside the square root) in one HIP pass.

    params / lr / betas / eps / weight_decay: as torch.optim.AdamW, parameter groups included; `group["lr"]` is read on every
        step, so learning-rate schedulers work unchanged.
    max_grad_norm, clip_params: clip the (unscaled) gradients of `clip_params` (default: every parameter) by their global
        2-norm inside the step; `last_grad_norm` / `last_clip_coef` are 0-dim device tensors afterwards.
    shadow16: "f16" | "bf16" - keep the 16-bit copies of every parameter with dim() >= 2 (module docstring).
    State: `step`, `exp_avg`, `exp_avg_sq` per parameter with torch's names and shapes (views into three flat buffers), so a
        `state_dict()` of torch.optim.AdamW loads here and the other way round.
    GradScaler: `scaler.step(opt)` hands over `grad_scale` / `found_inf` (the protocol of torch's fused optimizers): no host
        read; after `scaler.unscale_(opt)` `grad_scale` is None and the step does not unscale again."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_grad_norm=None, clip_params=None, shadow16=None):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedAdamW: a tensor lr would be read on the host every step; pass a float")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"FusedAdamW: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError(f"FusedAdamW: max_grad_norm={max_grad_norm}")
        if shadow16 not in (None,) + _lib.VARIANTS:
            raise ValueError(f"FusedAdamW: shadow16={shadow16!r} (None, 'f16' or 'bf16')")
        self._built = False
        # the keys torch.optim.AdamW keeps in a group, so that the two state_dicts are interchangeable
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._check_groups()
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.variant = shadow16
        self._flat = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if len(self.param_groups) > 16:
            raise NotImplementedError("FusedAdamW: more than 16 parameter groups (CDSEG_OPT_MAX_GROUPS)")
        devs = {p.device for p, _ in self._flat}
        if len(devs) != 1:
            raise NotImplementedError(f"FusedAdamW: the parameters of one optimizer live on one device, got {sorted(map(str, devs))}")
        self.device = devs.pop()
        for p, _ in self._flat:
            if p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous():
                raise NotImplementedError(f"FusedAdamW: parameters are dense contiguous fp32 tensors, got {p.dtype} {tuple(p.shape)}")
        ids = {id(p) for p, _ in self._flat}
        if clip_params is None:
            clip = ids
        else:
            clip = {id(p) for p in clip_params}
            if not clip <= ids:
                raise ValueError("FusedAdamW: clip_params holds tensors that are not parameters of this optimizer")
        self._clip = [max_grad_norm is not None and id(p) in clip for p, _ in self._flat]
        # state: views into three flat buffers (every tensor on a 16-byte boundary)
        sizes = [p.numel() for p, _ in self._flat]
        offs, total = _aligned_offsets(sizes, 4)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._m, self._v, self._steps = torch.zeros(total, **f32), torch.zeros(total, **f32), torch.zeros(len(sizes), **f32)
        self._views = [dict(step=self._steps[i], exp_avg=self._m[o:o + n].view_as(p), exp_avg_sq=self._v[o:o + n].view_as(p))
                       for i, ((p, _), o, n) in enumerate(zip(self._flat, offs, sizes))]
        self._shadow = [None] * len(sizes)
        if shadow16 is not None:
            which = [i for i, (p, _) in enumerate(self._flat) if p.dim() >= 2]
            offs16, total16 = _aligned_offsets([sizes[i] for i in which], 8)
            self._p16 = torch.zeros(total16, dtype=ops.LP_DTYPES[shadow16], device=self.device)
            for i, o in zip(which, offs16):
                self._shadow[i] = self._p16[o:o + sizes[i]].view_as(self._flat[i][0])
            self.refresh_shadows()
        self._table = None  # built on the first step (needs the library and the device)
        self.last_grad_norm = self.last_clip_coef = None
        self._built = True

    def _check_groups(self):
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or g.get("capturable"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize / differentiable / capturable are not implemented "
                                          "(torch.optim.AdamW has them)")

    def add_param_group(self, param_group):
        if getattr(self, "_built", False):
            raise NotImplementedError("FusedAdamW: parameter groups are fixed at construction (the state lives in flat buffers)")
        super().add_param_group(param_group)

    # ------------------------------------------------------------------ 16-bit weight copies
    def refresh_shadows(self):
        """Rewrite every 16-bit copy from its weight (the library's cast: saturating in the half build) and record the
        weights' present versions - after a change that `Tensor._version` does not see (`.data`, checkpoint loading)."""
        if self.variant is None:
            return
        ops._need_gpu(*[p for p, _ in self._flat])
        with _lib.use(self.variant):
            lib = _lib.load()
            for (p, _), s in zip(self._flat, self._shadow):
                if s is not None:
                    self._cast_shadow(lib, p, s)

    def _cast_shadow(self, lib, p, s):
        check(lib.cdseg_cast(ops._ptr(p), _lib.F32, ops._ptr(s), _lib.BF16, p.numel(), ops._stream()), "cast")
        register_shadow(p, s)

    def _forget_shadows(self):
        for (p, _), s in zip(self._flat, self._shadow):
            ent = _SHADOWS.get(p.data_ptr())
            if s is not None and ent is not None and ent[1] is s:
                ent[2] = -1

    # ------------------------------------------------------------------ state
    def load_state_dict(self, state_dict):
        """Accepts a state_dict of torch.optim.AdamW or of this class: the loaded moments are copied into the flat buffers."""
        super().load_state_dict(state_dict)
        self._check_groups()
        with torch.no_grad():
            for (p, _), view in zip(self._flat, self._views):
                st = self.state.get(p)
                if st is not None and len(st):
                    if st["exp_avg"] is not view["exp_avg"]:
                        view["exp_avg"].copy_(st["exp_avg"])
                        view["exp_avg_sq"].copy_(st["exp_avg_sq"])
                        step = st["step"]
                        view["step"].copy_(step) if isinstance(step, torch.Tensor) else view["step"].fill_(float(step))
                    self.state[p] = view
                else:
                    for t in view.values():
                        t.zero_()
                    self.state.pop(p, None)
        self._forget_shadows()

    def _prepare(self):
        lib = _lib.load(self.variant)
        count = len(self._flat)
        sizes = (ctypes.c_long * count)(*[p.numel() for p, _ in self._flat])
        nchunks = ctypes.c_long()
        check(lib.cdseg_opt_chunks(sizes, count, None, ctypes.byref(nchunks)), "opt_chunks")
        chunks = (ctypes.c_int32 * (2 * nchunks.value))()
        check(lib.cdseg_opt_chunks(sizes, count, chunks, ctypes.byref(nchunks)), "opt_chunks")
        self._nchunks = nchunks.value
        self._chunks = torch.tensor(list(chunks), dtype=torch.int32).to(self.device)  # uploaded once per optimizer
        self._ws = ops._scratch(max(256, lib.cdseg_opt_ws_bytes(count, self._nchunks)), self.device)
        self._out = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.last_grad_norm, self.last_clip_coef, self.last_nonfinite = self._out[0], self._out[1], self._out[2]
        # two host tables, taken in turn: the library copies a table with hipMemcpyAsync from pageable memory, which the
        # runtime stages before it returns (include/cdseg.h); the table a step fills is not the one the last step handed over
        self._tables = [(OptTensor * count)(), (OptTensor * count)()]
        self._table = self._tables[0]
        self._groups = (OptGroup * len(self.param_groups))()
        for table in self._tables:
            for e, (p, gi), view, s in zip(table, self._flat, self._views, self._shadow):
                e.p, e.m, e.v, e.step = p.data_ptr(), view["exp_avg"].data_ptr(), view["exp_avg_sq"].data_ptr(), view["step"].data_ptr()
                e.p16 = None if s is None else s.data_ptr()
                e.n, e.group = p.numel(), gi

    def _amp_scalar(self, name):
        t = getattr(self, name, None)
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or t.numel() != 1:
            raise NotImplementedError(f"FusedAdamW: {name} must be one fp32 value on {self.device} (GradScaler sets it so)")
        return t

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device.type != "cuda":
            raise _lib.CdsegError("FusedAdamW.step runs on the GPU only (HIP kernels); the parameters are CPU tensors")
        self._check_groups()
        if self._table is None:
            self._prepare()
        keep, stepped = [], []
        table = self._table = self._tables[1] if self._table is self._tables[0] else self._tables[0]
        for e, (p, _), clip in zip(table, self._flat, self._clip):
            g = p.grad
            if g is None:
                e.g, e.flags = e.p, OPT_SKIP  # (never read)
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != self.device:
                raise NotImplementedError("FusedAdamW: gradients are dense fp32 tensors on the parameters' device "
                                          f"(got {'sparse ' if g.is_sparse else ''}{g.dtype} on {g.device})")
            if e.p != p.data_ptr():
                raise _lib.CdsegError("FusedAdamW: a parameter's storage moved since the first step (the kernels hold addresses)")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            e.g, e.flags = g.data_ptr(), (OPT_CLIP if clip else 0)
            stepped.append(p)
        if not stepped:
            return loss
        for ge, g in zip(self._groups, self.param_groups):
            if isinstance(g["lr"], torch.Tensor):
                raise NotImplementedError("FusedAdamW: a tensor lr would be read on the host every step; pass a float")
            ge.lr, (ge.beta1, ge.beta2), ge.eps, ge.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        scale, found = self._amp_scalar("grad_scale"), self._amp_scalar("found_inf")
        current = [s is not None and shadow16(p, s.dtype) is s for (p, _), s in zip(self._flat, self._shadow)]
        count, ng = len(self._flat), len(self.param_groups)
        ws, wsb = ops._ptr(self._ws), self._ws.numel()
        lib = _lib.load(self.variant)
        st = ops.bind_stream()
        try:
            coef = None
            if self.max_grad_norm is not None:
                check(lib.cdseg_grad_norm(table, count, ops._ptr(self._chunks), self._nchunks, ops._ptr(scale),
                                          self.max_grad_norm, ops._ptr(self._out), ws, wsb, st), "grad_norm")
                coef = ctypes.c_void_p(self._out.data_ptr() + 4)
            check(lib.cdseg_adamw_step(table, count, self._groups, ng, ops._ptr(self._chunks), self._nchunks,
                                       ops._ptr(scale), ops._ptr(found), coef, ws, wsb, st), "adamw_step")
            # Copies that were NOT current going in (their weight moved since the last step, or load_state_dict forgot
            # them) and that the kernel has not certainly written are cast here, behind it on the same stream: those of
            # weights without a gradient, and, under found_inf, all of them - the device may skip the step (nothing stored)
            # and the host cannot know.  A copy that was current stays current whatever the device decided.
            for (p, _), s, was_current in zip(self._flat, self._shadow, current):
                if s is not None and not was_current and (p.grad is None or found is not None):
                    self._cast_shadow(lib, p, s)
        finally:
            ops.unbind_stream()
        # the kernels wrote through raw pointers: move the versions that train._derived and shadow16() key on
        written = [s for (p, _), s in zip(self._flat, self._shadow) if s is not None and p.grad is not None]
        torch.autograd.graph.increment_version(stepped + written)
        for (p, _), s, view in zip(self._flat, self._shadow, self._views):
            if p.grad is not None:
                if s is not None:
                    register_shadow(p, s)
                if p not in self.state or not len(self.state[p]):
                    self.state[p] = view
        return loss
