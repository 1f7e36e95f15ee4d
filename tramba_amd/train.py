"""Training-step pieces of the reference's train.py, device-resident (no .cpu() sync per step).

loss:       train.py:76-85 -- every output bilinearly resized to the label size, then
            binary_cross_entropy_with_logits + iou_loss (utils/loss.py:6-11), weights 1.
            `SodLoss` selects the reference's other two losses instead (structure_loss, wbce: utils/loss.py:14-42).
optimizer:  train.py:266-280 -- Adam, parameters whose name contains "encoder" at 0.1 x lr.
lr decay:   utils/lr.py:1-17.
epoch loop, resume / best-MAE checkpoint files: train.py:212-263.
"""
import os

import torch
import torch.nn.functional as F

from . import hip
from .modules import refresh_dw_packs, refresh_lowp_shadows


def iou_loss(pred, mask):
    """utils/loss.py:6-11."""
    pred = torch.sigmoid(pred)
    inter = (pred * mask).sum(dim=(2, 3))
    union = (pred + mask).sum(dim=(2, 3))
    return (1 - (inter + 1) / (union - inter + 1)).mean()


class _UpsampleBilinearHIP(torch.autograd.Function):
    """F.interpolate(x, size, mode="bilinear") with the library's backward (a gather per input pixel; torch's scatters with
    float atomics, 183 us per deep-supervision output at batch 8)."""

    @staticmethod
    def forward(ctx, x, size):
        ctx.in_hw = tuple(x.shape[-2:])
        return F.interpolate(x, size, mode="bilinear")

    @staticmethod
    def backward(ctx, g):
        from . import hip
        return hip.upsample_bilinear_bwd(g, *ctx.in_hw), None


def _resize_bilinear(o, size):
    """train.py:78-79: the deep-supervision outputs resized to the label"""
    if o.is_cuda and o.dtype == torch.float32 and o.requires_grad and size[0] >= o.shape[-2] and size[1] >= o.shape[-1]:
        return _UpsampleBilinearHIP.apply(o, tuple(size))
    return F.interpolate(o, size, mode="bilinear")


class _SodLossHIP(torch.autograd.Function):
    """The whole loss of train.py:76-85 in the library: three sums per image and output in one pass each (the resized logit
    map is never stored), one finishing block, and in the backward one gather per output that lands on the output's own
    resolution.  ~10 launches where the framework issued ~140.
    With a weight map the weighted losses through the same passes (five sums): `wmap` is the caller's (one launch per loss
    call, shared by the outputs) and form = (eps, per_pixel, with_iou, weight_is_raw).  wmap None: no map is formed or read."""

    @staticmethod
    def forward(ctx, label, wmap, weights, form, *outs):
        if wmap is None:
            loss, coefs = hip.sod_loss(outs, label, weights)
        else:
            eps, per_pixel, with_iou, raw = form
            loss, coefs = hip.sod_wloss(outs, label, wmap, weights, eps, per_pixel, with_iou, raw)
            ctx.form = (eps, raw)
        ctx.save_for_backward(label, wmap, coefs, *outs)
        return loss

    @staticmethod
    def backward(ctx, gl):
        label, wmap, coefs, *outs = ctx.saved_tensors
        gl = gl.to(torch.float32).contiguous()

        def grad(o, coef):
            if wmap is None:
                return hip.sod_loss_grad(o, label, coef, gl)
            return hip.sod_wloss_grad(o, label, wmap, coef, gl, *ctx.form)
        return (None,) * 4 + tuple(grad(o, coefs[i]) if ctx.needs_input_grad[4 + i] else None for i, o in enumerate(outs))


def _loss_on_device(outputs, label):
    """the library's loss takes logit maps no larger than the label, plane for plane"""
    # (a resized output's gradient kernel holds rows of the label in LDS: labels wider than 4096 only with outputs at label size)
    return (label.is_cuda and label.dim() == 4 and 0 < len(outputs) <= 8 and label.shape[0] * label.shape[1] <= 512
            and all(o.is_cuda and o.dim() == 4 and o.shape[:2] == label.shape[:2] and o.shape[-2] <= label.shape[-2]
                    and o.shape[-1] <= label.shape[-1] for o in outputs)
            and (label.shape[-1] <= 4096 or all(o.shape[-2:] == label.shape[-2:] for o in outputs)))


def _device_loss(outputs, label, wmap, loss_weights, form=None):
    weights = None if loss_weights is None else tuple(float(w) for w in loss_weights)
    return _SodLossHIP.apply(label, wmap, weights, form, *[o.float().contiguous() for o in outputs])


def _composed_loss(outputs, label, dtype, loss_weights, term):
    """host tensors / shapes the kernels refuse: term(output in `dtype`, at label size), summed with the loss weights"""
    h, w = label.shape[-2:]
    total = None
    for i, o in enumerate(outputs):
        o = o.to(dtype)
        if o.shape[-2:] != (h, w):
            o = _resize_bilinear(o, (h, w))
        t = term(o)
        if loss_weights is not None:
            t = t * loss_weights[i]
        total = t if total is None else total + t
    return total


def tramba_loss(outputs, label, loss_weights=None):
    """Sum over the deep-supervision outputs (3 for Tramba-R, 4 otherwise) of BCE-with-logits + IoU."""
    outputs = list(outputs)
    if loss_weights is not None and len(loss_weights) != len(outputs):
        raise ValueError(f"tramba_loss: {len(loss_weights)} loss weights for {len(outputs)} outputs")
    if _loss_on_device(outputs, label):
        return _device_loss(outputs, label.float().contiguous(), None, loss_weights)
    # the outputs in fp32 against the label as it is
    return _composed_loss(outputs, label, torch.float32, loss_weights,
                          lambda o: F.binary_cross_entropy_with_logits(o, label) + iou_loss(o, label))


# ----------------------------------------------------------------------------- structure loss / weighted BCE
# utils/loss.py:14-42.  The reference calls F.binary_cross_entropy_with_logits(..., reduce='none'): `reduce` is the legacy
# argument and a non-empty string is true, so the call returns the batch MEAN and the weight cancels out of the BCE term
# (lines 27-28, 40-41).  bce="reference" is that loss as it executes -- what continues a reference experiment;
# bce="pixel" weights the BCE pixel by pixel, the loss as published (F3Net).
_WLOSS_KINDS = {"structure": (31, 0.001, True), "wbce": (15, 0.0, False)}      # kind: (box window, label smoothing, IoU term)
_WLOSS_READINGS = ("reference", "pixel")


def _weighted_term(o, label, weit, eps, with_iou, per_pixel):
    """one output at label size against the label: utils/loss.py:26-34 (40-42 without the IoU term)"""
    bce = F.binary_cross_entropy_with_logits(o, (1 - eps) * label + eps / 2, reduction="none" if per_pixel else "mean")
    if per_pixel:
        bce = ((weit * bce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))).mean()
    if not with_iou:
        return bce
    p = torch.sigmoid(o)
    inter = ((p * label) * weit).sum(dim=(2, 3))
    union = ((p + label) * weit).sum(dim=(2, 3))
    return bce + (1 - (inter + 1) / (union - inter + 1)).mean()


def _weighted_loss(kind, bce, outputs, label, weight=None, loss_weights=None):
    if kind not in _WLOSS_KINDS:
        raise ValueError(f"unknown weighted loss {kind!r}: one of {sorted(_WLOSS_KINDS)}")
    if bce not in _WLOSS_READINGS:
        raise ValueError(f"bce={bce!r}: 'reference' (the loss as utils/loss.py executes) or 'pixel' (per-pixel weights)")
    k, eps, with_iou = _WLOSS_KINDS[kind]
    if weight is not None and kind != "structure":
        raise ValueError("only structure_loss takes a caller's weight (utils/loss.py:15)")
    outputs = list(outputs)
    if loss_weights is not None and len(loss_weights) != len(outputs):
        raise ValueError(f"{kind}: {len(loss_weights)} loss weights for {len(outputs)} outputs")
    per_pixel = bce == "pixel"
    if _loss_on_device(outputs, label) and (weight is None or (weight.is_cuda and weight.shape == label.shape)):
        lab = label.float().contiguous()
        wmap = hip.loss_weight_map(lab, k) if weight is None else weight.detach().float().contiguous()
        return _device_loss(outputs, lab, wmap, loss_weights, (eps, per_pixel, with_iou, weight is not None))
    # host tensors / shapes the kernels refuse: the reference's own composition.  The LABEL picks the precision, as
    # tramba_loss's .float() does: fp64 only when the label is fp64 (fp64 logits against an fp32 label compute in fp32),
    # fp32 for every other label dtype, bf16 logits included
    dtype = torch.float64 if label.dtype == torch.float64 else torch.float32
    label = label.to(dtype)
    if weight is None:
        weit = 1 + 5 * torch.abs(F.avg_pool2d(label, kernel_size=k, stride=1, padding=k // 2) - label)
    else:
        weit = 1 + 5 * weight.to(dtype)
    return _composed_loss(outputs, label, dtype, loss_weights, lambda o: _weighted_term(o, label, weit, eps, with_iou, per_pixel))


def structure_loss(pred, mask, weight=None, bce="reference"):
    """utils/loss.py:15-34 (L_STR): BCE against the smoothed labels + IoU weighted by 1 + 5 |avg_pool31(mask) - mask|, or by
    1 + 5 `weight`.  bce="reference": what the reference computes (its BCE term is the unweighted batch mean, see above);
    bce="pixel": the BCE weighted pixel by pixel.  On a HIP device the library's kernels, elsewhere a torch composition in
    fp32 -- in fp64 only when `mask` is fp64 (the mask, not `pred`, picks the precision).
    `weight` on the device must be a device tensor of exactly `mask`'s shape; any other `weight` (a host tensor, a shape
    that only broadcasts) takes the torch composition, as shapes the kernels refuse do in `tramba_loss`.  The kernels treat
    `weight` as a constant: no gradient flows to it on the device (the composition, like the reference, would give one)."""
    return _weighted_loss("structure", bce, [pred], mask, weight)


def wbce(pred, mask, bce="reference"):
    """utils/loss.py:38-42 (L_wBCE), window 15, no smoothing; bce="reference" is plain mean BCE (the weight cancels)."""
    return _weighted_loss("wbce", bce, [pred], mask)


class SodLoss:
    """Which loss a training step uses over the deep-supervision outputs: each output against the full-size label, the terms
    summed with `loss_weights`, as `tramba_loss` does.

      kind  "bce_iou"    BCE-with-logits + IoU (train.py:76-85): exactly `tramba_loss`, through the same kernels;
            "structure"  utils/loss.py:15-34;      "wbce"  utils/loss.py:38-42;
      bce   "reference" | "pixel": the two readings of the weighted BCE term (see `structure_loss`); no effect on "bce_iou".

    `loss(outputs, label, weight=None)`; `weight` only with kind="structure" (utils/loss.py:23-24)."""

    def __init__(self, kind="bce_iou", bce="reference", loss_weights=None):
        if kind != "bce_iou" and kind not in _WLOSS_KINDS:
            raise ValueError(f"SodLoss: kind={kind!r}: one of 'bce_iou', 'structure', 'wbce'")
        if bce not in _WLOSS_READINGS:
            raise ValueError(f"SodLoss: bce={bce!r}: 'reference' or 'pixel'")
        self.kind, self.bce = kind, bce
        self.loss_weights = None if loss_weights is None else tuple(float(w) for w in loss_weights)

    def __call__(self, outputs, label, weight=None):
        if self.kind == "bce_iou":
            if weight is not None:
                raise ValueError("SodLoss('bce_iou') takes no weight")
            return tramba_loss(outputs, label, self.loss_weights)
        return _weighted_loss(self.kind, self.bce, outputs, label, weight, self.loss_weights)

    def __repr__(self):
        return f"SodLoss(kind={self.kind!r}, bce={self.bce!r}, loss_weights={self.loss_weights!r})"


def _step_loss(loss, outputs, label):
    """the loss of a training step: `loss` is a SodLoss, None = tramba_loss.  Nothing else: a step may be recorded into a
    hipGraph, and only the spec's own paths are known to be capture-safe"""
    if loss is None:
        return tramba_loss(outputs, label)
    if not isinstance(loss, SodLoss):
        raise TypeError(f"loss={loss!r}: a tramba_amd.train.SodLoss or None")
    return loss(outputs, label)


class Adam(torch.optim.Adam):
    """torch.optim.Adam -- constructor, param_groups, per-parameter state {step, exp_avg, exp_avg_sq} and state_dict as the
    reference's optimizer (train.py:266-280) -- whose step() is the library's multi-tensor kernel (tramba_adam_step): one
    read of the gradient and one read + write of p / exp_avg / exp_avg_sq at HBM speed (torch's `fused=True` form ran the
    111 M parameters of Tramba-V at 2.7 TB/s in 27 launches), the bias corrections in fp64 as torch computes them.  The step
    counters live on the device (what torch does for `capturable` / `fused`), so a step can be recorded into a hipGraph.
    fp32 parameters on a HIP device only; amsgrad / maximize / differentiable are not implemented (the reference uses none)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable)
        self._plans = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}          # the state tensors have been replaced

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plans = {}

    def _plan(self, gi, ps):
        """pointer arrays of the parameters and their state for group gi: rebuilt when the set of parameters with a
        gradient or an address changes (the state tensors only change through load_state_dict)"""
        ptrs = [p.data_ptr() for p in ps]
        plan = self._plans.get(gi)
        if plan is not None and plan[0] == ptrs:
            # the state entries may have been replaced behind the optimizer's back (opt.state.clear(), a hand-made restore):
            # the plan must never keep updating orphaned tensors
            ms, vs, steps = plan[6]
            if all((st := self.state.get(p)) and st.get("exp_avg") is m and st.get("exp_avg_sq") is v and st.get("step") is t
                   for p, m, v, t in zip(ps, ms, vs, steps)):
                return plan
        ms, vs, steps = [], [], []
        for p in ps:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise hip.TrambaHipError("Adam: contiguous fp32 parameters on a HIP device only (no CPU fallback)")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not torch.is_tensor(st["step"]) or st["step"].device != p.device or st["step"].dtype != torch.float32:
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())   # a non-capturable checkpoint
            for k in ("exp_avg", "exp_avg_sq"):
                if st[k].dtype != torch.float32 or st[k].device != p.device or not st[k].is_contiguous() or st[k].numel() != p.numel():
                    raise hip.TrambaHipError(f"Adam: state '{k}' does not match its parameter {tuple(p.shape)}")
            ms.append(st["exp_avg"])
            vs.append(st["exp_avg_sq"])
            steps.append(st["step"])
        import ctypes
        n = len(ps)
        plan = (ptrs, hip.pointer_array(ps), hip.pointer_array(ms), hip.pointer_array(vs), hip.pointer_array(steps),
                (ctypes.c_int64 * n)(*[p.numel() for p in ps]), (ms, vs, steps))
        self._plans[gi] = plan
        return plan

    @torch.no_grad()
    def step(self, closure=None, gscale=None, skip=None, sched=None, ema=None):
        """`gscale` (fp32) / `skip` (int32): 0-dim device tensors read by the kernel when it runs -- every gradient is
        multiplied by the first before anything else, a non-zero second leaves parameters, moments and step counters as
        they are (StepControl hands both over; a captured step follows their values at replay).
        `sched`: a tramba_step_sched record on the device (hip.step_sched_record) -- every group steps at its lr times
        the record's lr_factor, read when the kernel runs.  `ema` (needs `sched`): a mapping parameter -> fp32 average of
        its size; the averages of the parameters this step updates move in the same pass by the record's ema_weight.
        With neither, the step runs the launches it always ran."""
        if ema is not None and sched is None:
            raise hip.TrambaHipError("Adam: an EMA needs the schedule record (its weight lives there)")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
                raise hip.TrambaHipError("Adam: amsgrad / maximize / differentiable are not implemented")
            ps = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
            if not ps:
                continue
            grads = [p.grad for p in ps]
            for p, g in zip(ps, grads):
                if g.dtype != torch.float32 or g.layout != torch.strided or not g.is_contiguous() or g.numel() != p.numel():
                    raise hip.TrambaHipError("Adam: dense contiguous fp32 gradients only")
            plan = self._plan(gi, ps)
            b1, b2 = group["betas"]
            avgs = None
            if ema is not None:
                avgs = [ema[p] for p in ps]
                for p, e in zip(ps, avgs):
                    if e.dtype != torch.float32 or e.device != p.device or not e.is_contiguous() or e.numel() != p.numel():
                        raise hip.TrambaHipError("Adam: an average is a contiguous fp32 tensor of its parameter's size and device")
                avgs = hip.pointer_array(avgs)
            hip.adam_step_raw(plan[1], hip.pointer_array(grads), plan[2], plan[3], plan[4], plan[5], len(ps), group["lr"], b1, b2,
                              group["eps"], group["weight_decay"], gscale=gscale, skip=skip, ema=avgs, sched=sched)
            # the kernel writes through raw pointers: bump the version counters as an in-place torch op would (every
            # derived-weight cache of the inference path is keyed on them)
            torch.autograd.graph.increment_version(ps)
        return loss


def get_opt(lr, model, capturable=False):
    """train.py:266-280: two Adam groups, encoder parameters at lr/10.  `capturable`: the whole step can be replayed as a
    hipGraph (tramba_amd.graph.GraphedTrainStep).  On the GPU the update is the library's one-pass multi-tensor kernel
    (`Adam` above: the same arithmetic and state_dict as the reference's default optimizer)."""
    base = [p for n, p in model.named_parameters() if "encoder" in n]
    other = [p for n, p in model.named_parameters() if "encoder" not in n]
    groups = [{"params": base, "lr": lr * 0.1}, {"params": other, "lr": lr}]
    if len(base + other) > 0 and all(p.is_cuda and p.dtype == torch.float32 for p in base + other):
        return Adam(groups, lr, capturable=capturable)
    return torch.optim.Adam(groups, lr, capturable=capturable)


def adjust_learning_rate(optimizer, epoch, decay_epochs, base_lr, decay_factors):
    """utils/lr.py:1-17: at a listed epoch set lr = base_lr * factor (encoder group at a tenth)."""
    assert len(decay_epochs) == len(decay_factors)
    if epoch in decay_epochs:
        f = decay_factors[decay_epochs.index(epoch)]
        optimizer.param_groups[1]["lr"] = base_lr * f
        optimizer.param_groups[0]["lr"] = base_lr * f * 0.1
    return optimizer.param_groups[1]["lr"]


DEFER_SUMS = True   # (scripts/graph_train.py times the step both ways)


def _has_standing_grads(opt):
    """any parameter of the optimizer whose .grad is set (backward would accumulate into it)"""
    for g in opt.param_groups:
        for p in g["params"]:
            if p.grad is not None:
                return True
    return False


def _is_pow2(x):
    import math
    return isinstance(x, (int, float)) and math.isfinite(x) and x > 0 and math.frexp(x)[0] == 0.5


class LossScale:
    """Hyper-parameters of dynamic loss scaling (what fp16 activations need: the gradient of a mean over B*H*W pixels lies
    below fp16's range).  The gradient of the loss is multiplied by `scale`; the optimizer sees the
    gradient divided by it again.  After a step that was skipped for an Inf / NaN gradient the scale is multiplied by
    `backoff` (not below `min_scale`); after `growth_interval` steps in a row that were not, by `growth` (not above
    `max_scale`).  torch.cuda.amp.GradScaler's defaults, plus the two clamps.  Every factor is a power of two, so scaling
    and un-scaling are exact and a run with a scaler equals the run without one wherever nothing over- or underflows."""

    def __init__(self, init=65536.0, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
        for name, v in (("init", init), ("growth", growth), ("backoff", backoff), ("min_scale", min_scale), ("max_scale", max_scale)):
            if not _is_pow2(v) or not 2.0 ** -126 <= v <= 2.0 ** 126:
                raise ValueError(f"LossScale: {name} must be a power of two in 2^-126 .. 2^126 (got {v!r})")
        if not growth > 1:
            raise ValueError(f"LossScale: growth must be above 1 (got {growth!r})")
        if not backoff < 1:
            raise ValueError(f"LossScale: backoff must be below 1 (got {backoff!r})")
        if int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError(f"LossScale: growth_interval must be a positive integer (got {growth_interval!r})")
        if not min_scale <= max_scale:
            raise ValueError(f"LossScale: min_scale {min_scale!r} above max_scale {max_scale!r}")
        # (`init` may lie outside the clamps: they bound where the scale MOVES to)
        self.init, self.growth, self.backoff = float(init), float(growth), float(backoff)
        self.growth_interval, self.min_scale, self.max_scale = int(growth_interval), float(min_scale), float(max_scale)

    def key(self):
        """the host scalars a captured update bakes in"""
        return (self.growth, self.backoff, self.growth_interval, self.min_scale, self.max_scale)

    def moved(self, scale, good_steps, skipped):
        """the rule: (scale, good_steps) after a step that was / was not skipped"""
        if skipped:
            return max(self.min_scale, scale * self.backoff), 0
        good_steps += 1
        if good_steps >= self.growth_interval:
            return min(self.max_scale, scale * self.growth), 0
        return scale, good_steps

    def __repr__(self):
        return (f"LossScale(init={self.init!r}, growth={self.growth!r}, backoff={self.backoff!r}, growth_interval="
                f"{self.growth_interval!r}, min_scale={self.min_scale!r}, max_scale={self.max_scale!r})")


class LrSchedule:
    """A learning-rate schedule as an immutable table of fp64 factors indexed by optimizer step and clamped to its last
    entry: in step t every group's rate is its own `lr` times `factor(t)`.  The table is built on the host once and
    uploaded once per device; StepControl(schedule=...) keeps the index in a device record, so the groups' `lr` values
    never move and a captured step is never re-captured for them.  The index counts the steps that were ATTEMPTED: a step
    skipped for a non-finite gradient uses up its entry, and a schedule ends at the step it was planned to end at.

    Constructors (t = 0, 1, ... is the optimizer step; the ramp of `warmup` steps is (t + 1) / (warmup + 1)):
      LrSchedule(factors)                         any sequence of non-negative finite numbers
      from_callable(fn, total)                    [fn(t) for t in range(total)]
      warmup_cosine(total, warmup, floor)         floor + (1 - floor) sin^2(pi / 2 * r),  r = (total - t) / (total - warmup)
                                                  (= floor + (1 - floor) (1 + cos(pi (t - warmup) / (total - warmup))) / 2,
                                                  in the form that keeps its precision at the end), total + 1 entries: the
                                                  last one, for every step from `total` on, is `floor`
      warmup_poly(total, warmup, power, floor)    floor + (1 - floor) r^power, same r and the same last entry
      step_decay(steps_per_epoch, epochs, decay_epochs, decay_factors)
                                                  `adjust_learning_rate` as a table: the factor of the latest listed
                                                  epoch reached, 1.0 before the first; with it the decoder group's rate
                                                  is that function's base_lr * f bit for bit"""

    def __init__(self, factors):
        import math
        fs = tuple(float(f) for f in factors)
        if not fs:
            raise ValueError("LrSchedule: an empty table")
        for t, f in enumerate(fs):
            if not math.isfinite(f) or f < 0:
                raise ValueError(f"LrSchedule: factor {f!r} at step {t}: finite and not negative")
        self._factors = fs
        self._tables = {}

    def __len__(self):
        return len(self._factors)

    @property
    def factors(self):
        return self._factors

    def factor(self, t):
        """the host value of step t's factor"""
        return self._factors[min(max(int(t), 0), len(self._factors) - 1)]

    def table(self, device):
        """the fp64 table on `device` (uploaded at the first call)"""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = torch.tensor(self._factors, dtype=torch.float64).to(device)
        return self._tables[key]

    @classmethod
    def from_callable(cls, fn, total):
        if int(total) != total or total < 1:
            raise ValueError(f"LrSchedule.from_callable: total must be a positive integer (got {total!r})")
        return cls([fn(t) for t in range(int(total))])

    @staticmethod
    def _ramp(what, total, warmup, floor):
        if int(total) != total or int(warmup) != warmup or not 0 <= warmup < total:
            raise ValueError(f"LrSchedule.{what}: 0 <= warmup < total, both integers (got warmup={warmup!r}, total={total!r})")
        if not 0.0 <= floor <= 1.0:
            raise ValueError(f"LrSchedule.{what}: floor in [0, 1] (got {floor!r})")
        return int(total), int(warmup), float(floor)

    @classmethod
    def warmup_cosine(cls, total, warmup=0, floor=0.0):
        import math
        total, warmup, floor = cls._ramp("warmup_cosine", total, warmup, floor)
        fs = [(t + 1) / (warmup + 1) for t in range(warmup)]
        fs += [floor + (1.0 - floor) * math.sin(0.5 * math.pi * ((total - t) / (total - warmup))) ** 2 for t in range(warmup, total + 1)]
        return cls(fs)

    @classmethod
    def warmup_poly(cls, total, warmup=0, power=0.9, floor=0.0):
        total, warmup, floor = cls._ramp("warmup_poly", total, warmup, floor)
        if not power > 0:
            raise ValueError(f"LrSchedule.warmup_poly: power must be positive (got {power!r})")
        fs = [(t + 1) / (warmup + 1) for t in range(warmup)]
        fs += [floor + (1.0 - floor) * ((total - t) / (total - warmup)) ** float(power) for t in range(warmup, total + 1)]
        return cls(fs)

    @classmethod
    def step_decay(cls, steps_per_epoch, epochs, decay_epochs, decay_factors):
        if int(steps_per_epoch) != steps_per_epoch or steps_per_epoch < 1 or int(epochs) != epochs or epochs < 1:
            raise ValueError("LrSchedule.step_decay: steps_per_epoch and epochs are positive integers")
        decay_epochs, decay_factors = list(decay_epochs), list(decay_factors)
        if len(decay_epochs) != len(decay_factors):
            raise ValueError("LrSchedule.step_decay: one factor per listed epoch")
        fs, f = [], 1.0
        for epoch in range(int(epochs)):
            if epoch in decay_epochs:
                f = float(decay_factors[decay_epochs.index(epoch)])
            fs += [f] * int(steps_per_epoch)
        return cls(fs)

    def __repr__(self):
        return f"LrSchedule({len(self._factors)} steps, {self._factors[0]!r} .. {self._factors[-1]!r})"


class WeightEMA:
    """An exponential moving average of the weights, moved by the optimizer step itself: ema += w_t * (p - ema) after the
    parameter's update of step t, with w_t = 1 - min(decay, (1 + t) / (10 + t)) (`warmup=True`: the average follows the
    weights closely while it is young) or w_t = 1 - decay (`warmup=False`).  The weights are a table, evaluated in fp64,
    rounded to fp32 and as long as it takes to reach 1 - decay; t is the schedule index of StepControl, which counts
    attempted steps.

    Hand it to StepControl(ema=...).  It owns one tensor per optimizer parameter (fp32 on the device path; the
    parameter's dtype where torch's optimizer runs), initialised to the parameter when the control first binds.  On the
    device path the optimizer kernel moves the average in the pass that updates the parameter (36 B per parameter instead
    of 28, no further launch), and a step that is skipped for a non-finite gradient leaves the averages alone.  Only
    parameters the optimizer updates in a step have their average moved in that step: one without a gradient (frozen, or
    unused in that forward) keeps its average as it is, which is where an average of a parameter that does not move
    would stay anyway.  Buffers (BatchNorm's running statistics) are not averaged: evaluation under `applied` uses the
    live model's."""

    def __init__(self, decay=0.999, warmup=True):
        import numpy as np
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay in [0, 1) (got {decay!r})")
        self.decay, self.warmup = float(decay), bool(warmup)
        ws, t = [], 0
        while True:
            d = min(self.decay, (1 + t) / (10 + t)) if self.warmup else self.decay
            ws.append(float(np.float32(1.0 - d)))
            if d >= self.decay:
                break
            t += 1
        self._weights = tuple(ws)
        self._tables = {}
        self._avg = {}              # parameter -> its average
        self._order = []            # the parameters in optimizer order
        self._pending = None        # tensors handed to load_state_dict before the parameters were known

    @property
    def weights(self):
        return self._weights

    def weight(self, t):
        """the host value of step t's weight (an fp32 number)"""
        return self._weights[min(max(int(t), 0), len(self._weights) - 1)]

    def table(self, device):
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = torch.tensor(self._weights, dtype=torch.float32).to(device)
        return self._tables[key]

    def _bind(self, opt):
        """averages for the optimizer's parameters that have none yet, initialised to the parameter (or to what
        load_state_dict left); the tensors of known parameters stay where they are"""
        params = [p for g in opt.param_groups for p in g["params"]]
        fresh = [p for p in params if p not in self._avg]
        self._order = params
        if self._pending is not None and len(self._pending) != len(params):
            raise ValueError(f"WeightEMA.load_state_dict: {len(self._pending)} tensors for {len(params)} optimizer parameters")
        with torch.no_grad():
            for p in fresh:
                self._avg[p] = p.detach().clone(memory_format=torch.contiguous_format)
            if self._pending is not None:
                for p, t in zip(params, self._pending):
                    if t.shape != p.shape:
                        raise ValueError(f"WeightEMA.load_state_dict: a tensor of shape {tuple(t.shape)} for a parameter of {tuple(p.shape)}")
                    self._avg[p].copy_(t)
                self._pending = None
        return bool(fresh)

    def tensors(self):
        """the averages in optimizer parameter order"""
        return [self._avg[p] for p in self._order]

    def average(self, p):
        return self._avg[p]

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "tensors": [t.detach().clone() for t in self.tensors()]}

    def load_state_dict(self, sd):
        if set(sd) != {"decay", "warmup", "tensors"}:
            raise ValueError(f"WeightEMA.load_state_dict: keys {sorted(sd)}")
        tensors = list(sd["tensors"])
        if self._order:
            if len(tensors) != len(self._order):
                raise ValueError(f"WeightEMA.load_state_dict: {len(tensors)} tensors for {len(self._order)} optimizer parameters")
            with torch.no_grad():
                for p, t in zip(self._order, tensors):
                    self._avg[p].copy_(t)
        else:
            self._pending = tensors

    def _model_params(self, model):
        ps = [p for p in model.parameters() if p in self._avg]
        if not ps:
            raise RuntimeError("WeightEMA: no parameter of this model has an average yet (they are laid out by the first "
                               "step of the StepControl that holds this object)")
        return ps

    def applied(self, model):
        """`with ema.applied(model):` -- the model computes with the averaged weights inside the block.  The averages are
        put into the parameters BY CONTENT: the live values are saved, the averages copied in (an in-place torch op, so the
        version counters move and the low-precision shadows, packed stencils and every other derived-weight cache are
        rebuilt), and on exit the live bits are copied back and the caches rebuilt again.  The data pointers never
        change, so captured graphs of the training step stay valid."""
        return _EmaApplied(self, model)

    def model_state_dict(self, model):
        """model.state_dict() with every averaged parameter replaced by (a copy of) its average; buffers are the live ones"""
        sd = model.state_dict()
        for name, p in model.named_parameters():
            if p in self._avg and name in sd:
                sd[name] = self._avg[p].detach().clone().to(sd[name].dtype).view_as(sd[name])
        return sd

    def __repr__(self):
        return f"WeightEMA(decay={self.decay!r}, warmup={self.warmup!r})"


def _refresh_derived(model):
    refresh_lowp_shadows(model, getattr(model, "compute_dtype", None))
    if any(p.is_cuda for p in model.parameters()):
        refresh_dw_packs(model)


class _EmaApplied:
    def __init__(self, ema, model):
        self.ema, self.model, self.live = ema, model, None

    def __enter__(self):
        ps = self.ema._model_params(self.model)
        with torch.no_grad():
            self.live = [(p, p.detach().clone()) for p in ps]
            torch._foreach_copy_([p.detach() for p in ps], [self.ema._avg[p].to(p.dtype).view_as(p) for p in ps])
        _refresh_derived(self.model)
        return self.model

    def __exit__(self, *exc):
        with torch.no_grad():
            ps = [p for p, _ in self.live]
            torch._foreach_copy_([p.detach() for p in ps], [v for _, v in self.live])
        self.live = None
        _refresh_derived(self.model)
        return False


class StepControl:
    """What an optimisation step built from several micro-batches needs to keep between them, and between replays of a
    captured step:

      accumulate      micro-batches per optimizer step: their gradients are added in fp32, in micro-batch order, and the
                      optimizer steps once on the mean (N micro-batches accumulated == N data-parallel ranks averaged);
      clip_norm       the mean gradient is scaled by min(1, clip_norm / (norm + 1e-6)), torch's clip_grad_norm_ rule;
      skip_nonfinite  a step whose accumulated gradient holds an Inf / NaN element changes nothing (parameters, moments,
                      Adam's step counters) and is counted in `skipped_steps`;
      loss_scale      None, "dynamic" (= LossScale()) or a LossScale: the gradient of every micro-batch's loss is multiplied
                      by a scale that lives next to the record (constant over the micro-batches of a step), the optimizer
                      gets the gradient divided by it again, and the scale moves after every optimizer step by the rule
                      of `LossScale`.  Implies skip_nonfinite (a skipped step is what cuts the scale; an explicit False is
                      refused).  The returned loss and `grad_norm` stay unscaled.

    On the device (fp32 parameters, the library's `Adam`) all three are the library's kernels around a 24-byte record in
    device memory (tramba_step_ctl): tramba_grad_accumulate after each backward, tramba_grad_norm once, and the optimizer
    kernel reads the scale and the skip flag from the record -- no host decision, so the whole step replays as hipGraphs
    (tramba_amd.graph.GraphedTrainStep(control=...)).  The gradients are NOT rewritten: after a step `p.grad` is a view of
    the accumulator and holds the unscaled SUM over the micro-batches; the scale lives in the optimizer kernel.  Host
    tensors / other dtypes (the rule `get_opt` picks the optimizer by) get the same semantics from torch's own functions
    (there `p.grad` ends up as the clipped mean, as clip_grad_norm_ leaves it).

    `grad_norm` (the norm of the mean gradient before clipping) and `skipped_steps` are 0-dim tensors on the parameters'
    device, valid after the first step: log them once per epoch, reading them costs a sync.  Memory: one fp32 accumulator
    per trainable parameter (with a data-parallel reducer its flat buckets are the accumulators).

    With a loss scale the device path keeps a second 24-byte record (tramba_loss_scale): the backward starts from a 0-dim
    view of its `scale` (the loss gradient kernels read it through their `gscale` pointer), tramba_grad_norm_scaled folds
    1 / scale into the one scalar the optimizer kernel multiplies in, and tramba_loss_scale_update moves the scale behind
    the optimizer's launches -- again no host decision, so a captured step replays all of it.  After such a step `p.grad`
    holds the SCALED sum over the micro-batches (p.grad / loss_scale-at-that-step / micro-batches is the mean gradient);
    on the host path it is the unscaled clipped mean as before.  `loss_scale` and `scale_backoffs` are 0-dim tensors like
    the two above (the scale the NEXT step will use; how often it was cut); `state_dict()` / `load_state_dict()` carry
    scale, good_steps, backoffs and skipped_steps across a restart.

      schedule        None or an LrSchedule: in optimizer step t every group steps at its own `lr` times schedule.factor(t);
      ema             None or a WeightEMA: an exponential moving average of the weights, moved by the optimizer step.

    With either, the device path keeps a third 24-byte record (tramba_step_sched: the steps attempted so far, the factor
    and the EMA weight of the step under way).  The optimizer kernel reads it when it runs (tramba_adam_step_sched: the
    step size is formed from lr * factor in fp64, the average moves in the pass that updates the parameter) and
    tramba_step_sched_advance moves it to the next table entries behind the optimizer's launches and the scale's move --
    no host decision, the groups' `lr` never change, and a captured step is never captured again for the rate.  The index
    counts ATTEMPTED steps: a skipped step uses up its entry, but leaves the averages as they are.  Without either, the
    step issues the launches it always issued.  `lr_factor` (the factor the next step will use) and `sched_step` are 0-dim
    tensors like the others; `state_dict()` gains `sched_step` (only then), the averages travel in `ema.state_dict()`."""

    def __init__(self, accumulate=1, clip_norm=None, skip_nonfinite=None, loss_scale=None, schedule=None, ema=None):
        if schedule is not None and not isinstance(schedule, LrSchedule):
            raise TypeError(f"StepControl: schedule={schedule!r}: None or an LrSchedule")
        if ema is not None and not isinstance(ema, WeightEMA):
            raise TypeError(f"StepControl: ema={ema!r}: None or a WeightEMA")
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"StepControl: accumulate must be a positive integer (got {accumulate!r})")
        if clip_norm is not None and not clip_norm > 0:
            raise ValueError(f"StepControl: clip_norm must be positive or None (got {clip_norm!r})")
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError(f"StepControl: loss_scale={loss_scale!r}: None, 'dynamic' or a LossScale")
            loss_scale = LossScale()
        if loss_scale is not None and not isinstance(loss_scale, LossScale):
            raise TypeError(f"StepControl: loss_scale={loss_scale!r}: None, 'dynamic' or a LossScale")
        if loss_scale is not None and skip_nonfinite is not None and not skip_nonfinite:
            raise ValueError("StepControl: a loss scale needs skip_nonfinite (a skipped step is what cuts the scale)")
        self.accumulate = int(accumulate)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.skip_nonfinite = bool(skip_nonfinite) or loss_scale is not None
        self.scaler = loss_scale
        self.schedule, self.ema = schedule, ema
        self._sched_record = self._sched = None   # device: the tramba_step_sched and its views; host: {"step", "lr_factor"}
        self._key = None            # what the buffers below were laid out for
        self._device_path = None
        self._record = self._fields = self._flat = self._workspace = None
        self._acc = {}              # parameter -> its accumulator (a 16-byte aligned view)
        self._norm = self._skipped = None
        self._ls_record = self._ls = None   # device: the tramba_loss_scale and its views; host: {"scale", "good_steps", "backoffs"}
        # what the records start from when they are laid out (load_state_dict before the first step lands here)
        self._start = {"skipped_steps": 0}
        if loss_scale is not None:
            self._start.update(scale=loss_scale.init, good_steps=0, backoffs=0)
        if self._scheduled:
            self._start["sched_step"] = 0
        self._plans = {}
        self._used = set()          # parameters that had a gradient in a micro-batch of the step under way
        self._dirty = set()         # parameters whose accumulator holds an earlier step's sums

    # ------------------------------------------------------------------ read-outs
    @property
    def grad_norm(self):
        if self._key is None:
            raise RuntimeError("StepControl.grad_norm: no step has run yet")
        return self._fields["norm"] if self._device_path else self._norm

    @property
    def skipped_steps(self):
        if self._key is None:
            raise RuntimeError("StepControl.skipped_steps: no step has run yet")
        return self._fields["skipped_steps"] if self._device_path else self._skipped

    def _scaler_field(self, name, what):
        if self.scaler is None:
            raise RuntimeError(f"StepControl.{what}: this control has no loss scale")
        if self._key is None:
            raise RuntimeError(f"StepControl.{what}: no step has run yet")
        return self._ls[name]

    @property
    def loss_scale(self):
        """the scale the next step multiplies its loss gradient by"""
        return self._scaler_field("scale", "loss_scale")

    @property
    def scale_backoffs(self):
        """how often a skipped step has cut the scale"""
        return self._scaler_field("backoffs", "scale_backoffs")

    @property
    def _scheduled(self):
        return self.schedule is not None or self.ema is not None

    def _sched_field(self, name, what):
        if not self._scheduled:
            raise RuntimeError(f"StepControl.{what}: this control has neither a schedule nor an EMA")
        if self._key is None:
            raise RuntimeError(f"StepControl.{what}: no step has run yet")
        return self._sched[name]

    @property
    def lr_factor(self):
        """what the next step multiplies every group's lr by (a 0-dim fp64 tensor; 1.0 without a schedule)"""
        return self._sched_field("lr_factor", "lr_factor")

    @property
    def sched_step(self):
        """optimizer steps attempted so far, skipped ones included: the index the next step reads its tables at"""
        return self._sched_field("step", "sched_step")

    def state_dict(self):
        """host numbers (reading them is a sync): skipped_steps, with a loss scale its scale, good_steps, backoffs, and with
        a schedule or an EMA sched_step"""
        if self._key is None:
            return dict(self._start)
        sd = {"skipped_steps": int(self.skipped_steps)}
        if self.scaler is not None:
            sd.update(scale=float(self._ls["scale"]), good_steps=int(self._ls["good_steps"]), backoffs=int(self._ls["backoffs"]))
        if self._scheduled:
            sd["sched_step"] = int(self._sched["step"])
        return sd

    def load_state_dict(self, sd):
        want = {"skipped_steps"} | ({"scale", "good_steps", "backoffs"} if self.scaler is not None else set())
        want |= {"sched_step"} if self._scheduled else set()
        if set(sd) != want:
            raise ValueError(f"StepControl.load_state_dict: keys {sorted(sd)} for a control that keeps {sorted(want)}")
        if self.scaler is not None and not (_is_pow2(float(sd["scale"])) and 2.0 ** -126 <= sd["scale"] <= 2.0 ** 126):
            raise ValueError(f"StepControl.load_state_dict: scale {sd['scale']!r} is no power of two in 2^-126 .. 2^126")
        if self._scheduled and (int(sd["sched_step"]) != sd["sched_step"] or sd["sched_step"] < 0):
            raise ValueError(f"StepControl.load_state_dict: sched_step {sd['sched_step']!r} is no step count")
        self._start = {k: (float(v) if k == "scale" else int(v)) for k, v in sd.items()}
        if self._key is not None:
            self._fill_state()

    def _fill_state(self):
        """write self._start into the records"""
        st = self._start
        (self._fields["skipped_steps"] if self._device_path else self._skipped).fill_(st["skipped_steps"])
        if self.scaler is not None:
            self._ls["scale"].fill_(st["scale"])
            self._ls["good_steps"].fill_(st["good_steps"])
            self._ls["backoffs"].fill_(st["backoffs"])
            if self._device_path:
                self._ls["inv_scale"].fill_(1.0 / st["scale"])
        if self._scheduled:
            t = st["sched_step"]
            self._sched["step"].fill_(t)
            self._sched["lr_factor"].fill_(1.0 if self.schedule is None else self.schedule.factor(t))
            if self._device_path:
                self._sched["ema_weight"].fill_(0.0 if self.ema is None else self.ema.weight(t))

    # ------------------------------------------------------------------ buffers
    def _bind(self, opt, reducer=None):
        """lay the record, the accumulators and the norm workspace out for the trainable parameters of `opt` (again when
        that set, or the reducer's buckets, change: freeze_encoder / unfreeze_encoder)"""
        params = [p for g in opt.param_groups for p in g["params"] if p.requires_grad and p.numel() > 0]
        if not params:
            raise ValueError("StepControl: the optimizer has no trainable parameter")
        if reducer is not None:
            reducer.begin_accumulation()
        key = (tuple(id(p) for p in params), id(reducer), None if reducer is None else tuple(f.data_ptr() for f in reducer.flat))
        if self.ema is not None:
            self.ema._bind(opt)                    # (averages for parameters it has not met; the others keep theirs)
        if key == self._key:
            return self._params
        dev = params[0].device
        device_path = isinstance(opt, Adam) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
        if reducer is not None:
            self._flat = reducer.flat
            self._acc = {p: v for bucket, views in zip(reducer.buckets, reducer._views) for p, v in zip(bucket, views)}
            # (the norm is taken over the whole buckets: a bucket view no optimizer group owns would never be written)
            if len(self._acc) != len(params) or any(p not in self._acc for p in params):
                raise ValueError("StepControl: the reducer's trainable parameters and the optimizer's must be the same set")
        else:
            self._acc, offs, n = {}, [], 0
            by_kind = {}
            for p in params:
                by_kind.setdefault((p.dtype, p.device), []).append(p)
            self._flat = []
            for (dtype, device), ps in by_kind.items():
                al = max(1, 16 // torch.empty((), dtype=dtype).element_size())
                offs, n = [], 0
                for p in ps:
                    offs.append(n)
                    n += (p.numel() + al - 1) // al * al
                flat = torch.zeros(n, dtype=dtype, device=device)
                self._flat.append(flat)
                for p, off in zip(ps, offs):
                    self._acc[p] = flat[off:off + p.numel()].view_as(p)
        self._start = self.state_dict()            # (a re-layout keeps the count and the scale)
        if device_path:
            import ctypes
            self._record, self._fields = hip.step_ctl_record(dev)
            if self.scaler is not None:
                self._ls_record, self._ls = hip.loss_scale_record(dev, self._start["scale"])
            numel = (ctypes.c_int64 * len(self._flat))(*[f.numel() for f in self._flat])
            nbytes = hip.grad_norm_workspace(numel, len(self._flat))
            self._workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            if self._scheduled:
                self._sched_record, self._sched = hip.step_sched_record(dev)
        else:
            self._norm = torch.zeros((), dtype=params[0].dtype if params[0].dtype.is_floating_point else torch.float32, device=dev)
            self._skipped = torch.zeros((), dtype=torch.int64, device=dev)
            if self.scaler is not None:
                self._ls_record = None
                self._ls = {"scale": torch.zeros((), dtype=torch.float32, device=dev),
                            "good_steps": torch.zeros((), dtype=torch.int32, device=dev),
                            "backoffs": torch.zeros((), dtype=torch.int64, device=dev)}
            if self._scheduled:
                self._sched_record = None
                self._sched = {"step": torch.zeros((), dtype=torch.int64, device=dev),
                               "lr_factor": torch.ones((), dtype=torch.float64, device=dev)}
        self._device_path, self._params, self._key, self._plans = device_path, params, key, {}
        self._fill_state()
        self._dirty = set(params) if reducer is not None else set()    # own buffers start as zeros, a reducer's buckets may not
        return params

    def _tables(self, device):
        """(lr table, ema table) on the device, None where there is none: what tramba_step_sched_advance reads"""
        return (None if self.schedule is None else self.schedule.table(device),
                None if self.ema is None else self.ema.table(device))

    def _begin_step(self):
        """a step starts with no micro-batch accumulated, whatever became of the last one (a step that raised between two
        micro-batches leaves the record's counter standing, and the next store would be an add)"""
        self._used = set()
        if self._device_path:
            self._fields["micro"].zero_()

    def _state_tensors(self):
        """every tensor of this object that a step rewrites (GraphedTrainStep saves and restores them around its warm-up)"""
        ts = [self._record] if self._device_path else [self._norm, self._skipped]
        if self.scaler is not None:
            ts += [self._ls_record] if self._device_path else list(self._ls.values())
        if self._scheduled:
            ts += [self._sched_record] if self._device_path else list(self._sched.values())
        if self.ema is not None:
            ts += self.ema.tensors()
        return ts + list(self._flat)

    def _backward_seed(self, loss):
        """what the backward of a micro-batch's loss starts from: None (ones), or the loss scale -- on the device a VIEW of
        the record, so a captured backward reads the scale of the step it is replayed in"""
        if self.scaler is None:
            return None
        scale = self._ls["scale"]
        return scale if scale.dtype == loss.dtype and scale.shape == loss.shape else scale.to(loss.dtype).reshape(loss.shape)

    # ------------------------------------------------------------------ the two halves of a step
    def _accumulate(self, params, first, all_ranks):
        """fold the gradients autograd has just left in .grad into the accumulators; -> the parameters that had one"""
        have = [p for p in params if p.grad is not None]
        if self._device_path:
            import ctypes
            for p in have:
                g = p.grad
                if g.dtype != torch.float32 or g.layout != torch.strided or not g.is_contiguous() or g.numel() != p.numel():
                    raise hip.TrambaHipError("StepControl: dense contiguous fp32 gradients only")
            # a parameter without a gradient takes part with a null pointer (= zeros) when it had one in an earlier
            # micro-batch, or when other ranks may have one
            take = params if all_ranks else [p for p in params if p.grad is not None or p in self._used]
            if take:
                ids = tuple(id(p) for p in take)
                plan = self._plans.get(ids)
                if plan is None:
                    plan = self._plans[ids] = (hip.pointer_array([self._acc[p] for p in take]),
                                               (ctypes.c_int64 * len(take))(*[p.numel() for p in take]))
                grads = (ctypes.c_void_p * len(take))(*[None if p.grad is None else p.grad.data_ptr() for p in take])
                # a parameter first used in a LATER micro-batch: its accumulator still holds an older step's values
                late = [self._acc[p] for p in take if not first and p not in self._used and not all_ranks]
                if late:
                    torch._foreach_zero_(late)
                hip.grad_accumulate_raw(plan[0], grads, plan[1], len(take), self._record)
        else:
            with torch.no_grad():
                if first:
                    none = [self._acc[p] for p in params if p.grad is None]
                    if none:
                        torch._foreach_zero_(none)
                    if have:
                        torch._foreach_copy_([self._acc[p] for p in have], [p.grad for p in have])
                elif have:
                    torch._foreach_add_([self._acc[p] for p in have], [p.grad for p in have])
        self._used.update(have)
        return have

    def _finish(self, opt, params, count, reducer, all_ranks):
        """the accumulated sums become the gradients; norm, clip factor and skip decision; one optimizer step"""
        used = params if all_ranks else [p for p in params if p in self._used]
        for p in params:
            p.grad = self._acc[p] if (all_ranks or p in self._used) else None
        self._used = set()
        if reducer is not None:
            reducer.reduce_accumulated()
        if not used:
            return
        if self._device_path:
            import ctypes
            # The norm is taken over the FLAT buffers the accumulators are views of -- one aligned stream in one launch
            # instead of 673 tensors in five (the padding between the views is zero).  Accumulators of parameters that
            # had a gradient in an earlier step and none in this one hold that step's sums: zeroed first.
            now = set(used)
            stale = [self._acc[p] for p in self._dirty if p not in now]
            if stale:
                torch._foreach_zero_(stale)
            self._dirty = now
            plan = self._plans.get("norm")
            if plan is None:
                plan = self._plans["norm"] = (hip.pointer_array(self._flat),
                                              (ctypes.c_int64 * len(self._flat))(*[f.numel() for f in self._flat]))
            hip.grad_norm_raw(plan[0], plan[1], len(self._flat), 1.0 / count, self.clip_norm, self.skip_nonfinite, self._record,
                              self._workspace, ls=self._ls_record if self.scaler is not None else None)
            opt.step(gscale=self._fields["scale"], skip=self._fields["skip"], sched=self._sched_record,   # (None: unscheduled)
                     ema=None if self.ema is None else self.ema._avg)
            if self.scaler is not None:
                hip.loss_scale_update_raw(self._ls_record, self._record, *self.scaler.key())
            if self._scheduled:                     # behind the optimizer's launches and the scale's move; skipped or not
                hip.step_sched_advance_raw(self._sched_record, *self._tables(params[0].device))
            return
        with torch.no_grad():
            grads = [p.grad for p in used]
            finite = bool(torch.stack([torch.isfinite(g).all() for g in grads]).all()) if self.skip_nonfinite else True
            torch._foreach_div_(grads, float(count))
            if self.scaler is not None:                # a power of two: the unscaled mean, bit for bit
                scale, good = float(self._ls["scale"]), int(self._ls["good_steps"])
                torch._foreach_mul_(grads, 1.0 / scale)
            norm = torch.nn.utils.clip_grad_norm_(used, float("inf") if self.clip_norm is None else self.clip_norm)
            self._norm.copy_(norm)
        if self._scheduled:
            t = int(self._sched["step"])
        if finite:
            if self.schedule is None:
                opt.step()
            else:                                   # every group at its own rate times the factor of this step; between
                bases = [g["lr"] for g in opt.param_groups]     # steps the groups hold their base rates, as on the device path
                try:
                    for g, base in zip(opt.param_groups, bases):
                        g["lr"] = base * self.schedule.factor(t)
                    opt.step()
                finally:
                    for g, base in zip(opt.param_groups, bases):
                        g["lr"] = base
            if self.ema is not None:                # a skipped step leaves the averages alone
                with torch.no_grad():
                    torch._foreach_lerp_([self.ema.average(p) for p in used], [p.detach() for p in used], self.ema.weight(t))
        else:
            self._skipped += 1
        if self._scheduled:                         # skipped or not: the index counts attempted steps
            self._sched["step"].fill_(t + 1)
            self._sched["lr_factor"].fill_(1.0 if self.schedule is None else self.schedule.factor(t + 1))
        if self.scaler is not None:
            scale, good = self.scaler.moved(scale, good, not finite)
            self._ls["scale"].fill_(scale)
            self._ls["good_steps"].fill_(good)
            if not finite:
                self._ls["backoffs"] += 1


def _micro_batches(images, label, control):
    """the micro-batches of one controlled step: `images` / `label` as one tensor each (split in order into
    control.accumulate equal parts) or as sequences of equal-shaped tensors, one per micro-batch"""
    if torch.is_tensor(images) != torch.is_tensor(label):
        raise ValueError("train_step: images and label are either both tensors or both sequences of micro-batches")
    if torch.is_tensor(images):
        n = control.accumulate
        if images.shape[0] != label.shape[0] or images.shape[0] == 0 or images.shape[0] % n:
            raise ValueError(f"train_step: a batch of {images.shape[0]} images (labels: {label.shape[0]}) does not split into "
                             f"{n} equal micro-batches")
        return list(images.chunk(n)), list(label.chunk(n))
    xs, ys = list(images), list(label)
    if len(xs) != len(ys) or not 1 <= len(xs) <= control.accumulate:
        raise ValueError(f"train_step: {len(xs)} image / {len(ys)} label micro-batches for accumulate={control.accumulate}")
    if any(x.shape != xs[0].shape for x in xs) or any(y.shape != ys[0].shape for y in ys):
        raise ValueError("train_step: the micro-batches of a step have one shape")
    return xs, ys


def _controlled_micro_batch(model, opt, images, label, control, params, first, all_ranks, loss_fn=None):
    """forward, loss, backward of one micro-batch and its gradients added to the accumulators; -> the loss"""
    loss = _step_loss(loss_fn, model(images), label)
    # .grad = None on every parameter: the engine then adopts the gradient tensors as they are, which is what lets the
    # deferred partial sums stay on (see train_step) -- the adding is tramba_grad_accumulate's, not one `+=` per parameter
    for g in opt.param_groups:
        for p in g["params"]:
            p.grad = None
    seed = control._backward_seed(loss)              # the loss scale, constant over the micro-batches of a step
    if DEFER_SUMS:
        with hip.deferred_sums():
            loss.backward(gradient=seed)
    else:
        loss.backward(gradient=seed)
    control._accumulate(params, first, all_ranks)
    return loss.detach()


def _controlled_finish(model, opt, control, params, count, reducer, all_ranks, on_device):
    control._finish(opt, params, count, reducer, all_ranks)
    refresh_lowp_shadows(model, getattr(model, "compute_dtype", None))
    if on_device:
        refresh_dw_packs(model)


def _controlled_step(model, opt, images, label, reducer, control, loss_fn=None):
    xs, ys = _micro_batches(images, label, control)
    params = control._bind(opt, reducer)
    all_ranks = reducer is not None and reducer.world > 1      # another rank may hold a gradient this one does not
    control._begin_step()
    total = None
    for k, (x, y) in enumerate(zip(xs, ys)):
        loss = _controlled_micro_batch(model, opt, x, y, control, params, k == 0, all_ranks, loss_fn)
        total = loss if total is None else total + loss
    _controlled_finish(model, opt, control, params, len(xs), reducer, all_ranks, xs[0].is_cuda)
    return total / len(xs)


def train_step(model, opt, images, label, reducer=None, control=None, loss=None):
    """One optimisation step (train.py:74-89).  `reducer` (tramba_amd.parallel.GradBucketReducer)
    averages gradients across data-parallel ranks; its all-reduces overlap the backward.
    `control` (StepControl): the step is built from `control.accumulate` micro-batches -- `images` / `label` are tensors
    whose leading dimension splits into that many equal parts, or sequences of equal-shaped tensors, one per micro-batch
    (a shorter sequence is a step over what it holds).  Every micro-batch runs forward, loss and backward by itself (its own
    stochastic-depth table, its own BatchNorm statistics, as a data-parallel rank would), the gradients are added in
    micro-batch order, then -- with a reducer: one all-reduce round of the accumulated buckets -- the norm of the mean
    gradient, the clip factor and the skip decision are formed and the optimizer steps once.  Returns the mean of the
    micro-batch losses.
    `loss` (SodLoss): the loss over the deep-supervision outputs; None is `tramba_loss` (BCE + IoU, train.py:76-85)."""
    if control is not None:
        return _controlled_step(model, opt, images, label, reducer, control, loss)
    outputs = model(images)
    loss = _step_loss(loss, outputs, label)
    if reducer is not None:
        reducer.prepare()
    else:
        opt.zero_grad(set_to_none=True)
    # Deferred partial sums hand autograd gradient tensors that are FILLED at the exit of the context: safe only where the engine
    # stores them as they are -- an fp32 leaf whose .grad is None (the call sites defer for fp32 parameters only; a gradient that is
    # already set would be accumulated into, i.e. read, before the flush: gradient accumulation, zero_grad(set_to_none=False))
    if DEFER_SUMS and not _has_standing_grads(opt):
        with hip.deferred_sums():  # the parameter-gradient partial sums of the pass run as a few batched launches at the exit
            loss.backward()
    else:
        loss.backward()
    if reducer is not None:
        reducer.finish()
    opt.step()
    refresh_lowp_shadows(model, getattr(model, "compute_dtype", None))   # next forward's bf16 weights: one fused cast
    if images.is_cuda:
        refresh_dw_packs(model)                                          # ... and its packed depth-wise stencils: one launch
    return loss.detach()


# ----------------------------------------------------------------------------- checkpoints / epoch loop
# File formats and names of the reference's `fit` (train.py:212-263), so checkpoints interoperate both ways:
#   <save_model>/<method>/<method>_resume.pth           {"model": state_dict, "optimizer": state_dict, "epoch": e}
#   <save_model>/<method>/<method>_MAE_<mae>_<e+1>.pth   bare state_dict of a best-MAE epoch
def _ckpt_dir(save_model, method):
    return os.path.join(save_model, method)


def save_resume(save_model, method, model, opt, epoch, control=None):
    """train.py:254-262 (written every 5th epoch there).  A `control` with a loss scale, a schedule or an EMA adds its
    state under the extra key "step_control" (the reference's loader reads the three keys it knows and ignores the
    others), one with an EMA the averages under "ema"; without any of them the file holds the reference's three keys and
    nothing else."""
    d = _ckpt_dir(save_model, method)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"{method}_resume.pth")
    ck = {"model": model.state_dict(), "optimizer": opt.state_dict(), "epoch": epoch}
    if control is not None and (control.scaler is not None or control._scheduled):
        ck["step_control"] = control.state_dict()
    if control is not None and control.ema is not None:
        ck["ema"] = control.ema.state_dict()
    torch.save(ck, path)
    return path


def save_best(save_model, method, model, mae, epoch, ema=None):
    """train.py:250-253: `<method>_MAE_<mae>_<epoch+1>.pth` holds the bare state_dict -- with `ema` (WeightEMA) the
    averaged weights the MAE was measured with."""
    d = _ckpt_dir(save_model, method)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"{method}_MAE_{mae}_{epoch + 1}.pth")
    torch.save(model.state_dict() if ema is None else ema.model_state_dict(model), path)
    return path


def load_resume(resume, save_model, method, model, opt, map_location=None, control=None):
    """train.py:214-229.  resume=None -> 0; "last" -> the resume file (model + optimizer, continues at epoch+1);
    anything else is a state_dict path whose file name ends in `_<epoch>.pth` (continues at that number).
    `control`: a StepControl with a loss scale, a schedule or an EMA continues from the state `save_resume(..., control=)`
    wrote, when the file has one (a file written without leaves the control as it is: a fresh one starts at its `init`,
    at step 0 and with averages equal to the loaded weights)."""
    if resume is None:
        return 0
    if resume == "last":
        ck = torch.load(os.path.join(_ckpt_dir(save_model, method), f"{method}_resume.pth"), map_location=map_location)
        model.load_state_dict(ck["model"], strict=True)
        opt.load_state_dict(ck["optimizer"])
        if control is not None and (control.scaler is not None or control._scheduled) and "step_control" in ck:
            control.load_state_dict(ck["step_control"])
        if control is not None and control.ema is not None and "ema" in ck:
            control.ema.load_state_dict(ck["ema"])
        return ck["epoch"] + 1
    model.load_state_dict(torch.load(resume, map_location=map_location), strict=True)
    return int(os.path.basename(resume).split("_")[-1].split(".")[0])


def _grouped(batches, n):
    """(images, label) batches -> ([images] * n, [label] * n) groups in order; the last one may be shorter, and a batch of
    another shape (the short last batch of an epoch) starts a group of its own"""
    xs, ys = [], []
    for images, label in batches:
        if xs and (images.shape != xs[0].shape or label.shape != ys[0].shape):
            yield xs, ys
            xs, ys = [], []
        xs.append(images)
        ys.append(label)
        if len(xs) == n:
            yield xs, ys
            xs, ys = [], []
    if xs:
        yield xs, ys


def fit(model, opt, batches, epochs, base_lr, decay_epochs, decay_factors, save_model, method, start_epoch=0,
        evaluate=None, see=0, best_mae=None, reducer=None, is_main=True, log=None, graph=False, control=None, loss=None):
    """Epoch loop of train.py:212-263 around `train_step`.  `batches(epoch)` yields (images, label) device tensors;
    `evaluate(model, epoch) -> MAE` runs from epoch `see` on (train.py:237); rank 0 (`is_main`) writes the files.
    `graph=True` (single process, optimizer from `get_opt(..., capturable=True)`): every step is a hipGraph replay
    (tramba_amd.graph.GraphedTrainStep), re-captured by itself when the learning rate steps.
    `control` (StepControl): `control.accumulate` consecutive batches of `batches(epoch)` make one optimizer step; a short
    last group is a step over the batches it has, as a short last batch is a step today.  With a loss scale its state
    goes into the resume file (`save_resume(..., control=)`; hand the same control to `load_resume`).
    With `control.schedule` (LrSchedule) the rate follows the schedule per optimizer step and `adjust_learning_rate` is
    not called: `decay_epochs` / `decay_factors` must be empty or None (two rules at once are refused), the groups' `lr`
    stay as `get_opt` set them, a graphed step is never re-captured for the rate, and history's "lr" is base_lr times
    the factor of the epoch's first step (from the host table).  With `control.ema` (WeightEMA) `evaluate` runs inside
    `ema.applied(model)` and the best-MAE file holds the averaged weights.
    `loss` (SodLoss): the loss every step uses (None: `tramba_loss`)."""
    loss_fn = loss
    step_fn = train_step
    schedule = None if control is None else control.schedule
    ema = None if control is None else control.ema
    if schedule is not None and (decay_epochs or decay_factors):
        raise ValueError("fit: control.schedule sets the learning rate per step: decay_epochs / decay_factors must be empty "
                         "(LrSchedule.step_decay states the epoch rule as a schedule)")
    steps_done = control.state_dict()["sched_step"] if schedule is not None else 0   # (one read before the first step)
    if graph:
        from .graph import GraphedTrainStep
        graphed = GraphedTrainStep(model, opt, reducer=reducer, control=control, loss=loss_fn)
        step_fn = lambda m_, o_, images, label, reducer=None, **kw: graphed(images, label)  # noqa: E731
    history = []
    for epoch in range(start_epoch, epochs):
        if schedule is None:
            lr = adjust_learning_rate(opt, epoch, decay_epochs, base_lr, decay_factors)
        else:
            lr = base_lr * schedule.factor(steps_done)
        total, n = None, 0
        for images, label in (batches(epoch) if control is None else _grouped(batches(epoch), control.accumulate)):
            if control is None:
                loss = step_fn(model, opt, images, label, reducer=reducer, loss=loss_fn)
            else:
                loss = step_fn(model, opt, images, label, reducer=reducer, control=control, loss=loss_fn)
            total = loss.clone() if total is None else total + loss     # clone: a graphed step reuses its loss buffer
            n += 1
        steps_done += n
        mean_loss = float(total / max(n, 1)) if total is not None else float("nan")   # one host sync per epoch
        mae = None
        if evaluate is not None and epoch + 1 >= see:
            if ema is None:
                mae = evaluate(model, epoch)
            else:
                with ema.applied(model):
                    mae = evaluate(model, epoch)
            if is_main and (best_mae is None or mae < best_mae):
                save_best(save_model, method, model, mae, epoch, ema=ema)
        if is_main and (epoch + 1) % 5 == 0:
            save_resume(save_model, method, model, opt, epoch, control=control)
        history.append({"epoch": epoch, "lr": lr, "loss": mean_loss, "mae": mae})
        if log is not None:
            log(history[-1])
    return history
