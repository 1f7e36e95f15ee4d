"""hipGraph replay of an inference forward.

A Tramba-V forward is ~400 dependent launches of 5-100 us each: run eagerly, Python and the launch path cost more than
the kernels at batch 1.  `GraphedForward` captures `model(x)` once per input shape into a hipGraph
(after eager warm-up passes, which also fill the per-module scan-table / weight caches on the capturing thread) and
replays it: one launch call per image.  This is the deployment form of the reference's evaluation loops
(test_TSOD.py:53-64, train.py:116-125), which call `model(images)` at batch 1 in a Python loop.

The graph holds raw pointers to the weights and to the low-precision weight shadows: capture AFTER loading a checkpoint
and build a new `GraphedForward` (or call `reset()`) whenever the weights change (e.g. per evaluation epoch in training).
Outputs are the graph's static buffers, valid until the next call with the same input shape; clone what must outlive it.
"""
import torch


class GraphedForward:
    def __init__(self, model, warmup=2, strict=False):
        if model.training:
            raise RuntimeError("GraphedForward captures an inference forward: call model.eval() first")
        self.model = model
        self.warmup = warmup
        self.strict = strict          # True: a failed capture raises instead of falling back to eager launches
        self._graphs = {}

    def reset(self):
        self._graphs.clear()

    def _capture(self, x):
        static_in = x.clone()
        with torch.no_grad():
            for _ in range(self.warmup):
                self.model(static_in)
        torch.cuda.synchronize(x.device)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.no_grad(), torch.cuda.graph(graph):
                out = self.model(static_in)
        except Exception:
            if self.strict:
                raise
            torch.cuda.synchronize(x.device)
            return None
        return graph, static_in, out

    def __call__(self, x):
        if self.model.training:
            raise RuntimeError("GraphedForward: the model was switched back to training mode")
        if not x.is_cuda:
            raise RuntimeError("GraphedForward needs a device tensor (there is no CPU path)")
        key = (tuple(x.shape), x.dtype, x.device)
        if key not in self._graphs:
            self._graphs[key] = self._capture(x)
        entry = self._graphs[key]
        if entry is None:                              # capture unavailable: same kernels, launched eagerly
            with torch.no_grad():
                return self.model(x)
        graph, static_in, out = entry
        static_in.copy_(x, non_blocking=True)
        graph.replay()
        return out


class GraphedTrainStep:
    """One optimisation step (tramba_amd.train.train_step: forward, loss, backward, Adam, weight-shadow refresh) captured
    as ONE hipGraph and replayed per batch -- the eager step issues ~6000 launches from Python.

    Requirements: an optimizer built with `capturable=True` (`train.get_opt(lr, model, capturable=True)`: Adam's step
    counters live on the device).  With a data-parallel `reducer` (world size > 1) the bucketed RCCL all-reduces launched
    from the autograd hooks are captured with the step (RCCL's stream joins the capture through the usual event edges) and
    replayed as graph nodes: every rank must capture and replay the same sequence (same batch shapes per step), and the
    reducer must not use `find_unused` (its host read of the flag vector cannot be captured).  One graph per batch shape (a short last batch of an epoch gets its
    own).  Learning rates are baked into the captured kernels: the graphs are dropped and re-captured when
    `adjust_learning_rate` changes them.  A capture needs eager warm-up steps (optimizer state and lazy caches must exist
    before the stream is captured); parameters and optimizer state are saved before and restored after them, so every call
    -- capturing or not -- advances the optimisation by exactly one step on the batch it was given.  Stochastic depth draws
    from torch's device generator, which hipGraph capture advances per replay.  Returns the loss (a static buffer).

    With `control` (tramba_amd.train.StepControl) a call takes what `train_step(..., control=control)` takes -- tensors that
    split into `control.accumulate` micro-batches, or sequences of micro-batches -- and the whole controlled step replays
    without a host decision, as TWO graphs per micro-batch shape that share one memory pool: "micro-batch + accumulate",
    replayed for all micro-batches but the last (each copied into the static input first), and "micro-batch + accumulate
    + (all-reduce +) norm + Adam + refreshes" for the last one.  Whether a micro-batch stores or adds is decided by the
    control record's counter on the device; the clip norm and 1 / micro-batches are host scalars baked into the second
    graph like the learning rates, so they are part of its key (a short last group of an epoch gets an update graph of
    its own, the full one stays).  The warm-up steps are one-micro-batch controlled steps; the control record, the
    accumulators and `skipped_steps` are put back with the parameters afterwards.  Returns the mean micro-batch loss.
    A control with a loss scale (StepControl(loss_scale=...)) replays the same way: both graphs start their backward from
    the scale in the device record, the update graph ends with the scale's move, and the scaler's hyper-parameters are
    host scalars of that launch and so part of the update graph's key; the scaler record is put back after the warm-up
    with the rest.
    A control with a schedule or an EMA (StepControl(schedule=..., ema=...)) never re-captures for the learning rate: the
    groups' `lr` values stay where they are, the optimizer launches of the update graph read the factor (and the EMA
    weight) from the schedule record, and the graph ends with the record's move to the next table entries.  The tables'
    addresses and lengths are arguments of that launch and so part of the update graph's key; the record and the averages
    are put back after the warm-up with the rest.

    `loss` (tramba_amd.train.SodLoss; None: `tramba_loss`) is what `train_step(..., loss=loss)` takes; it is recorded into
    the graphs, so it is fixed here, at construction."""

    def __init__(self, model, opt, reducer=None, warmup=2, control=None, loss=None):
        if reducer is not None and getattr(reducer, "world", 1) > 1 and getattr(reducer, "find_unused", False):
            raise RuntimeError("GraphedTrainStep: a reducer with find_unused=True reads flags on the host every step and "
                               "cannot be captured")
        if not all(g.get("capturable", False) for g in opt.param_groups):
            raise RuntimeError("GraphedTrainStep needs an optimizer with capturable=True")
        self.model, self.opt, self.reducer, self.warmup = model, opt, reducer, warmup
        self.control = control
        self.loss = loss
        self._graphs = {}
        self._lr_key = None
        self._trainable_key = None

    def _lrs(self):
        return tuple(float(g["lr"]) for g in self.opt.param_groups)

    def _snapshot(self):
        params = [p for g in self.opt.param_groups for p in g["params"]]
        saved = []
        for p in params:
            st = self.opt.state.get(p)
            saved.append((p, p.detach().clone(),
                          None if not st else {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}))
        buffers = [(b, b.detach().clone()) for b in self.model.buffers()]         # buffers: BatchNorm running statistics
        if self.control is not None:
            buffers += [(t, t.clone()) for t in self.control._state_tensors()]
        return saved, buffers

    def _restore(self, snapshot):
        from .modules import refresh_dw_packs, refresh_lowp_shadows
        saved, buffers = snapshot
        with torch.no_grad():
            for b, value in buffers:
                b.copy_(value)
            for p, value, st in saved:
                p.copy_(value)
                for k, v in self.opt.state.get(p, {}).items():
                    if torch.is_tensor(v):               # in place: the graph holds pointers to these tensors
                        if st is not None and k in st:
                            v.copy_(st[k])
                        else:
                            v.zero_()                    # state created by the warm-up: back to "never stepped"
        refresh_lowp_shadows(self.model, getattr(self.model, "compute_dtype", None))
        if any(p.is_cuda for p in self.model.parameters()):
            refresh_dw_packs(self.model)

    def _touched(self):
        """Every tensor a replay rewrites in place behind autograd's back: parameters, optimizer state, buffers."""
        ts = [p for g in self.opt.param_groups for p in g["params"]]
        ts += [v for p in list(ts) for v in self.opt.state.get(p, {}).values() if torch.is_tensor(v)]
        ts += list(self.model.buffers())
        return ts

    def _mark_modified(self):
        """A graph replay updates the weights without bumping their version counters, and every derived-weight cache of
        the inference path (packed stencils, -exp(A_logs), fp32 views, head biases, the low-precision shadows) is keyed
        on those counters: bump them, then re-stamp the shadows the replay has just refreshed as current."""
        from .modules import restamp_lowp_shadows
        torch.autograd.graph.increment_version(self._touched())
        restamp_lowp_shadows(self.model)

    def _capture(self, images, label):
        from .train import train_step
        sx, sy = images.clone(), label.clone()
        saved = self._snapshot()
        dev = images.device
        rng = torch.cuda.get_rng_state(dev)                 # the warm-up steps draw stochastic-depth masks: undone below
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # optimizer state and all lazy caches exist before capture
            for _ in range(self.warmup):
                train_step(self.model, self.opt, sx, sy, reducer=self.reducer, loss=self.loss)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        from .modules import model_mask_pool
        pool = model_mask_pool(self.model)
        pool.forget_draw()                                  # the step's one stochastic-depth draw must be IN the graph
        graph = torch.cuda.CUDAGraph()
        # With collectives in the step, ProcessGroupNCCL's watchdog / heartbeat threads keep making runtime calls (event
        # queries on the warm-up steps' work objects) while this thread records: under the default "global" capture mode
        # any such call from ANOTHER thread invalidates the capture.  "thread_local" flags only this thread's own unsafe
        # calls -- what PyTorch documents for capturing NCCL collectives.
        mode = "thread_local" if (self.reducer is not None and getattr(self.reducer, "world", 1) > 1) else "global"
        with torch.cuda.graph(graph, capture_error_mode=mode):   # records, executes nothing
            loss = train_step(self.model, self.opt, sx, sy, reducer=self.reducer, loss=self.loss)
        keep_alive = (pool.probs, pool.buf, pool.buf32)              # the keep-probabilities the captured bernoulli / divide nodes read
        pool.forget_draw()                                  # (the table drawn during capture lives in the graph's pool)
        self._restore(saved)
        torch.cuda.set_rng_state(rng, dev)
        return graph, sx, sy, loss, keep_alive

    # ------------------------------------------------------------------ a controlled step: two graphs per shape
    def _capture_controlled(self, sx, sy, count, pool, update):
        """one micro-batch on the static inputs (+ the update of a `count`-micro-batch step) -> (graph, loss, keep_alive)"""
        from . import train
        from .modules import model_mask_pool
        control, all_ranks = self.control, self.reducer is not None and getattr(self.reducer, "world", 1) > 1
        params = control._bind(self.opt, self.reducer)
        masks = model_mask_pool(self.model)
        masks.forget_draw()
        graph = torch.cuda.CUDAGraph()
        mode = "thread_local" if all_ranks else "global"
        control._used = set()
        with torch.cuda.graph(graph, pool=pool, capture_error_mode=mode):
            # (first=True: store-or-add is the record's decision at replay, the host treats every micro-batch alike)
            loss = train._controlled_micro_batch(self.model, self.opt, sx, sy, control, params, True, all_ranks, self.loss)
            if update:
                train._controlled_finish(self.model, self.opt, control, params, count, self.reducer, all_ranks, True)
        control._used = set()
        keep_alive = (masks.probs, masks.buf, masks.buf32)
        masks.forget_draw()
        return graph, loss, keep_alive

    def _warm_controlled(self, x, y):
        """static inputs for this micro-batch shape; optimizer state, accumulators and all lazy caches exist afterwards"""
        from .train import train_step
        sx, sy = x.clone(), y.clone()
        self.control._bind(self.opt, self.reducer)
        if not self.control._device_path:
            raise RuntimeError("GraphedTrainStep(control=...): only the library's optimizer on fp32 device parameters "
                               "(train.get_opt(..., capturable=True)) can be captured: torch's functions decide the skip "
                               "of a non-finite step on the host")
        saved = self._snapshot()
        dev = x.device
        rng = torch.cuda.get_rng_state(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(self.warmup):
                train_step(self.model, self.opt, [sx], [sy], reducer=self.reducer, control=self.control, loss=self.loss)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        return sx, sy, saved, rng

    def _call_controlled(self, images, label):
        from .train import _micro_batches
        control = self.control
        xs, ys = _micro_batches(images, label, control)
        count, x0, y0 = len(xs), xs[0], ys[0]
        shape_key = (tuple(x0.shape), x0.dtype, tuple(y0.shape), y0.dtype)
        entry = self._graphs.get(shape_key)
        if entry is None:
            entry = self._graphs[shape_key] = {"static": None, "mid": None, "update": {}, "pool": torch.cuda.graph_pool_handle()}
        need_mid = count > 1 and entry["mid"] is None
        update_key = (count, control.clip_norm, control.skip_nonfinite, None if control.scaler is None else control.scaler.key())
        if control._scheduled:                      # the tables' addresses and lengths are arguments of the advance launch
            update_key += tuple(None if t is None else (t.data_ptr(), t.numel()) for t in control._tables(x0.device))
        need_update = update_key not in entry["update"]
        if need_mid or need_update:
            if entry["static"] is None:
                sx, sy, saved, rng = self._warm_controlled(x0, y0)
                entry["static"] = (sx, sy)
            else:                                   # (a further update graph for a known shape: everything is warm)
                sx, sy = entry["static"]
                saved = rng = None                  # (a capture executes nothing: there is nothing to put back)
            if need_mid:
                entry["mid"] = self._capture_controlled(sx, sy, count, entry["pool"], False)
            if need_update:
                entry["update"][update_key] = self._capture_controlled(sx, sy, count, entry["pool"], True)
            if saved is not None:
                self._restore(saved)
                torch.cuda.set_rng_state(rng, x0.device)
        sx, sy = entry["static"]
        control._begin_step()                       # (outside the graphs: one 4-byte fill per optimizer step)
        total = None
        for k, (x, y) in enumerate(zip(xs, ys)):
            graph, loss = (entry["mid"] if k < count - 1 else entry["update"][update_key])[:2]
            sx.copy_(x, non_blocking=True)
            sy.copy_(y, non_blocking=True)
            graph.replay()
            total = loss.clone() if total is None else total + loss
        self._mark_modified()
        return total / count

    def __call__(self, images, label):
        if not self.model.training:
            raise RuntimeError("GraphedTrainStep: the model is in eval mode (an evaluation callback must switch it back "
                               "with model.train() before the next step)")
        # learning rates AND the set of trainable parameters are baked into a capture (freeze_encoder / unfreeze_encoder
        # flip requires_grad: the eager step follows them, a stale graph would keep updating frozen weights)
        lrs, trainable = self._lrs(), tuple(p.requires_grad for g in self.opt.param_groups for p in g["params"])
        if lrs != self._lr_key or trainable != self._trainable_key:
            self._graphs.clear()
            self._lr_key, self._trainable_key = lrs, trainable
        if self.control is not None:
            return self._call_controlled(images, label)
        key = (tuple(images.shape), images.dtype, tuple(label.shape), label.dtype)
        entry = self._graphs.get(key)
        if entry is None:
            entry = self._graphs[key] = self._capture(images, label)
        graph, sx, sy, loss = entry[:4]
        sx.copy_(images, non_blocking=True)
        sy.copy_(label, non_blocking=True)
        graph.replay()
        self._mark_modified()
        return loss
