"""Deployment pipeline: uint8 camera frames in, uint8 saliency maps at each frame's own size out, all on the device.

The reference's inference path (test_TSOD.py:46-68 with data/dataloader.py:91-127) resizes and normalises every image on
the host (PIL bilinear resize, numpy normalisation), runs the model, and resizes the logits back to the image's size before
sigmoid, *255 and the cast to uint8.  Here both ends are HIP kernels (csrc/frames.hip):

  preprocess   (B, H, W, 3) u8 frames -> (B, 3, S, S) f32 model input, bit for bit `data.get_transform(S, "Test")`'s image
               (tramba_frames_to_input; the PIL fixed-point weights and the normalisation table are built by the library
               on the host, uploaded once per (frame size, S) and cached);
  postprocess  (B, 1, S, S) logits -> (B, H, W) u8, what `evaluate.save_predictions` computes per image
               (tramba_logits_to_u8).

`FramePredictor` chains preprocess, forward and postprocess and replays the chain as ONE hipGraph per input shape;
`predict_folder` is the device counterpart of `ImageLoader` + `save_predictions` and writes the same PNG bytes.

A LIST of frames is a batch of frames of different sizes (a dataset folder).  `pack_frames` puts it into one packed uint8
buffer led by per-frame descriptors (sizes, byte offsets, the coefficient tables themselves), which goes up in one copy;
tramba_frames_to_input_ragged / tramba_logits_to_u8_ragged read the sizes from those descriptors, so their launches do not
depend on them and `FramePredictor` needs ONE hipGraph per (batch size, capacity bucket) for every mix of sizes.  Each
frame's input plane and map are bit for bit what the uniform kernels give for that frame alone.
"""
import os
import warnings
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import data, hip

_BGR = {"RGB": False, "BGR": True}
_tables = {}
MAX_GRAPHS = 8          # captured graphs a FramePredictor keeps, per-shape and ragged together (each holds a forward's activations)
MAX_HOST_TABLES = 256   # host coefficient tables kept for pack_frames (a dataset has hundreds of sizes; <= 70 KB each at S = 384)
MIN_BUCKET = 1 << 16    # the smallest capacity of a ragged graph's packed input / output buffer, in bytes
# descriptor words of a packed batch (include/tramba_hip.h)
_R_FRAME, _R_H, _R_W, _R_TABLE, _R_KX, _R_KY, _R_OUT, _R_RH, _R_RW = range(9)
_ALIGN = 16
_host_tables = OrderedDict()


def _bgr(channels):
    try:
        return _BGR[channels.upper()]
    except (AttributeError, KeyError):
        raise ValueError(f"channels must be 'RGB' or 'BGR', got {channels!r}") from None


def check_frames(frames):
    """frames: uint8 (H, W, 3) or (B, H, W, 3), numpy or torch, host or device -> a (B, H, W, 3) uint8 tensor (not moved).
    Raises TypeError for another dtype and ValueError for another layout or a side beyond hip.FRAME_MAX_DIM."""
    if isinstance(frames, np.ndarray):
        if frames.dtype != np.uint8:
            raise TypeError(f"frames must be uint8, got {frames.dtype}")
        with warnings.catch_warnings():        # a decoded PIL image is a read-only array; nothing here writes to it
            warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
            frames = torch.from_numpy(np.ascontiguousarray(frames))
    elif not torch.is_tensor(frames):
        raise TypeError(f"frames must be a numpy array or a tensor, got {type(frames).__name__}")
    elif frames.dtype != torch.uint8:
        raise TypeError(f"frames must be uint8, got {frames.dtype}")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be (H, W, 3) or (B, H, W, 3), got {tuple(frames.shape)}")
    b, h, w, _ = frames.shape
    if not (b >= 1 and 1 <= h <= hip.FRAME_MAX_DIM and 1 <= w <= hip.FRAME_MAX_DIM):
        raise ValueError(f"frames {tuple(frames.shape)}: each side must be 1 .. {hip.FRAME_MAX_DIM}")
    return frames


def resize_table(h, w, img_size, device):
    """device copy of the library's coefficient table for (h, w) -> (img_size, img_size), cached per device"""
    key = (h, w, img_size, str(device))
    t = _tables.get(key)
    if t is None:
        host = hip.resize_table_host(h, w, img_size, img_size, data.IMAGENET_MEAN, data.IMAGENET_STD)
        t = torch.from_numpy(host).to(device)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(device).synchronize()     # the table is shared by every stream from here on
        _tables[key] = t
    return t


# ----------------------------------------------------------------------------- packed batches of mixed sizes
def check_frame_list(frames):
    """a non-empty list / tuple of uint8 (H_i, W_i, 3) frames, numpy or torch, in host memory -> a list of contiguous
    numpy arrays.  TypeError for another container, element type or dtype, ValueError for an empty list, another layout, a
    device tensor or a side beyond hip.FRAME_MAX_DIM."""
    if not isinstance(frames, (list, tuple)):
        raise TypeError(f"a batch of mixed-size frames must be a list or a tuple, got {type(frames).__name__}")
    if not 1 <= len(frames) <= 65535:
        raise ValueError(f"a batch of mixed-size frames holds 1 .. 65535 frames, got {len(frames)}")
    out = []
    for i, f in enumerate(frames):
        if torch.is_tensor(f):
            if f.is_cuda:
                raise ValueError(f"frame {i}: a mixed-size batch is packed on the host, got a device tensor")
            if f.dtype != torch.uint8:
                raise TypeError(f"frame {i} must be uint8, got {f.dtype}")
            f = f.contiguous().numpy()
        elif not isinstance(f, np.ndarray):
            raise TypeError(f"frame {i} must be a numpy array or a tensor, got {type(f).__name__}")
        elif f.dtype != np.uint8:
            raise TypeError(f"frame {i} must be uint8, got {f.dtype}")
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"frame {i} must be (H, W, 3), got {tuple(f.shape)}")
        if not (1 <= f.shape[0] <= hip.FRAME_MAX_DIM and 1 <= f.shape[1] <= hip.FRAME_MAX_DIM):
            raise ValueError(f"frame {i} {tuple(f.shape)}: each side must be 1 .. {hip.FRAME_MAX_DIM}")
        out.append(np.ascontiguousarray(f))
    return out


def _host_table(h, w, img_size):
    """the library's coefficient table for (h, w) -> (img_size, img_size) as host bytes, least recently used dropped"""
    key = (h, w, img_size)
    t = _host_tables.get(key)
    if t is None:
        t = hip.resize_table_host(h, w, img_size, img_size, data.IMAGENET_MEAN, data.IMAGENET_STD).view(np.uint8)
        _host_tables[key] = t
        while len(_host_tables) > MAX_HOST_TABLES:
            _host_tables.popitem(last=False)
    else:
        _host_tables.move_to_end(key)
    return t


def _taps(n, img_size):
    """taps per output sample of one axis, as the library's tables have them (csrc/frames.hip resample_taps)"""
    return 1 if n == img_size else int(np.ceil(max(n / img_size, 1.0))) * 2 + 1


def _up(n):
    return -(-n // _ALIGN) * _ALIGN


def size_descriptors(sizes, img_size):
    """[(h, w)] -> (B, hip.FRAMES_DESC_WORDS) int64 descriptors with the words of the output side filled: h, w, the map's
    byte offset (16-byte aligned, in order) and the fp32 bits of img_size / h and img_size / w (fp32 division, as the
    uniform entry computes torch's scale)."""
    desc = np.zeros((len(sizes), hip.FRAMES_DESC_WORDS), dtype=np.int64)
    at = 0
    s = np.float32(img_size)
    for d, (h, w) in zip(desc, sizes):
        h, w = int(h), int(w)
        d[_R_H], d[_R_W], d[_R_OUT] = h, w, at
        d[_R_RH] = int((s / np.float32(h)).view(np.uint32)) if h > 0 else 0
        d[_R_RW] = int((s / np.float32(w)).view(np.uint32)) if w > 0 else 0
        at = _up(at + max(h, 0) * max(w, 0))
    return desc


def pack_frames(frames, img_size=384, pin=None):
    """frames: a list / tuple of uint8 (H_i, W_i, 3) arrays (numpy or torch, host) -> {"packed": (N,) u8 host tensor,
    "batch": B, "img_size": S}.  The buffer holds B descriptors of hip.FRAMES_DESC_WORDS int64 words (`descriptors`), then
    the coefficient table of every distinct frame size, then the frames, each at a 16-byte aligned offset.  pin: page-lock
    the buffer (default: when a HIP device is present and this is not a DataLoader worker, whose batches the loader pins)."""
    frames = check_frame_list(frames)
    img_size = int(img_size)
    desc = size_descriptors([f.shape[:2] for f in frames], img_size)
    at = desc.nbytes
    tables = {}
    for d, f in zip(desc, frames):
        h, w = f.shape[:2]
        if (h, w) not in tables:
            t = _host_table(h, w, img_size)
            tables[(h, w)] = (at, t)
            at = _up(at + t.nbytes)
        d[_R_TABLE], d[_R_KX], d[_R_KY] = tables[(h, w)][0], _taps(w, img_size), _taps(h, img_size)
    for d, f in zip(desc, frames):
        d[_R_FRAME] = at
        at = _up(at + f.size)
    if pin is None:
        pin = torch.cuda.is_available() and torch.utils.data.get_worker_info() is None
    buf = torch.empty(at, dtype=torch.uint8, pin_memory=bool(pin))
    flat = buf.numpy()
    flat[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    for o, t in tables.values():
        flat[o:o + t.nbytes] = t
    for d, f in zip(desc, frames):
        flat[d[_R_FRAME]:d[_R_FRAME] + f.size] = f.reshape(-1)
    return {"packed": buf, "batch": len(frames), "img_size": img_size}


class PackFrames:
    """DataLoader collate_fn over a dataset of uint8 frames (runs in the worker): `pack_frames` at one model input size."""

    def __init__(self, img_size=384):
        self.img_size = img_size

    def __call__(self, frames):
        return pack_frames(frames, self.img_size)


def descriptors(batch):
    """the (B, hip.FRAMES_DESC_WORDS) int64 view of a packed batch's descriptors (host memory)"""
    b = batch["batch"]
    return batch["packed"][:b * hip.FRAMES_DESC_WORDS * 8].numpy().view(np.int64).reshape(b, hip.FRAMES_DESC_WORDS)


def frame_sizes(desc):
    return [(int(d[_R_H]), int(d[_R_W])) for d in desc]


def output_bytes(desc):
    """bytes of the output buffer a batch needs: the end of its last map, rounded up to 16"""
    return _up(int(desc[-1, _R_OUT] + desc[-1, _R_H] * desc[-1, _R_W]))


def capacity_bucket(nbytes):
    """the capacity of the graph buffer that takes `nbytes`: the smallest power of two that holds them, at least MIN_BUCKET"""
    nbytes = int(nbytes)
    if nbytes < 1:
        raise ValueError(f"capacity_bucket: {nbytes} bytes")
    return max(MIN_BUCKET, 1 << (nbytes - 1).bit_length())


def _map_views(out, desc):
    return [out[int(d[_R_OUT]):int(d[_R_OUT] + d[_R_H] * d[_R_W])].view(int(d[_R_H]), int(d[_R_W])) for d in desc]


def _current_device():
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------------- the two ends
def _on_device(frames, device=None):
    if frames.is_cuda:
        return frames.contiguous()
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return frames.to(device).contiguous()


def preprocess(frames, img_size=384, channels="RGB"):
    """uint8 frames (H, W, 3) / (B, H, W, 3), numpy or torch, host or device, RGB or BGR -> (B, 3, S, S) f32 on the
    device: bit for bit the `image` that `data.get_transform(S, "Test")` makes of each frame (channels in RGB order).
    A list / tuple of (H_i, W_i, 3) host frames of any sizes goes through `pack_frames` and one ragged launch; row i is
    `preprocess(frames[i])`."""
    bgr = _bgr(channels)
    if isinstance(frames, (list, tuple)):
        batch = pack_frames(frames, img_size)
        packed = batch["packed"].to(_current_device(), non_blocking=True)
        return hip.frames_to_input_ragged(packed, descriptors(batch), int(img_size), bgr)
    x = _on_device(check_frames(frames))
    _, h, w, _ = x.shape
    return hip.frames_to_input(x, resize_table(h, w, int(img_size), x.device), int(img_size), int(img_size), bgr)


def postprocess(logits, size):
    """logits (B, 1, S, S) on the device (f32 / f16 / bf16), size (H, W) -> (B, H, W) uint8 on the device: what
    `evaluate.save_predictions` writes, uint8(sigmoid(bilinear resize to (H, W), align_corners=False) * 255).
    size a sequence of B sizes [(H_i, W_i)] (logits square): a list of B (H_i, W_i) uint8 views into ONE device buffer,
    map i = `postprocess(logits[i:i+1], size[i])[0]`."""
    if np.ndim(size) == 2:
        sizes = [(int(h), int(w)) for h, w in size]
        if logits.dim() != 4 or len(sizes) != logits.shape[0]:
            raise ValueError(f"postprocess: {len(sizes)} sizes for logits {tuple(logits.shape)}")
        desc = size_descriptors(sizes, logits.shape[-1])
        hip.frames_ragged_check(desc, logits.shape[-1], 0, output_bytes(desc), hip.RAGGED_OUT)    # before any allocation
        head = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(logits.device)
        out = torch.empty(output_bytes(desc), dtype=torch.uint8, device=logits.device)
        return _map_views(hip.logits_to_u8_ragged(logits, head, desc, out), desc)
    h, w = (int(v) for v in size)
    return hip.logits_to_u8(logits, h, w)


class FramePredictor:
    """`pred(frames)` -> (B, H, W) uint8 saliency maps on the device, frames as `preprocess` takes them; for a list of
    frames of different sizes, a list of (H_i, W_i) uint8 maps on the device (views into one buffer).

    With graph=True, preprocess + forward + postprocess are captured as ONE hipGraph per (B, H, W, channels), after eager
    warm-up passes (as `GraphedForward` does), and replayed; the copy of host frames into the graph's static input happens
    before the replay, outside the graph.  Same caveats as `GraphedForward`: capture after loading the weights and build a
    new predictor (or call `reset()`) when they change; the returned maps are the graph's static buffers, valid until the
    next call with the same shape -- clone (or copy to the host) what must outlive it.  At most MAX_GRAPHS shapes are kept
    (least recently used dropped).  A capture that fails falls back to the same kernels launched eagerly (strict=True
    raises instead); graph=False always launches eagerly.

    A list of frames needs ONE graph per (B, input capacity, output capacity, channels) whatever the sizes in it: the graph
    holds a packed input buffer and an output buffer whose capacities are `capacity_bucket` of the first batch's byte
    counts; a later batch of B frames replays the smallest kept graph it fits into, and one that fits none captures the
    next bucket.  The packed batch is checked (hip.frames_ragged_check) and uploaded with one non_blocking copy from pinned
    memory before the replay, outside the graph.  These graphs share the MAX_GRAPHS bound with the per-shape ones, and the
    returned maps are valid until the next call that replays the same graph."""

    def __init__(self, model, img_size=384, channels="RGB", graph=True, warmup=2, strict=False):
        if model.training:
            raise RuntimeError("FramePredictor runs an inference forward: call model.eval() first")
        params = list(model.parameters())
        if not params or not all(p.is_cuda for p in params):
            raise RuntimeError("FramePredictor needs the model's parameters on a HIP device (there is no CPU path)")
        self.model = model
        self.device = params[0].device
        self.img_size = int(img_size)
        _bgr(channels)                                   # raises on anything but RGB / BGR
        self.channels = channels.upper()
        self.graph = graph
        self.warmup = warmup
        self.strict = strict
        self._graphs = OrderedDict()

    def reset(self):
        self._graphs.clear()

    def _run(self, x):
        inp = preprocess(x, self.img_size, self.channels)
        out = self.model(inp)
        if isinstance(out, (list, tuple)):
            out = out[-1]
        return postprocess(out, x.shape[1:3])

    def _capture(self, x):
        static_in = x.clone()
        with torch.no_grad():
            for _ in range(self.warmup):        # also uploads the coefficient table and fills the model's caches
                self._run(static_in)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.no_grad(), torch.cuda.graph(graph):
                out = self._run(static_in)
        except Exception:
            if self.strict:
                raise
            torch.cuda.synchronize(self.device)
            return None
        return graph, static_in, out

    def _run_ragged(self, packed, desc, out):
        inp = hip.frames_to_input_ragged(packed, desc, self.img_size, _bgr(self.channels))
        res = self.model(inp)
        if isinstance(res, (list, tuple)):
            res = res[-1]
        return hip.logits_to_u8_ragged(res, packed, desc, out)

    def _eager_ragged(self, batch, desc):
        with torch.no_grad(), torch.cuda.device(self.device):
            packed = batch["packed"].to(self.device, non_blocking=True)
            out = torch.empty(output_bytes(desc), dtype=torch.uint8, device=self.device)
            return _map_views(self._run_ragged(packed, desc, out), desc)

    def _capture_ragged(self, batch, desc, cap_in, cap_out):
        n = batch["packed"].numel()
        static_in = torch.empty(cap_in, dtype=torch.uint8, device=self.device)
        static_out = torch.empty(cap_out, dtype=torch.uint8, device=self.device)
        static_in[:n].copy_(batch["packed"])
        with torch.no_grad():
            for _ in range(self.warmup):
                self._run_ragged(static_in, desc, static_out)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.no_grad(), torch.cuda.graph(graph):
                self._run_ragged(static_in, desc, static_out)
        except Exception:
            if self.strict:
                raise
            torch.cuda.synchronize(self.device)
            return None
        return graph, static_in, static_out

    def _call_ragged(self, frames):
        batch = pack_frames(frames, self.img_size)
        desc = descriptors(batch)
        if not self.graph:
            return self._eager_ragged(batch, desc)
        b, n, need = batch["batch"], batch["packed"].numel(), output_bytes(desc)
        fits = [k for k in self._graphs if k[0] == "ragged" and k[1] == b and k[4] == self.channels and k[2] >= n and k[3] >= need]
        if fits:
            key = min(fits, key=lambda k: (k[2], k[3]))
            self._graphs.move_to_end(key)
        else:
            key = ("ragged", b, capacity_bucket(n), capacity_bucket(need), self.channels)
            with torch.cuda.device(self.device):
                self._graphs[key] = self._capture_ragged(batch, desc, key[2], key[3])
            while len(self._graphs) > MAX_GRAPHS:
                self._graphs.popitem(last=False)
        entry = self._graphs[key]
        if entry is None:                                # capture unavailable: same kernels, launched eagerly
            return self._eager_ragged(batch, desc)
        graph, static_in, static_out = entry
        hip.frames_ragged_check(desc, self.img_size, n, static_out.numel())   # no library entry runs in a replay
        static_in[:n].copy_(batch["packed"], non_blocking=True)
        graph.replay()
        return _map_views(static_out, desc)

    def __call__(self, frames):
        if self.model.training:
            raise RuntimeError("FramePredictor: the model was switched back to training mode")
        if isinstance(frames, (list, tuple)):
            return self._call_ragged(frames)
        x = check_frames(frames)
        if not self.graph:
            with torch.no_grad(), torch.cuda.device(self.device):
                return self._run(_on_device(x, self.device))
        key = (tuple(x.shape), self.channels)
        if key in self._graphs:
            self._graphs.move_to_end(key)
        else:
            with torch.cuda.device(self.device):
                self._graphs[key] = self._capture(_on_device(x, self.device))
            while len(self._graphs) > MAX_GRAPHS:
                self._graphs.popitem(last=False)
        entry = self._graphs[key]
        if entry is None:                                # capture unavailable: same kernels, launched eagerly
            with torch.no_grad(), torch.cuda.device(self.device):
                return self._run(_on_device(x, self.device))
        graph, static_in, out = entry
        static_in.copy_(x, non_blocking=x.is_cuda or x.is_pinned())
        graph.replay()
        return out


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def folder_groups(paths, batch):
    """consecutive groups of `batch` paths in the order given (the loader's); the last group may be shorter"""
    if not isinstance(batch, (int, np.integer)) or isinstance(batch, bool) or not 1 <= batch <= 65535:
        raise ValueError(f"batch must be an integer in 1 .. 65535, got {batch!r}")
    return [list(paths[i:i + batch]) for i in range(0, len(paths), batch)]


def predict_folder(model, folder, save_path, img_size=384, graph=True, workers=8, batch=1):
    """Device counterpart of `ImageLoader(folder)` + `evaluate.save_predictions`: every .jpg / .png / .jpeg of `folder` (or
    the one file), in the loader's order, to <save_path>/<stem>.png, byte-identical to what save_predictions writes for
    the same images.  PIL decodes (convert('RGB')) and the PNGs are written on a pool of at most 16 threads.  With batch=1
    frames go through the model one at a time, as in the reference's loop.  With batch=N consecutive groups of N files
    (`folder_groups`; the last may be shorter) go through the mixed-size path of `FramePredictor` as one forward each,
    whatever their sizes; the PNG bytes then equal what save_predictions writes when it is given the same images grouped
    into the same batches in the same order.  batch=N and batch=1 outputs may differ in a few bytes: the forward's kernel
    schedules depend on the batch size, so a batched forward rounds some maps differently
    (tests/test_gpu_properties.py::test_full_forward_is_batch_independent_and_deterministic).  Returns the written paths."""
    folder_groups([], batch)                      # refuses a bad batch before anything is read
    if os.path.isdir(folder):
        paths = data._listing(folder, (".jpg", ".png", ".jpeg"))
    elif os.path.isfile(folder):
        paths = [folder]
    else:
        raise FileNotFoundError(folder)
    os.makedirs(save_path, exist_ok=True)
    from .evaluate import write_png_gray8
    pred = FramePredictor(model, img_size, "RGB", graph=graph)
    workers = max(1, min(16, int(workers)))
    written, pending = [], []
    if batch > 1:
        def use(path, m, _):
            out = os.path.join(save_path, data._stem(path) + ".png")
            pending.append(pool.submit(write_png_gray8, out, m.cpu().numpy()))     # a copy: the graph's buffer is reused
            written.append(out)
            while len(pending) > 2 * workers + batch:
                pending.pop(0).result()

        with ThreadPoolExecutor(max_workers=workers) as pool:
            _predict_groups(pred, paths, batch, pool, workers, lambda p: (_read_rgb(p), None), use)
            for f in pending:
                f.result()
        return written
    with ThreadPoolExecutor(max_workers=workers) as pool:
        ahead = [pool.submit(_read_rgb, p) for p in paths[:2 * workers]]      # bounded read-ahead, in order
        for i, path in enumerate(paths):
            frame = ahead[i].result()
            ahead[i] = None
            if i + 2 * workers < len(paths):
                ahead.append(pool.submit(_read_rgb, paths[i + 2 * workers]))
            m = pred(frame)[0].cpu().numpy()                 # a copy: the graph's output buffer is reused
            out = os.path.join(save_path, data._stem(path) + ".png")
            pending.append(pool.submit(write_png_gray8, out, m))
            written.append(out)
            while len(pending) > 2 * workers:               # bounded write-behind
                pending.pop(0).result()
        for f in pending:
            f.result()
    return written


def _predict_groups(pred, paths, batch, pool, workers, read, use):
    """the batched folder loop: decode with bounded read-ahead on `pool` (`read(path)` -> (frame, extra)), run the ragged
    predictor per group of `batch` paths, and hand `use(path, map on the device, extra)` every map in order"""
    ahead = [pool.submit(read, p) for p in paths[:2 * workers + batch]]
    for group in folder_groups(range(len(paths)), batch):
        got = []
        for i in group:
            got.append(ahead[i].result())
            ahead[i] = None
            if i + 2 * workers + batch < len(paths):
                ahead.append(pool.submit(read, paths[i + 2 * workers + batch]))
        for i, m, (_, extra) in zip(group, pred([f for f, _ in got]), got):
            use(paths[i], m, extra)
