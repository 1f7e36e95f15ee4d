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
MAX_GRAPHS = 8          # captured frame shapes a FramePredictor keeps (each holds a forward's activations)


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


def _on_device(frames, device=None):
    if frames.is_cuda:
        return frames.contiguous()
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return frames.to(device).contiguous()


def preprocess(frames, img_size=384, channels="RGB"):
    """uint8 frames (H, W, 3) / (B, H, W, 3), numpy or torch, host or device, RGB or BGR -> (B, 3, S, S) f32 on the
    device: bit for bit the `image` that `data.get_transform(S, "Test")` makes of each frame (channels in RGB order)."""
    bgr = _bgr(channels)
    x = _on_device(check_frames(frames))
    _, h, w, _ = x.shape
    return hip.frames_to_input(x, resize_table(h, w, int(img_size), x.device), int(img_size), int(img_size), bgr)


def postprocess(logits, size):
    """logits (B, 1, S, S) on the device (f32 / f16 / bf16), size (H, W) -> (B, H, W) uint8 on the device: what
    `evaluate.save_predictions` writes, uint8(sigmoid(bilinear resize to (H, W), align_corners=False) * 255)."""
    h, w = (int(v) for v in size)
    return hip.logits_to_u8(logits, h, w)


class FramePredictor:
    """`pred(frames)` -> (B, H, W) uint8 saliency maps on the device, frames as `preprocess` takes them.

    With graph=True, preprocess + forward + postprocess are captured as ONE hipGraph per (B, H, W, channels), after eager
    warm-up passes (as `GraphedForward` does), and replayed; the copy of host frames into the graph's static input happens
    before the replay, outside the graph.  Same caveats as `GraphedForward`: capture after loading the weights and build a
    new predictor (or call `reset()`) when they change; the returned maps are the graph's static buffers, valid until the
    next call with the same shape -- clone (or copy to the host) what must outlive it.  At most MAX_GRAPHS shapes are kept
    (least recently used dropped).  A capture that fails falls back to the same kernels launched eagerly (strict=True
    raises instead); graph=False always launches eagerly."""

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

    def __call__(self, frames):
        if self.model.training:
            raise RuntimeError("FramePredictor: the model was switched back to training mode")
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


def predict_folder(model, folder, save_path, img_size=384, graph=True, workers=8):
    """Device counterpart of `ImageLoader(folder)` + `evaluate.save_predictions`: every .jpg / .png / .jpeg of `folder` (or
    the one file), in the loader's order, to <save_path>/<stem>.png, byte-identical to what save_predictions writes for
    the same images.  PIL decodes (convert('RGB')) and the PNGs are written on a pool of at most 16 threads.  Frames go
    through the model one at a time, as in the reference's loop: the forward's kernel schedules depend on the batch size,
    so a batched forward would round some maps differently (tests/test_gpu_properties.py).  Returns the written paths."""
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
