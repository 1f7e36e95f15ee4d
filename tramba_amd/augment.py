"""Training augmentation on the device: uint8 image / mask pairs in, train batches out.

`data.train_loader` runs the train transform (`data.get_transform(S, "train")`: static resize, scale-crop, mirror,
rotation, enhancers, to_tensors) in PIL and numpy inside the DataLoader workers.  Here the workers only decode the pair and
make the transform's numpy draws (`DrawRecorder`, in exactly `data.Augment`'s order, touching no pixels); `collate` packs a
batch of pairs of any sizes into ONE uint8 buffer led by per-sample descriptors, which is uploaded with one asynchronous
copy, and `transform` runs the whole chain as four HIP launches (csrc/augment.hip) on tables the library builds on the
host and this module caches per device.  The batches are `torch.equal` to `data.device_batches(data.train_loader(...))`
under the same numpy and torch seeds.

    batches = device_train_batches(root, img_size=384, batch_size=8)   # what train.fit consumes
"""
import numpy as np
import torch
from PIL import Image, ImageEnhance

from . import data, hip

# descriptor words (csrc/augment.hip)
_D_IMG, _D_MASK, _D_H, _D_W, _D_SRC, _D_R, _D_OFF, _D_SCALE, _D_TAPS, _D_MIRROR, _D_ROT, _D_COEF = range(12)
_D_ENH, _D_OP, _D_FAC, _D_DEG = 17, 18, 21, 24
_ENH_CODE = {ImageEnhance.Contrast: hip.AUG_CONTRAST, ImageEnhance.Brightness: hip.AUG_BRIGHTNESS,
             ImageEnhance.Sharpness: hip.AUG_SHARPNESS}
_ALIGN = 16


class DrawRecorder(data.Augment):
    """`data.Augment`'s draws without its pixels: the same numpy calls in the same order (the scale drawn even when it is
    not applied, the vertical flip drawn and discarded, randint then random for the rotation, the enhancer list shuffled in
    place and carried from sample to sample).  Calling it with the output side S returns the sample's record:
    {"scale": R = int(round(S f)) or 0, "mirror": bool, "degrees": angle in [0, 360) or None, "enhance": [(code, factor)]}."""

    def __call__(self, size):
        return super().__call__({"size": size, "scale": 0, "mirror": False, "degrees": None, "enhance": []})

    def _scale_crop(self, s):
        factor = self.rng.random() * (self.scale[1] - self.scale[0]) + self.scale[0]
        if self.rng.random() < 0.5:
            s["scale"] = int(np.round(s["size"] * factor))

    def _flip(self, s):
        s["mirror"] = bool(self.rng.random() < 0.5)
        self.rng.random()

    def _rotate(self, s):
        deg = int(self.rng.randint(self.degrees[0], self.degrees[1]))
        if deg < 0:
            deg += 360
        if self.rng.random() < 0.5:
            s["degrees"] = deg

    def _enhance(self, s):
        self.rng.shuffle(self.enhancers)
        for make in self.enhancers:
            if self.rng.random() > 0.5:
                s["enhance"].append((_ENH_CODE[make], float(1 + self.rng.random() / 10)))


class PairDataset(data.RGB_Dataset):
    """`data.RGB_Dataset`'s pairs, decoded as there (convert("RGB") / convert("L")), returned as uint8 arrays with the
    draws of the train transform: (image (h, w, 3), mask (h, w), record)."""

    def __init__(self, root, sets, img_size, rng=None):
        super().__init__(root, sets, img_size, "train", rng)
        self.img_size = img_size
        self.recorder = DrawRecorder(rng)

    def __getitem__(self, index):
        image = np.asarray(Image.open(self.images[index]).convert("RGB"))
        gt = np.asarray(Image.open(self.gts[index]).convert("L"))
        return image, gt, self.recorder(self.img_size)


def _record_words(d, rec, size):
    r = rec["scale"]
    if r and r != size:                       # R == S is Pillow's copy
        d[_D_R], d[_D_OFF] = r, (r - size) // 2
    d[_D_MIRROR] = int(rec["mirror"])
    deg = rec["degrees"]
    if deg is not None:
        d[_D_DEG] = deg
        d[_D_ROT] = int(deg != 0)             # 0 degrees: Image.rotate copies
    d[_D_ENH] = len(rec["enhance"])
    for e, (code, factor) in enumerate(rec["enhance"]):
        d[_D_OP + e] = code
        d[_D_FAC + e] = int(np.float32(factor).view(np.uint32))


def pack(samples, size):
    """[(image (h, w, 3) u8, mask (h, w) u8, record)] -> {"packed": (N,) u8 tensor, "batch": B}: B descriptors of
    hip.AUG_DESC_WORDS int64 words, then each image and mask.  The device table addresses are filled by `bind`."""
    b = len(samples)
    at = b * hip.AUG_DESC_WORDS * 8
    spans = []
    for image, gt, _ in samples:
        h, w = gt.shape
        if image.shape != (h, w, 3) or image.dtype != np.uint8 or gt.dtype != np.uint8:
            raise ValueError(f"pack: image {image.shape} {image.dtype} does not go with mask {gt.shape} {gt.dtype}")
        spans.append((at, at + h * w * 3))
        at = -(-(at + h * w * 4) // _ALIGN) * _ALIGN
    buf = torch.empty(at, dtype=torch.uint8)
    flat = buf.numpy()
    desc = np.zeros((b, hip.AUG_DESC_WORDS), dtype=np.int64)
    for d, (image, gt, rec), (oi, om) in zip(desc, samples, spans):
        h, w = gt.shape
        flat[oi:om] = np.ascontiguousarray(image).reshape(-1)
        flat[om:om + h * w] = np.ascontiguousarray(gt).reshape(-1)
        d[_D_IMG], d[_D_MASK], d[_D_H], d[_D_W] = oi, om, h, w
        _record_words(d, rec, size)
    flat[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    return {"packed": buf, "batch": b}


class Collate:
    """DataLoader collate_fn of `PairDataset` (runs in the worker): `pack` at the dataset's output side."""

    def __init__(self, size):
        self.size = size

    def __call__(self, samples):
        return pack(samples, self.size)


_source, _size, _rot, _workspace = {}, {}, {}, {}


def _upload(host, device):
    t = torch.from_numpy(host).to(device)
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).synchronize()     # the table is shared by every stream from here on
    return t


def source_table(h, w, size, device):
    key = (h, w, size, str(device))
    if key not in _source:
        _source[key] = _upload(hip.augment_source_table_host(h, w, size), device)
    return _source[key]


def size_table(size, device):
    """(device table, host table) of one output side, cached per device"""
    key = (size, str(device))
    if key not in _size:
        host = hip.augment_size_table_host(size, data.IMAGENET_MEAN, data.IMAGENET_STD)
        _size[key] = (_upload(host, device), host)
    return _size[key]


def _rotation(size, deg):
    key = (size, deg)
    if key not in _rot:
        _rot[key] = hip.augment_rotation(size, deg)
    return _rot[key]


def descriptors(batch):
    """the (B, AUG_DESC_WORDS) int64 view of a packed batch's descriptors (host memory, writable)"""
    b = batch["batch"]
    return batch["packed"][:b * hip.AUG_DESC_WORDS * 8].numpy().view(np.int64).reshape(b, hip.AUG_DESC_WORDS)


def bind(desc, size, device):
    """write the device addresses of the tables each sample needs (and its rotation words) into its descriptor"""
    dev_st, host_st = size_table(size, device)
    lo = int(host_st[1040])
    for d in desc:
        d[_D_SRC] = source_table(int(d[_D_H]), int(d[_D_W]), size, device).data_ptr()
        r = int(d[_D_R])
        if r:
            d[_D_SCALE] = dev_st.data_ptr() + 4 * int(host_st[1042 + r - lo])
            d[_D_TAPS] = hip.augment_scale_taps(size, r)
        if d[_D_ROT]:
            d[_D_COEF:_D_COEF + 6] = _rotation(size, int(d[_D_DEG]))
    return desc


def transform(packed, desc, size):
    """packed: the device copy of a bound batch, desc: its host descriptors -> (images (B, 3, S, S) f32, label
    (B, 1, S, S) f32) on packed's device and the current stream: the train transform of every sample, bit for bit."""
    device = packed.device
    b = desc.shape[0]
    key = (size, str(device))
    need = hip.augment_workspace_bytes(b, size)
    ws = _workspace.get(key)
    if ws is None or ws.numel() < need:
        ws = _workspace[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return hip.augment_batch(packed, desc, size_table(size, device)[0], size, ws)


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def device_train_batches(root, img_size=384, batch_size=4, num_workers=8, rank=0, world_size=1, seed=1026,
                         distinct_workers=True, device="cuda"):
    """The `batches(epoch)` callable of `tramba_amd.train.fit` (arguments as `data.train_loader`): the same shuffle,
    shards, worker streams and draws, the transform on the device.  Each packed batch goes up with one asynchronous copy on
    a side stream (it overlaps the previous step), which the current stream waits for before the transform."""
    ds = PairDataset(root, ["Train"], img_size)
    loader = data._train_dataloader(ds, batch_size, num_workers, rank, world_size, seed, distinct_workers,
                                    collate_fn=Collate(img_size))
    device = _device(device)
    streams = {}

    def batches(epoch):
        if hasattr(loader.sampler, "set_epoch"):
            loader.sampler.set_epoch(epoch)
        for batch in loader:
            desc = bind(descriptors(batch), img_size, device)
            cur = torch.cuda.current_stream(device)
            side = streams.get(cur.cuda_stream)
            if side is None:
                side = streams[cur.cuda_stream] = torch.cuda.Stream(device)
            with torch.cuda.stream(side):
                packed = batch["packed"].to(device, non_blocking=True)
            cur.wait_stream(side)
            packed.record_stream(cur)
            yield transform(packed, desc, img_size)

    batches.loader = loader
    return batches
