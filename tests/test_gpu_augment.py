"""GPU tests of the device train transform (tramba_amd/augment.py, csrc/augment.hip): bit for bit the reference-made golden
train cases and data.get_transform(S, "train") under the same draws, independent of the batch, capturable, and
device_train_batches equal to device_batches(train_loader(...)) over a folder.  The host side: tests/test_augment_host.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


def _pair(h, w, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[: h // 3, : w // 3] = 255
    img[2 * h // 3:, 2 * w // 3:] = 0
    yy, xx = np.mgrid[0:h, 0:w]
    gt = (((yy - h / 2) ** 2 / max(h, 1) ** 2 + (xx - w / 3) ** 2 / max(w, 1) ** 2) < 0.1).astype(np.uint8) * 255
    gt[::7] = rs.randint(0, 256, gt[::7].shape)         # grey levels too
    return img, gt


def _device(samples, size):
    from tramba_amd import augment
    batch = augment.pack(samples, size)
    desc = augment.bind(augment.descriptors(batch), size, torch.device(DEV, torch.cuda.current_device()))
    packed = batch["packed"].to(DEV)
    return augment.transform(packed, desc, size)



def test_golden_train_cases():
    from tramba_amd import augment
    gold = np.load(os.path.join(HERE, "golden", "golden_data.npz"))
    rec = augment.DrawRecorder(np.random.RandomState(1026))
    samples = []
    for i in range(synth.DATA_TRAIN_SAMPLES):
        w, h = synth.DATA_SOURCES[i % len(synth.DATA_SOURCES)]
        img, gt = synth.image_pair(f"train{i}", w, h)
        samples.append((np.asarray(img.convert("RGB")), np.asarray(gt.convert("L")), rec(synth.DATA_SIZE)))
    image, label = _device(samples, synth.DATA_SIZE)
    for i in range(synth.DATA_TRAIN_SAMPLES):
        assert torch.equal(image[i].cpu(), torch.from_numpy(gold[f"train{i}_image"])), i
        assert torch.equal(label[i].cpu(), torch.from_numpy(gold[f"train{i}_gt"])), i


SOURCES = [(1080, 1920), (375, 500), (383, 385), (2, 3000), (1, 1), (384, 384), (600, 200), (256, 256)]


@pytest.mark.parametrize("size,n", [(384, 200), (256, 208)])
def test_seeded_samples_equal_the_host_transform(size, n):
    from tramba_amd import augment
    seed = 4242 + size
    host_rng, dev_rng = np.random.RandomState(seed), np.random.RandomState(seed)
    rec = augment.DrawRecorder(dev_rng)
    from tramba_amd import data
    tf = data.get_transform(size, "train", rng=host_rng)
    cover = set()
    pairs = [_pair(h, w, 11 * h + w) for h, w in SOURCES]
    for start in range(0, n, 8):
        samples, want = [], []
        for i in range(start, start + 8):
            img, gt = pairs[i % len(pairs)]
            r = rec(size)
            s = tf({"image": Image.fromarray(img), "gt": Image.fromarray(gt)})
            want.append((s["image"], s["gt"]))
            samples.append((img, gt, r))
            cover.add("up" if r["scale"] > size else "down" if r["scale"] and r["scale"] < size else
                      "same" if r["scale"] == size else "noscale")
            cover.add("mirror" if r["mirror"] else "nomirror")
            d = r["degrees"]
            cover.add("norot" if d is None else "zero" if d == 0 else "neg" if d > 180 else "pos")
            cover.update(f"e{code}@{pos}" for pos, (code, _) in enumerate(r["enhance"]))
        image, label = _device(samples, size)
        for j, (wi, wg) in enumerate(want):
            assert torch.equal(image[j].cpu(), wi), (start + j, samples[j][2])
            assert torch.equal(label[j].cpu(), wg), (start + j, samples[j][2])
    need = {"up", "down", "noscale", "mirror", "nomirror", "norot", "neg", "pos", "zero"}
    need |= {f"e{c}@{p}" for c in range(3) for p in range(3)}
    assert need <= cover, need - cover


def test_sample_is_independent_of_its_batch():
    from tramba_amd import augment
    size = 256
    rec = augment.DrawRecorder(np.random.RandomState(99))
    samples = [(*_pair(h, w, h + 3 * w), rec(size)) for h, w in SOURCES]
    image, label = _device(samples, size)
    for j in (0, 3, 7):
        one_i, one_l = _device([samples[j]], size)
        assert torch.equal(one_i[0], image[j]) and torch.equal(one_l[0], label[j]), j


def test_captured_graph_replays_equal_to_eager():
    from tramba_amd import augment
    size = 256
    rec = augment.DrawRecorder(np.random.RandomState(5))
    samples = [(*_pair(h, w, h * 5 + w), rec(size)) for h, w in SOURCES[:4]]
    batch = augment.pack(samples, size)
    dev = torch.device(DEV, torch.cuda.current_device())
    desc = augment.bind(augment.descriptors(batch), size, dev)
    packed = batch["packed"].to(DEV)
    eager = augment.transform(packed, desc, size)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            got = augment.transform(packed, desc, size)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        got[0].zero_()
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])


def _folder(root, n=7):
    for sub in ("image", "mask"):
        os.makedirs(os.path.join(root, "Train", sub))
    sizes = [(40, 30), (33, 47), (64, 64), (20, 90), (50, 51), (31, 29), (77, 40)]
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        img, gt = _pair(h, w, 100 + i)
        Image.fromarray(img).save(os.path.join(root, "Train", "image", f"p{i}.png"))
        Image.fromarray(gt).save(os.path.join(root, "Train", "mask", f"p{i}.png"))


@pytest.mark.parametrize("workers", [0, 2])
def test_device_train_batches_equal_the_host_loader(tmp_path, workers):
    from tramba_amd import augment, data
    root = str(tmp_path)
    _folder(root)
    for world, ranks in ((1, [0]), (2, [0, 1])):
        for rank in ranks:
            def run(make):
                np.random.seed(1026)
                torch.manual_seed(1026)
                batches = make()
                return [[(i.clone(), l.clone()) for i, l in batches(e)] for e in range(2)]
            want = run(lambda: data.device_batches(data.train_loader(root, 32, batch_size=3, num_workers=workers,
                                                                     rank=rank, world_size=world)))
            got = run(lambda: augment.device_train_batches(root, 32, batch_size=3, num_workers=workers, rank=rank,
                                                           world_size=world))
            assert len(got) == len(want) == 2
            for e in range(2):
                assert len(got[e]) == len(want[e]) > 0
                for (gi, gl), (wi, wl) in zip(got[e], want[e]):
                    assert gi.is_cuda and torch.equal(gi, wi) and torch.equal(gl, wl), (workers, world, rank, e)


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.vssm_encoder = nn.Conv2d(3, 4, 3, padding=1)
        self.decoder = nn.Conv2d(4, 1, 1)

    def forward(self, x):
        y = self.decoder(torch.relu(self.vssm_encoder(x)))
        return [nn.functional.avg_pool2d(y, 2), y]


def test_fit_runs_on_device_batches(tmp_path):
    from tramba_amd import augment, train
    root = str(tmp_path / "data")
    _folder(root)
    torch.manual_seed(0)
    m = _Tiny().to(DEV)
    opt = train.get_opt(1e-3, m)
    batches = augment.device_train_batches(root, 32, batch_size=2, num_workers=0)
    hist = train.fit(m, opt, batches, epochs=2, base_lr=1e-3, decay_epochs=[], decay_factors=[],
                     save_model=str(tmp_path / "ck"), method="Tramba-V-TSOD")
    assert len(hist) == 2
    assert all(np.isfinite(h["loss"]) for h in hist)
