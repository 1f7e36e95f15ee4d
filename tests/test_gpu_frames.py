"""GPU tests of the deployment pipeline (tramba_amd/infer.py, csrc/frames.hip): preprocess is bit for bit the loader's test
transform, postprocess is bit for bit save_predictions' torch sequence, and FramePredictor / predict_folder give the maps
and the PNG bytes that save_predictions gives for the same images.  The host side: tests/test_frames_host.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(384, 384), (384, 500), (500, 384), (200, 600), (600, 200), (1, 1), (2, 3000), (5, 7), (375, 500), (383, 385),
         (1080, 1920), (3000, 4000)]
TARGETS = [256, 384, 768]


def _frame(h, w, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[: h // 2, : w // 2] = 255
    img[h // 2:, w // 2:] = 0
    return img


def _loader_image(img, s):
    from tramba_amd import data
    return data.get_transform(s, "Test")({"image": Image.fromarray(img)})["image"]


def _torch_post(logits, h, w):
    """evaluate.save_predictions, per image"""
    up = F.interpolate(logits.float(), size=(h, w), mode="bilinear", align_corners=False)
    return (torch.sigmoid(up) * 255).to(torch.uint8)[:, 0]


# ----------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("s", TARGETS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_preprocess_equals_loader_transform(hw, s):
    from tramba_amd import infer
    img = _frame(*hw, seed=hw[0] * 31 + hw[1])
    got = infer.preprocess(torch.from_numpy(img).to(DEV), s)
    assert got.shape == (1, 3, s, s) and got.dtype == torch.float32 and got.is_cuda
    want = _loader_image(img, s)
    assert torch.equal(got[0].cpu(), want), int((got[0].cpu() != want).sum())


@pytest.mark.parametrize("hw", [(1080, 1920), (200, 600), (7, 5)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_preprocess_batches_host_input_and_bgr(hw):
    from tramba_amd import infer
    frames = np.stack([_frame(*hw, seed=k) for k in range(3)])
    want = torch.stack([_loader_image(f, 384) for f in frames])
    host = infer.preprocess(frames, 384)                              # numpy on the host
    dev = infer.preprocess(torch.from_numpy(frames).to(DEV), 384)     # tensor on the device
    bgr = infer.preprocess(np.ascontiguousarray(frames[..., ::-1]), 384, channels="BGR")
    for got in (host, dev, bgr):
        assert got.shape == (3, 3, 384, 384) and torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------- postprocess
@pytest.mark.parametrize("size", [(1080, 1920), (384, 384), (200, 600), (777, 333), (1, 1), (2000, 64)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_postprocess_equals_torch_sequence(size, dtype):
    from tramba_amd import infer
    g = torch.Generator().manual_seed(size[0] * 7 + size[1])
    logits = (torch.randn(2, 1, 384, 384, generator=g) * 6).to(dtype).to(DEV)
    got = infer.postprocess(logits, size)
    want = _torch_post(logits, *size)
    assert got.shape == (2,) + size and got.dtype == torch.uint8
    assert torch.equal(got, want), int((got != want).sum())


@pytest.fixture(scope="module")
def model():
    """Tramba-V with synthetic weights, prepared for bf16 inference (the deployment form).  Its forward is bitwise
    reproducible run to run; the fp32 forward is not (measured on an MI355X: ~140k of 147k output floats of a 384x384 map
    differ between two eager runs), so the byte-exact comparisons below would not be meaningful with it."""
    import tramba_amd as ta
    torch.manual_seed(0)
    m = ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=384, dims=128, depths=[2, 2, 2, 2])
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        if k not in new:
            new[k] = sd[k]
    m.load_state_dict(new, strict=True)
    return ta.prepare_inference(m.to(DEV).eval(), torch.bfloat16)


@pytest.mark.parametrize("size", [(1080, 1920), (384, 384), (500, 375)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_postprocess_of_a_tramba_output(model, size):
    from tramba_amd import infer
    x = torch.stack([_loader_image(_frame(*size, seed=5), 384)]).to(DEV)
    with torch.no_grad():
        res = model(x)[-1]
    assert torch.equal(infer.postprocess(res, size), _torch_post(res, *size))


# ----------------------------------------------------------------------------- the whole pipeline
SET = [("a_1080p", (1080, 1920)), ("b_small", (300, 500)), ("c_small", (300, 500)), ("d_tall", (640, 360))]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """<root>/Test/image/*.png + mask/*.png, the layout eval_loader reads"""
    root = tmp_path_factory.mktemp("frames_set")
    for sub in ("image", "mask"):
        os.makedirs(root / "Test" / sub)
    for k, (name, hw) in enumerate(SET):
        Image.fromarray(_frame(*hw, seed=100 + k)).save(root / "Test" / "image" / f"{name}.png")
        Image.fromarray(np.zeros(hw, np.uint8)).save(root / "Test" / "mask" / f"{name}.png")
    return root


@pytest.fixture(scope="module")
def saved(model, dataset):
    """what save_predictions writes for the set"""
    from tramba_amd import data, evaluate
    out = dataset / "saved"
    evaluate.save_predictions(model, data.eval_loader(str(dataset), 384, num_workers=0), str(out))
    return out


def test_frame_predictor_graphed_equals_eager_and_save_predictions(model, dataset, saved):
    from tramba_amd import infer
    graphed = infer.FramePredictor(model, 384, graph=True, strict=True)
    eager = infer.FramePredictor(model, 384, graph=False)
    for name, hw in SET:
        frame = np.asarray(Image.open(dataset / "Test" / "image" / f"{name}.png").convert("RGB"))
        want = np.asarray(Image.open(saved / f"{name}.png"))
        first = graphed(frame).clone()
        again = graphed(torch.from_numpy(frame).to(DEV))
        e = eager(frame)
        assert first.shape == (1,) + hw and first.dtype == torch.uint8
        assert torch.equal(first, again), "graph replays differ"
        assert torch.equal(first, e), "graphed and eager differ"
        assert np.array_equal(first[0].cpu().numpy(), want), int((first[0].cpu().numpy() != want).sum())
    assert len(graphed._graphs) == 3 and all(v is not None for v in graphed._graphs.values())


def test_predict_folder_writes_save_predictions_bytes(model, dataset, saved, tmp_path):
    from tramba_amd import infer
    for graph in (True, False):
        out = tmp_path / f"pred_{graph}"
        written = infer.predict_folder(model, str(dataset / "Test" / "image"), str(out), 384, graph=graph, workers=4)
        assert sorted(os.path.basename(p) for p in written) == sorted(f"{n}.png" for n, _ in SET)
        for name, _ in SET:
            assert (out / f"{name}.png").read_bytes() == (saved / f"{name}.png").read_bytes(), name


# ----------------------------------------------------------------------------- refusals
def test_refusals(model):
    import tramba_amd as ta
    from tramba_amd import hip, infer
    pred = infer.FramePredictor(model, 384, graph=False)
    with pytest.raises(TypeError):
        pred(np.zeros((32, 32, 3), np.float32))
    with pytest.raises(TypeError):
        infer.preprocess(torch.zeros(32, 32, 3, device=DEV))
    with pytest.raises(ValueError):
        pred(np.zeros((32, 32, 4), np.uint8))
    with pytest.raises(ValueError):
        infer.preprocess(np.zeros((32, 32, 1), np.uint8))
    with pytest.raises(ValueError):
        infer.preprocess(np.zeros((32, 32, 3), np.uint8), channels="RGBA")
    over = torch.zeros(1, hip.FRAME_MAX_DIM + 1, 1, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        infer.preprocess(over)
    with pytest.raises(hip.TrambaHipError):                        # the wrapper / ABI refuse it too, before a launch
        hip.frames_to_input(over, torch.zeros(1 << 16, dtype=torch.int32, device=DEV), 384, 384)
    with pytest.raises(hip.TrambaHipError):
        infer.preprocess(np.zeros((32, 32, 3), np.uint8), img_size=hip.FRAME_MAX_OUT + 1)
    with pytest.raises(hip.TrambaHipError):
        infer.postprocess(torch.zeros(1, 1, 8, 8, device=DEV), (hip.FRAME_MAX_DIM + 1, 8))
    cpu = ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=384).eval()
    with pytest.raises(RuntimeError, match="CPU"):
        infer.FramePredictor(cpu)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            infer.FramePredictor(model)
        with pytest.raises(RuntimeError, match="training"):
            pred(np.zeros((32, 32, 3), np.uint8))
    finally:
        model.eval()
