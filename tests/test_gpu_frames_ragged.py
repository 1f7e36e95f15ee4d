"""GPU tests of the mixed-size frame path (tramba_amd/infer.py on a LIST of frames, csrc/frames.hip *_ragged): every
frame's input plane and map are bit for bit what the uniform kernels give for that frame alone, one captured graph serves
every mix of sizes that fits its buffers, predict_folder(batch=N) writes save_predictions' bytes for the same grouping,
and evaluate_dataset gives exactly evaluate_folder's numbers over those PNGs.  The host side:
tests/test_frames_ragged_host.py.  Every GPU step is an ordinary launch; the refusals are all caught on the host."""
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


def _mixed_batches():
    """the 12 sizes shuffled (seeded) into batches of 1, 3, 4 and 7 frames; the last batch wraps round"""
    order = [SIZES[i] for i in np.random.RandomState(12).permutation(len(SIZES))]
    order = order + order[:3]
    return [order[0:1], order[1:4], order[4:8], order[8:15]]


# ----------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("channels", ["RGB", "BGR"])
@pytest.mark.parametrize("s", TARGETS)
def test_preprocess_of_a_mixed_list_equals_each_frame_alone_and_the_loader(s, channels):
    from tramba_amd import infer
    for k, sizes in enumerate(_mixed_batches()):
        rgb = [_frame(h, w, seed=1000 * k + i) for i, (h, w) in enumerate(sizes)]
        frames = [np.ascontiguousarray(f[..., ::-1]) for f in rgb] if channels == "BGR" else rgb
        got = infer.preprocess(frames, s, channels=channels)                 # host input: a list of numpy frames
        assert got.shape == (len(sizes), 3, s, s) and got.dtype == torch.float32 and got.is_cuda
        alone = torch.cat([infer.preprocess(f, s, channels=channels) for f in frames])
        assert torch.equal(got, alone), (sizes, int((got != alone).sum()))
        for i, f in enumerate(rgb):
            want = _loader_image(f, s)
            assert torch.equal(got[i].cpu(), want), (sizes[i], int((got[i].cpu() != want).sum()))


def test_preprocess_takes_tuples_and_host_tensors():
    from tramba_amd import infer
    frames = (torch.from_numpy(_frame(40, 60, 1)), _frame(61, 33, 2))
    got = infer.preprocess(frames, 256)
    for i, f in enumerate(frames):
        assert torch.equal(got[i].cpu(), _loader_image(np.asarray(f), 256))


# ----------------------------------------------------------------------------- postprocess
POST_SIZES = [(384, 384), (1, 1), (2000, 64), (1080, 1920), (5, 7), (384, 383), (777, 333)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_postprocess_with_a_list_of_sizes(dtype):
    from tramba_amd import infer
    g = torch.Generator().manual_seed(77)
    logits = (torch.randn(len(POST_SIZES), 1, 384, 384, generator=g) * 6).to(dtype).to(DEV)
    maps = infer.postprocess(logits, POST_SIZES)
    assert isinstance(maps, list) and len(maps) == len(POST_SIZES)
    for i, (m, size) in enumerate(zip(maps, POST_SIZES)):
        assert m.shape == size and m.dtype == torch.uint8 and m.is_cuda
        alone = infer.postprocess(logits[i:i + 1], size)[0]
        want = _torch_post(logits[i:i + 1], *size)[0]
        assert torch.equal(m, alone), (size, int((m != alone).sum()))
        assert torch.equal(m, want), (size, int((m != want).sum()))
    base = maps[0].data_ptr()
    assert all((m.data_ptr() - base) % 16 == 0 for m in maps)           # views into one buffer, each 16-byte aligned


def test_postprocess_leaves_a_canary_past_the_capacity_untouched():
    from tramba_amd import hip, infer
    sizes = [(1, 1), (300, 401), (5, 7), (384, 384)]
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(len(sizes), 1, 384, 384, generator=g) * 6).to(DEV)
    desc = infer.size_descriptors(sizes, 384)
    need = infer.output_bytes(desc)
    head = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(DEV)
    for cap in (need, need + 4096 * 3 + 16):                             # exact, and with workgroups past the last byte
        whole = torch.full((cap + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        hip.logits_to_u8_ragged(logits, head, desc, whole[:cap])
        assert bool((whole[cap:] == 0xA5).all()), "bytes past the capacity were written"
        for i, (m, size) in enumerate(zip(infer._map_views(whole, desc), sizes)):
            assert torch.equal(m, _torch_post(logits[i:i + 1], *size)[0]), size


@pytest.fixture(scope="module")
def model():
    """Tramba-V with synthetic weights, prepared for bf16 inference (the deployment form).  Its forward is bitwise
    reproducible run to run, which the fp32 forward is not (tests/test_gpu_frames.py), so byte-exact comparisons of whole
    pipelines are meaningful with it."""
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


def test_postprocess_of_a_tramba_output_with_a_list_of_sizes(model):
    from tramba_amd import infer
    sizes = [(1080, 1920), (384, 384), (500, 375)]
    x = torch.stack([_loader_image(_frame(*hw, seed=5 + i), 384) for i, hw in enumerate(sizes)]).to(DEV)
    with torch.no_grad():
        res = model(x)[-1]
    for i, (m, size) in enumerate(zip(infer.postprocess(res, sizes), sizes)):
        assert torch.equal(m, infer.postprocess(res[i:i + 1], size)[0]) and torch.equal(m, _torch_post(res[i:i + 1], *size)[0])


# ----------------------------------------------------------------------------- one graph for every mix
# five mixes of four frames whose packed bytes and map bytes fall into ONE pair of capacity buckets (4 MiB in, 1 MiB out)
MIXES = [[(480, 640), (375, 500), (600, 400), (300, 500)],
         [(500, 375), (640, 480), (333, 777), (200, 600)],
         [(720, 540), (360, 640), (384, 384), (100, 1000)],
         [(1, 1), (768, 1024), (5, 7), (300, 400)],
         [(427, 640), (640, 427), (512, 512), (250, 333)]]
BIGGER = [(1080, 1920), (300, 400), (5, 7), (384, 384)]


def _saved_maps(model, frames, names, out_dir):
    """what save_predictions writes for these frames as ONE batch, read back"""
    from tramba_amd import evaluate
    batch = {"image": torch.stack([_loader_image(f, 384) for f in frames]),
             "shape": (torch.tensor([f.shape[1] for f in frames]), torch.tensor([f.shape[0] for f in frames])),
             "name": list(names)}
    evaluate.save_predictions(model, [batch], str(out_dir))
    return [np.asarray(Image.open(os.path.join(out_dir, n + ".png"))) for n in names]


def _ragged_keys(pred):
    return [k for k in pred._graphs if k[0] == "ragged"]


def test_one_graph_serves_every_mix_of_sizes(model, tmp_path):
    from tramba_amd import infer
    graphed = infer.FramePredictor(model, 384, graph=True, strict=True)
    eager = infer.FramePredictor(model, 384, graph=False)
    batches = [[_frame(h, w, seed=31 * k + i) for i, (h, w) in enumerate(mix)] for k, mix in enumerate(MIXES)]
    buckets = set()
    for frames in batches:                                   # the premise: one bucket pair
        b = infer.pack_frames(frames, 384)
        buckets.add((infer.capacity_bucket(b["packed"].numel()), infer.capacity_bucket(infer.output_bytes(infer.descriptors(b)))))
    assert len(buckets) == 1, buckets
    first = None
    for k, (frames, mix) in enumerate(zip(batches, MIXES)):
        got = [m.clone() for m in graphed(frames)]
        assert [tuple(m.shape) for m in got] == mix and all(m.dtype == torch.uint8 and m.is_cuda for m in got)
        want = _saved_maps(model, frames, [f"m{k}_{i}" for i in range(4)], tmp_path)
        for i, (m, e, w) in enumerate(zip(got, eager(frames), want)):
            assert torch.equal(m, e), (k, i, "graphed and eager differ", int((m != e).sum()))
            assert np.array_equal(m.cpu().numpy(), w), (k, i, int((m.cpu().numpy() != w).sum()))
        if first is None:
            first = got
        assert len(_ragged_keys(graphed)) == 1 and len(graphed._graphs) == 1
    assert all(v is not None for v in graphed._graphs.values())
    # a batch that does not fit moves to the next bucket: exactly one more graph
    big = [_frame(h, w, seed=900 + i) for i, (h, w) in enumerate(BIGGER)]
    got = [m.clone() for m in graphed(big)]
    assert len(_ragged_keys(graphed)) == 2 and all(v is not None for v in graphed._graphs.values())
    for m, e in zip(got, eager(big)):
        assert torch.equal(m, e)
    # the first mix again: the smaller graph, the first result bit for bit
    again = graphed(batches[0])
    assert len(_ragged_keys(graphed)) == 2
    for m, f in zip(again, first):
        assert torch.equal(m, f), "a replay of the first mix differs from its first result"
    # BGR is a graph of its own, with the same maps
    bgr = infer.FramePredictor(model, 384, channels="BGR", graph=True, strict=True)
    for m, f in zip(bgr([np.ascontiguousarray(f[..., ::-1]) for f in batches[0]]), first):
        assert torch.equal(m, f)


def test_uniform_input_keeps_its_path_and_its_result(model):
    from tramba_amd import hip, infer
    frames = np.stack([_frame(300, 500, seed=k) for k in range(3)])
    x = torch.from_numpy(frames).to(DEV)
    with torch.no_grad():
        inp = hip.frames_to_input(x, infer.resize_table(300, 500, 384, x.device), 384, 384, False)
        want = hip.logits_to_u8(model(inp)[-1], 300, 500)
    for graph in (True, False):
        pred = infer.FramePredictor(model, 384, graph=graph, strict=True)
        got = pred(frames)
        assert torch.is_tensor(got) and got.shape == (3, 300, 500) and torch.equal(got, want)
        assert torch.equal(pred(frames[0])[0], pred(frames[:1])[0])
        assert not _ragged_keys(pred) and len(pred._graphs) == (2 if graph else 0)
    assert torch.equal(infer.preprocess(frames, 384), inp)


# ----------------------------------------------------------------------------- folders
FOLDER = [("a_wide", (300, 500)), ("b_tall", (640, 360)), ("c_1080p", (1080, 1920)), ("d_small", (97, 131)),
          ("e_wide", (300, 500)), ("f_square", (384, 384)), ("g_odd", (333, 777))]


def _mask(h, w, k):
    """seeded blobs; image 1 has an empty mask and image 2 a full one"""
    if k == 1:
        return np.zeros((h, w), np.uint8)
    if k == 2:
        return np.full((h, w), 255, np.uint8)
    rs = np.random.RandomState(500 + k)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(3):
        cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.randint(min(h, w) // 8 + 1, min(h, w) // 3 + 2)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return np.where(m, rs.choice([255, 128, 1]), 0).astype(np.uint8)        # non-zero is foreground, whatever the level


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """<root>/Test/image/*.png + mask/*.png; the names sort the same way naturally and as plain strings, and image and
    mask share the full file name, so RGB_Dataset and evaluate_folder pair and order them alike"""
    root = tmp_path_factory.mktemp("ragged_set")
    for sub in ("image", "mask"):
        os.makedirs(root / "Test" / sub)
    for k, (name, hw) in enumerate(FOLDER):
        Image.fromarray(_frame(*hw, seed=300 + k)).save(root / "Test" / "image" / f"{name}.png")
        Image.fromarray(_mask(*hw, k)).save(root / "Test" / "mask" / f"{name}.png")
    return root


def test_predict_folder_in_batches_writes_save_predictions_bytes(model, dataset, tmp_path):
    from tramba_amd import data, evaluate, infer
    folder = dataset / "Test" / "image"
    frames = [np.asarray(Image.open(folder / f"{n}.png").convert("RGB")) for n, _ in FOLDER]
    names = [n for n, _ in FOLDER]
    ref = tmp_path / "ref3"
    for lo in (0, 3, 6):                                          # the same groups of 3 / 3 / 1, in the same order
        _saved_maps(model, frames[lo:lo + 3], names[lo:lo + 3], ref)
    for graph in (True, False):
        out = tmp_path / f"pred3_{graph}"
        written = infer.predict_folder(model, str(folder), str(out), 384, graph=graph, workers=4, batch=3)
        assert [os.path.basename(p) for p in written] == [f"{n}.png" for n in names]
        for n in names:
            assert (out / f"{n}.png").read_bytes() == (ref / f"{n}.png").read_bytes(), (graph, n)
    one = tmp_path / "ref1"
    evaluate.save_predictions(model, data.eval_loader(str(dataset), 384, num_workers=0), str(one))
    out = tmp_path / "pred1"
    infer.predict_folder(model, str(folder), str(out), 384, workers=4, batch=1)
    for n in names:
        assert (out / f"{n}.png").read_bytes() == (one / f"{n}.png").read_bytes(), n


@pytest.mark.parametrize("batch", [1, 4])
def test_evaluate_dataset_equals_evaluate_folder_over_predict_folder(model, dataset, tmp_path, batch):
    """Order: evaluate_dataset steps a_wide .. g_odd in the loader's natural order, evaluate_folder in sorted() order of
    the same names; the two coincide for this set, so the floating-point means are taken over the same sequence."""
    from tramba_amd import evaluate, infer
    pngs = tmp_path / "pngs"
    infer.predict_folder(model, str(dataset / "Test" / "image"), str(pngs), 384, batch=batch)
    want = evaluate.evaluate_folder(str(pngs), str(dataset / "Test" / "mask"))
    saved = tmp_path / "saved"
    for save_path in (None, str(saved)):
        got = evaluate.evaluate_dataset(model, str(dataset), 384, batch=batch, save_path=save_path)
        assert list(got) == list(want)
        for key in want:
            print(batch, save_path is not None, key, got[key] if np.ndim(got[key]) == 0 else "curve", flush=True)
            if isinstance(want[key], np.ndarray) and want[key].ndim:
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
            else:
                assert got[key] == want[key], (key, got[key], want[key])
    for n, _ in FOLDER:
        assert (saved / f"{n}.png").read_bytes() == (pngs / f"{n}.png").read_bytes(), n
    assert 0.0 < float(want["MAE_r"]) < 1.0 and float(want["Wmeasure_r"]) >= 0.0
    light = evaluate.evaluate_dataset(model, str(dataset), 384, batch=batch, graph=False, weighted=False)
    assert light["Wmeasure_r"] is None and light["MAE_r"] == want["MAE_r"] and light["Smeasure_r"] == want["Smeasure_r"]
    assert not model.training


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_predictor_working(model):
    from tramba_amd import hip, infer
    ok = _frame(32, 48, 0)
    for graph in (False, True):
        pred = infer.FramePredictor(model, 384, graph=graph, strict=True)
        with pytest.raises(TypeError):
            pred([ok, np.zeros((32, 32, 3), np.float32)])
        with pytest.raises(ValueError):
            pred([np.zeros((32, 32, 4), np.uint8)])
        with pytest.raises(ValueError):
            pred([ok, np.zeros((hip.FRAME_MAX_DIM + 1, 1, 3), np.uint8)])
        with pytest.raises(ValueError):
            pred([])
        with pytest.raises(ValueError):
            pred([torch.from_numpy(ok).to(DEV)])                   # a mixed-size batch is packed on the host
        maps = pred([ok, _frame(20, 10, 1)])
        assert [tuple(m.shape) for m in maps] == [(32, 48), (20, 10)]
        again = infer.FramePredictor(model, 384, graph=False)([ok, _frame(20, 10, 1)])    # the same batch of two
        assert torch.equal(maps[0], again[0]) and torch.equal(maps[1], again[1])
    with pytest.raises(ValueError):
        infer.postprocess(torch.zeros(2, 1, 8, 8, device=DEV), [(4, 4)])
    with pytest.raises(hip.TrambaHipError):
        infer.postprocess(torch.zeros(1, 1, 8, 8, device=DEV), [(hip.FRAME_MAX_DIM + 1, 8)])
    with pytest.raises(ValueError):
        infer.predict_folder(model, ".", ".", batch=0)
