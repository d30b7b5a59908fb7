"""GPU tests of the grounding input pipeline (csrc/input.hip det_* kernels through fiber_amd/data.py): the padded batch against the numpy
restatement of tests/det_input_cases.py over the WHOLE tensor with np.array_equal (integer work plus single correctly rounded fp32
operations: there is no tolerance), the committed PIL fixtures on the device, the box kernel against the reference-run fixture, the bicubic
neighbour after the coefficient code was generalised, and raw samples through device_collate_grounding into GeneralizedVLRCNN."""
import numpy as np
import pytest
import torch

import det_input_cases as dc
import fpn_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_SIZES, MAX_SIZE = (48, 64, 80), 133


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from fiber_amd import lib as L
    L.load()
    return L


def _images(shapes, seed):
    """Host images of the (H, W) shapes, the second to last a row-strided view of a wider one -> (host arrays, device tensors)"""
    rng = np.random.default_rng(seed)
    host = [dc.synth_image(H, W, seed=H * 1000 + W) if i % 2 == 0 else rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            for i, (H, W) in enumerate(shapes)]
    dev = [torch.from_numpy(im).to(DEV) for im in host]
    if len(shapes) > 2:
        i = len(shapes) - 2
        H, W = shapes[i]
        wide = torch.from_numpy(rng.integers(0, 256, (H, W + 30, 3), dtype=np.uint8)).to(DEV)
        dev[i] = wide[:, 10:10 + W]                                # packed pixels, row stride > 3 W
        host[i] = dev[i].cpu().numpy()
        assert dev[i].stride(0) == 3 * (W + 30)
    return host, dev


def _find_seed(shapes, cond, flip=0.5):
    for seed in range(1, 4000):
        ch = dc.choices_ref(seed, shapes, MIN_SIZES, MAX_SIZE, flip)
        if cond(ch):
            return seed, ch
    raise AssertionError("no seed below 4000 gives the wanted choices")


# the ragged batch: a downscale, an upscale, a capped portrait, the early return (when 64 is drawn), a cap-engaged panorama, a sliver that is
# one pixel high after the resize, a row-strided view, an odd upscale
RAGGED = [(97, 131), (20, 30), (150, 40), (64, 64), (61, 200), (2, 200), (50, 60), (33, 47)]


def _ragged_cond(ch):
    sizes, flips = [c[0] for c in ch], [c[1] for c in ch]
    return (sizes[3] == (64, 64) and any(f and s[1] % 2 == 1 for s, f in ch) and any(f and s[1] % 2 == 0 for s, f in ch)
            and not all(flips[:5]) and flips[5] and flips[6])


@pytest.mark.parametrize("fmt", ["bgr255", "rgb"])
def test_ragged_batch_bit_exact(lib, fmt):
    from fiber_amd import data
    mean, std = (dc.BGR255_MEAN, dc.BGR255_STD) if fmt == "bgr255" else (dc.RGB_MEAN, dc.RGB_STD)
    cfg = dc.input_cfg(min_size=MIN_SIZES, max_size=MAX_SIZE, fmt="" if fmt == "bgr255" else fmt, mean=mean, std=std)
    t = data.DeviceDetectionTransform(cfg, is_train=True)
    seed, ch = _find_seed(RAGGED, _ragged_cond)
    assert ch[4][0][1] > 128 and ch[5][0][0] == 1 and ch[0][0][0] < 97 and ch[1][0][0] > 20        # cap engaged, the sliver, down, up
    host, dev = _images(RAGGED, 5)
    out = t(dev, seed)
    assert out.image_sizes == [c[0] for c in ch] and out.original == [(H, W, c[1]) for (H, W), c in zip(RAGGED, ch)]
    ref = dc.batch_ref(host, ch, fmt, mean, std, 32)
    got = out.tensors.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got, ref), [b for b in range(len(host)) if not np.array_equal(got[b], ref[b])]
    for b, ((oh, ow), _) in enumerate(ch):                          # the padding is exactly +0.0
        assert not got[b, :, oh:].any() and not got[b, :, :, ow:].any()
        assert not np.signbit(got[b, :, oh:]).any() and not np.signbit(got[b, :, :, ow:]).any()
    # the same seed gives the same batch bit for bit, without a seed the key stream advances
    assert torch.equal(t(dev, seed).tensors, out.tensors)


def test_no_padding_image_and_a_much_narrower_one(lib):
    """An image whose (oh, ow) already equals (Hp, Wp) beside one that fills 48 of 128 columns.  (With max_size 133 and divisibility 32
    the cap-engaged panorama of the ragged batch is 134 wide, Wp = 160, and no resized image can be: this pair is a batch of its own.)"""
    from fiber_amd import data
    shapes = [(64, 128), (60, 45)]
    seed, ch = _find_seed(shapes, lambda ch: ch[0][0] == (64, 128) and ch[1][0] == (64, 48) and ch[1][1])
    t = data.DeviceDetectionTransform(dc.input_cfg(min_size=MIN_SIZES, max_size=MAX_SIZE), is_train=True)
    host, dev = _images(shapes, 6)
    out = t(dev, seed)
    assert tuple(out.tensors.shape) == (2, 3, 64, 128)
    assert np.array_equal(out.tensors.cpu().numpy(), dc.batch_ref(host, ch, "bgr255", dc.BGR255_MEAN, dc.BGR255_STD, 32))


@pytest.mark.parametrize("fmt", ["bgr255", "rgb"])
def test_single_image_eval(lib, fmt):
    """B = 1, is_train False: MIN_SIZE_TEST, never flipped"""
    from fiber_amd import data
    mean, std = (dc.BGR255_MEAN, dc.BGR255_STD) if fmt == "bgr255" else (dc.RGB_MEAN, dc.RGB_STD)
    cfg = dc.input_cfg(min_size=MIN_SIZES, max_size=MAX_SIZE, fmt="" if fmt == "bgr255" else fmt, mean=mean, std=std)
    t = data.DeviceDetectionTransform(cfg, is_train=False)
    img = dc.synth_image(97, 131, 3)
    out = t([torch.from_numpy(img).to(DEV)], seed=77)
    ch = [(dc.get_size_ref(131, 97, 48, MAX_SIZE), False)]
    assert out.image_sizes == [ch[0][0]] and out.original == [(97, 131, False)]
    assert np.array_equal(out.tensors.cpu().numpy(), dc.batch_ref([img], ch, fmt, mean, std, 32))


def test_device_resize_matches_pil_fixtures_and_skips_an_unchanged_axis(lib, golden):
    """The committed PIL results on the device: with format "rgb255", mean 0 and std 1 the output IS the resized byte (fl(fl(v / 255) 255)
    = v), padded to the batch.  Then sizes Resize.get_size never returns -- one axis unchanged, the other resized -- through apply(): Pillow
    skips that pass, so the result equals PIL's (checked live on the host by the restatement's own tests)."""
    from fiber_amd import data
    assert [lib.plain("fiber_resample_ksize_bilinear", a, b) for a, b in ((131, 64), (30, 64), (64, 64))] == [7, 3, 3]      # Pillow's window lengths
    t = data.DeviceDetectionTransform(dc.input_cfg(fmt="rgb255", mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), divisible=0), is_train=False)
    names = list(dc.RESIZE_CASES)
    imgs = [dc.case_image(n) for n in names]
    sizes = [dc.RESIZE_CASES[n][2:] for n in names]
    got = t.apply([torch.from_numpy(im).to(DEV) for im in imgs], sizes, [False] * len(names)).tensors.cpu().numpy()
    assert got.shape == (len(names), 3, 97, 113)                    # divisibility 0: the plain maximum, odd widths (scalar stores)
    for b, n in enumerate(names):
        oh, ow = sizes[b]
        want = np.zeros((3, 97, 113), np.float32)
        want[:, :oh, :ow] = np.transpose(golden(n)["resized"], (2, 0, 1))
        assert np.array_equal(got[b], want), n
    img = dc.synth_image(97, 131, 9)
    sizes, flips = [(97, 86), (64, 131), (97, 131)], [True, False, True]
    out = t.apply([torch.from_numpy(img).to(DEV)] * 3, sizes, flips).tensors.cpu().numpy()
    ref = dc.batch_ref([img] * 3, list(zip(sizes, flips)), "rgb255", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0)
    assert np.array_equal(out, ref)


# ---------------------------------------------------------------------------------------------------- boxes
def test_boxes_match_reference_fixture(lib, golden):
    from fiber_amd import data
    gold = golden(dc.BOX_GOLDEN)
    names = list(dc.BOX_CASES)
    G, n = 9, 7                                                      # two padding rows; the last image keeps 4 of its 7 boxes
    boxes = np.full((len(names), G, 4), 123.0, np.float32)           # garbage in the padding rows: the kernel writes them as zero
    num_gt, rows = [], []
    for b, name in enumerate(names):
        (w, h), (nw, nh), flip = dc.BOX_CASES[name]
        boxes[b, :n] = dc.case_boxes(name)
        num_gt.append(4 if b == len(names) - 1 else n)
        rows.append((float(nw) / float(w), float(nh) / float(h), int(flip), float(nw), num_gt[-1]))
    d = torch.from_numpy(boxes).to(DEV)
    table = data._box_table(rows, DEV)
    lib.call("fiber_det_boxes_f32", lib.ptr(d), lib.ptr(table), len(names), G)
    got = d.cpu().numpy()
    for b, name in enumerate(names):
        k = num_gt[b]
        assert np.array_equal(got[b, :k], gold[name][:k]), name
        orig, new, flip = dc.BOX_CASES[name]
        assert np.array_equal(got[b, :k], dc.boxes_ref(dc.case_boxes(name), orig, new, flip)[:k]), name
        assert not got[b, k:].any(), name


def test_boxes_to_original(lib):
    from fiber_amd import data
    il = data.DetImageList(None, [(64, 86), (80, 113)], [(97, 131, False), (33, 47, False)])
    g = np.random.default_rng(2)
    boxes = np.stack([g.uniform(0, 60, (5, 4)), g.uniform(0, 75, (5, 4))]).astype(np.float32)
    got = il.boxes_to_original(torch.from_numpy(boxes).to(DEV)).cpu().numpy()
    assert np.array_equal(got[0], dc.boxes_ref(boxes[0], (86, 64), (131, 97), False))
    assert np.array_equal(got[1], dc.boxes_ref(boxes[1], (113, 80), (47, 33), False))


# ---------------------------------------------------------------------------------------------------- the bicubic neighbour
def test_bicubic_transform_unchanged(lib):
    """DeviceImageTransform after coeff_row / fiber_resample_ksize were generalised over the filter: still bit-equal to the oracle (this
    test uses nothing the generalisation added, so it also passes on the tree before it)"""
    from fiber_amd import data
    from oracle import image_ref as R
    shapes = [(97, 131), (20, 30), (150, 40), (100, 64), (64, 64)]
    host = [dc.synth_image(H, W, seed=H * 1000 + W) for H, W in shapes]
    out = data.DeviceImageTransform(64)([torch.from_numpy(im).to(DEV) for im in host]).cpu().numpy()
    for i, im in enumerate(host):
        assert np.array_equal(out[i], R.albef_transform(im, 64)), (i, im.shape)
    assert [lib.plain("fiber_resample_ksize", a, b) for a, b in ((131, 64), (30, 64), (64, 64))] == [11, 5, 5]


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def pipeline(lib):
    from fiber_amd.modules import GeneralizedVLRCNN
    torch.manual_seed(0)
    cfg = dc.input_cfg(fc.model_cfg(), min_size=(64,), max_size=96)
    model = GeneralizedVLRCNN(cfg).to(DEV)
    g = np.random.default_rng(0)
    shapes = [(120, 160), (150, 100)]
    T = 256
    pm = [np.zeros((2, T), np.uint8), np.zeros((1, T), np.uint8)]
    pm[0][0, 1:3], pm[0][1, 4], pm[1][0, 2:5] = 1, 1, 1
    samples = [
        {"image": torch.from_numpy(g.integers(0, 256, (120, 160, 3), dtype=np.uint8)).to(DEV),
         "boxes": torch.tensor([[10.0, 8.0, 120.0, 100.0], [60.0, 30.0, 150.0, 110.0]]), "labels": torch.tensor([1, 2]),
         "positive_map": torch.from_numpy(pm[0]), "input_ids": torch.tensor([0] + list(range(100, 107)) + [2])},
        {"image": torch.from_numpy(g.integers(0, 256, (150, 100, 3), dtype=np.uint8)).to(DEV),
         "boxes": torch.tensor([[5.0, 20.0, 90.0, 140.0]]), "labels": torch.tensor([1]),
         "positive_map": torch.from_numpy(pm[1]), "input_ids": torch.tensor([0] + list(range(200, 212)) + [2])},
    ]
    return model, cfg, samples, shapes


def test_collate_into_a_training_step(pipeline):
    from fiber_amd import data
    model, cfg, samples, shapes = pipeline
    t = data.DeviceDetectionTransform(cfg, is_train=True)
    seed = next(s for s in range(1, 100) if [c[1] for c in dc.choices_ref(s, shapes, (64,), 96, 0.5)] == [True, False])
    images, targets, tok = data.device_collate_grounding(samples, t, cfg, seed)
    again = data.device_collate_grounding(samples, t, cfg, seed)
    assert torch.equal(images.tensors, again[0].tensors) and torch.equal(targets.boxes, again[1].boxes)          # one seed: bitwise equal
    assert torch.equal(tok["input_ids"], again[2]["input_ids"]) and torch.equal(targets.positive_map, again[1].positive_map)
    assert images.image_sizes == [(64, 85), (96, 64)] and tuple(images.tensors.shape) == (2, 3, 96, 96)
    assert images.original == [(120, 160, True), (150, 100, False)]
    assert tok["input_ids"].shape == (2, 256) and tok["attention_mask"].sum(1).tolist() == [9, 14]
    want = np.zeros((2, 2, 4), np.float32)
    want[0] = dc.boxes_ref(samples[0]["boxes"].numpy(), (160, 120), (85, 64), True)
    want[1, :1] = dc.boxes_ref(samples[1]["boxes"].numpy(), (100, 150), (64, 96), False)
    assert np.array_equal(targets.boxes.cpu().numpy(), want) and targets.num_gt.tolist() == [2, 1]
    model.train()
    model.zero_grad(set_to_none=True)
    losses = model(images, targets=targets, tokenizer_input=tok)
    assert set(losses) == {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(losses.values()).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(gr).all()) for gr in grads)


def test_collate_into_eval_and_back_to_the_original_frame(pipeline):
    from fiber_amd import data
    from fiber_amd.modules import Detections
    model, cfg, samples, shapes = pipeline
    t = data.DeviceDetectionTransform(cfg, is_train=False)
    images, _, tok = data.device_collate_grounding(samples, t, cfg, 3)
    assert images.original == [(120, 160, False), (150, 100, False)]
    model.eval()
    with torch.no_grad():
        det = model(images, positive_map={1: [1, 2], 2: [4], 3: 7}, tokenizer_input=tok)
    assert isinstance(det, Detections)
    back = images.boxes_to_original(det)
    assert back.shape == det.boxes.shape and back.dtype == torch.float32
    count, boxes, resized = det.count.cpu().tolist(), back.cpu().numpy(), det.boxes.cpu().numpy()
    for b, (H, W) in enumerate(shapes):
        k = count[b]
        oh, ow = images.image_sizes[b]
        assert np.array_equal(boxes[b], dc.boxes_ref(resized[b], (ow, oh), (W, H), False))
        assert (boxes[b, :k, 0::2] >= 0).all() and (boxes[b, :k, 0::2] <= W).all(), b
        assert (boxes[b, :k, 1::2] >= 0).all() and (boxes[b, :k, 1::2] <= H).all(), b
