"""CPU: the fp64 restatement of tests/fpn_cases.py against the reference-run fixture tests/golden/fpn_neck.npz and against mutations of itself,
the nearest index rule against F.interpolate, and the construction, checkpoint keys and refusals of modules/fpn.py and
modules/grounding_model.py.  (The kernels themselves are tested on the GPU: tests/test_hip_fpn.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_cases as fc


def _weights(gold):
    return {k[2:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("w.")}


def _seeds(gold):
    return [gold["draw.s16"], gold["draw.s8"]]


def test_restatement_agrees_with_the_reference_fixture(golden):
    """fp64 against the reference's fp32: eval, train (replaying the recorded draws) and the gradients of the linear loss, to fp32 accuracy"""
    gold = golden(fc.GOLDEN)
    maps, proj = fc.neck_inputs()
    with torch.no_grad():
        for n, o in zip(fc.OUT_NAMES, fc.neck_ref(_weights(gold), maps)):
            assert tuple(o.shape) == gold["eval." + n].shape
            assert fc.rel_l2(o, gold["eval." + n]) < 2e-6, n
    wg = {k: v.double().requires_grad_(True) for k, v in _weights(gold).items()}
    xs = [m.double().requires_grad_(True) for m in maps]
    tr = fc.neck_ref(wg, xs, train_seeds=_seeds(gold))
    sum((o * p.double()).sum() for o, p in zip(tr, proj)).backward()
    for n, o in zip(fc.OUT_NAMES, tr):
        assert fc.rel_l2(o.detach(), gold["train." + n]) < 2e-6, n
    assert xs[0].grad is None                                # the stride-4 map is never read
    for i, x in enumerate(xs[1:]):
        assert fc.rel_l2(x.grad, gold[f"grad.x{i + 3}"]) < 1e-5, i
    for k, v in wg.items():
        assert fc.rel_l2(v.grad, gold["grad." + k]) < 1e-5, k
    assert set(wg) == set(fc.WEIGHT_KEYS)
    assert all(gold["draw." + s].sum() > 0 for s in ("s16", "s8"))           # the train-mode fixture does drop blocks


def test_bf16_restatement_distances_are_the_recorded_ones(golden):
    """fpn_cases.BF16_DISTANCE (from which the GPU tolerances follow) is what the bf16-rounding restatement measures against the fixture"""
    gold = golden(fc.GOLDEN)
    maps, proj = fc.neck_inputs()
    got = {}
    with torch.no_grad():
        for n, o in zip(fc.OUT_NAMES, fc.neck_ref(_weights(gold), maps, bf16=True)):
            got["eval." + n] = fc.rel_l2(o, gold["eval." + n])
    wg = {k: v.double().requires_grad_(True) for k, v in _weights(gold).items()}
    xs = [m.double().requires_grad_(True) for m in maps]
    tr = fc.neck_ref(wg, xs, train_seeds=_seeds(gold), bf16=True)
    sum((o * p.double()).sum() for o, p in zip(tr, proj)).backward()
    for n, o in zip(fc.OUT_NAMES, tr):
        got["train." + n] = fc.rel_l2(o.detach(), gold["train." + n])
    for i, x in enumerate(xs[1:]):
        got[f"grad.x{i + 3}"] = fc.rel_l2(x.grad, gold[f"grad.x{i + 3}"])
    for k, v in wg.items():
        got["grad." + k] = fc.rel_l2(v.grad, gold["grad." + k])
    assert set(got) == set(fc.BF16_DISTANCE)
    for k, v in got.items():
        assert abs(v - fc.BF16_DISTANCE[k]) <= 1e-3 * fc.BF16_DISTANCE[k] + 1e-7, (k, v, fc.BF16_DISTANCE[k])


@pytest.mark.parametrize("mutate,outs", [("drop_top", ("p5", "p6", "p7")), ("p6_from_c5", ("p6", "p7")), ("int_index", ())])
def test_module_mutations_leave_the_fixture(golden, mutate, outs):
    """The wiring's quirks are visible in the fixture: a restatement that drops the top level, or reads P6 from C5's lateral instead of
    P5, is far outside the GPU tolerance on exactly the levels it touches; the integer index rule does not show at these sizes (that is
    what the (58, 30) kernel case is for)."""
    gold = golden(fc.GOLDEN)
    maps, _ = fc.neck_inputs()
    with torch.no_grad():
        tr = fc.neck_ref(_weights(gold), maps, train_seeds=_seeds(gold), mutate=mutate)
    for n, o in zip(fc.OUT_NAMES, tr):
        d = fc.rel_l2(o, gold["train." + n])
        if n in outs:
            assert d > 10 * fc.gpu_tolerance("train." + n), (n, d)
        else:
            assert d < 2e-6, (n, d)


@pytest.mark.parametrize("with_keep", [False, True])
def test_integer_index_rule_breaks_the_bounds_at_58_30(with_keep):
    x = fc.merge_inputs("f32_rule", with_keep)
    assert not np.array_equal(fc.src_index(58, 30), fc.src_index_integer(58, 30))
    ref, mut = fc.merge_fwd_ref(x), fc.merge_fwd_ref(x, index=fc.src_index_integer)
    for k in ref:
        assert (np.abs(mut[k][0] - ref[k][0]) > ref[k][1]).any(), k
    rb = fc.merge_bwd_ref(x, use_dropped=with_keep)
    mb = fc.merge_bwd_ref(x, use_dropped=with_keep, index=fc.src_index_integer)
    assert (np.abs(mb["d_coarse"][0] - rb["d_coarse"][0]) > rb["d_coarse"][1]).any()
    # ... and at the other cases' sizes the two rules agree, so only this case can tell them apart
    for name, (_, H, W, Hc, Wc, _) in fc.MERGE_CASES.items():
        if name != "f32_rule":
            assert np.array_equal(fc.src_index(H, Hc), fc.src_index_integer(H, Hc)) and np.array_equal(fc.src_index(W, Wc), fc.src_index_integer(W, Wc))


@pytest.mark.parametrize("name", list(fc.MERGE_CASES))
def test_scale_from_the_rounded_sum_breaks_the_bounds(name):
    x = fc.merge_inputs(name, True)
    ref, mut = fc.merge_fwd_ref(x), fc.merge_fwd_ref(x, scale_from_rounded=True)
    # what such a kernel would store: the bf16 rounding of the mutated value
    stored = torch.from_numpy(mut["dropped"][0]).to(torch.bfloat16).double().numpy()
    assert (np.abs(stored - ref["dropped"][0]) > ref["dropped"][1]).any()
    assert not (np.abs(torch.from_numpy(ref["dropped"][0]).to(torch.bfloat16).double().numpy() - ref["dropped"][0]) > ref["dropped"][1]).any()


def test_children_counts_of_the_merge_cases():
    """The case table's claims: 2 and 4 children at (5, 6) -> (3, 3), 1, 2 and 4 at (5, 5) -> (3, 3); 16 at (4, 4) -> (1, 1); one each
    at equal sizes"""
    def counts(name):
        _, H, W, Hc, Wc, _ = fc.MERGE_CASES[name]
        n = np.zeros((Hc, Wc), dtype=int)
        for h in fc.src_index(H, Hc):
            for w in fc.src_index(W, Wc):
                n[h, w] += 1
        return set(n.reshape(-1).tolist())
    assert counts("odd_2_4") == {2, 4}
    assert counts("odd_1_2_4") == {1, 2, 4}
    assert counts("sixteen") == {16}
    assert counts("same_size") == {1}


def test_index_rule_equals_interpolate_below_700():
    """The restated fp32 rule is F.interpolate(mode="nearest", size=...) for every H < 700 and Hc in {H // 2, (H + 1) // 2, (H + 2) // 2}
    (and Hc = H); the exact rational is not."""
    differs = []
    for H in range(1, 700):
        for Hc in sorted({H // 2, (H + 1) // 2, (H + 2) // 2, H}):
            if Hc < 1:
                continue
            want = F.interpolate(torch.arange(Hc, dtype=torch.float32).view(1, 1, Hc, 1), size=(H, 1), mode="nearest").view(-1).long().numpy()
            assert np.array_equal(fc.src_index(H, Hc), want), (H, Hc)
            if not np.array_equal(fc.src_index_integer(H, Hc), want):
                differs.append((H, Hc))
    assert differs[0] == (58, 30) and (194, 98) in differs and (198, 100) in differs


def test_mask_restatement_is_the_reference_block_mask():
    g = np.random.default_rng(0)
    for block in fc.MASK_BLOCKS:
        for shape in fc.MASK_SHAPES:
            seeds = (g.random(shape) < 0.1).astype(np.uint8)
            keep, kept = fc.mask_ref(seeds, block)
            bm = 1 - F.max_pool2d(torch.from_numpy(seeds).float()[:, None], kernel_size=(block, block), stride=(1, 1), padding=block // 2).squeeze(1)
            assert np.array_equal(keep, bm.numpy().astype(np.uint8)) and kept == int(bm.sum())
    s = fc.hash_seeds(fc.MASK_SEED, (2, 25, 33), fc.DROP_PROB / 9)
    assert 20 < int(s.sum()) < 100                           # 1650 draws at 1 / 30


# ---- modules -----------------------------------------------------------------------------------------------------------------------------
def test_fpn_module_keys_shapes_and_init(golden):
    from fiber_amd.modules.fpn import FPN, DropBlock2D, LastLevelP6P7, build_swint_fpn
    gold = golden(fc.GOLDEN)
    torch.manual_seed(0)
    neck = build_swint_fpn(fc.neck_cfg())
    assert isinstance(neck, FPN) and isinstance(neck.top_blocks, LastLevelP6P7) and isinstance(neck.drop_block, DropBlock2D)
    sd = neck.state_dict()
    assert tuple(sd) == fc.WEIGHT_KEYS
    for k, v in sd.items():
        assert tuple(v.shape) == gold["w." + k].shape, k     # nn.Conv2d-shaped, as the reference's
    assert neck.top_blocks.use_P5
    for k, v in sd.items():
        if k.endswith(".bias"):
            assert not v.any()
        else:                                                # kaiming_uniform_(a=1): U(-b, b), b = sqrt(3 / fan_in)
            b = (3.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
            assert float(v.abs().max()) <= b and float(v.abs().max()) > 0.8 * b, k
    neck.load_state_dict(_weights(gold))
    assert build_swint_fpn(fc.neck_cfg(DROP_BLOCK=False)).drop_block is None


@pytest.mark.parametrize("key", ["USE_GN", "USE_RELU", "USE_DYRELU", "USE_SPP", "USE_PAN", "USE_DYHEAD", "RETURN_SWINT_FEATURE_BEFORE_FUSION"])
def test_fpn_unsupported_options_raise(key):
    from fiber_amd.modules.fpn import build_swint_fpn
    with pytest.raises(NotImplementedError, match=key):
        build_swint_fpn(fc.neck_cfg(**{key: True}))


def test_fpn_even_drop_size_raises():
    from fiber_amd.modules.fpn import build_swint_fpn
    with pytest.raises(NotImplementedError, match="DROP_SIZE"):
        build_swint_fpn(fc.neck_cfg(DROP_SIZE=4))


def _reference_fpn_keys():
    """The key list the reference's module names give for the RETINANET wiring: fpn.py:40-53 registers fpn_inner{idx} / fpn_layer{idx}
    for every non-zero entry of in_channels_list = [0, C3, C4, C5] (idx from 1), LastLevelP6P7 registers p6 / p7 under top_blocks"""
    keys = []
    for idx, c in enumerate([0, 1, 1, 1], 1):
        if c:
            keys += [f"fpn_inner{idx}.weight", f"fpn_inner{idx}.bias", f"fpn_layer{idx}.weight", f"fpn_layer{idx}.bias"]
    return keys + [f"top_blocks.p{i}.{p}" for i in (6, 7) for p in ("weight", "bias")]


@pytest.fixture(scope="module")
def model():
    from fiber_amd.modules import GeneralizedVLRCNN
    torch.manual_seed(0)
    return GeneralizedVLRCNN(fc.model_cfg())


def test_detector_state_dict_keys(model):
    from fiber_amd.modules import VLDyHeadModule
    from fiber_amd.modules.fusion_swin import FusionSwinTransformer
    keys = set(model.state_dict())
    bare = FusionSwinTransformer(depths=(2, 2, 2, 2), drop_path_rate=0.0)
    want = {"fusion_backbone." + k for k in bare.state_dict()}                  # backbone.body.* and language_backbone.body.model.*
    want |= {"fusion_backbone.backbone.fpn." + k for k in _reference_fpn_keys()}
    want |= {"rpn." + k for k in VLDyHeadModule(fc.model_cfg()).state_dict()}   # rpn.head.*
    assert keys == want, (sorted(keys - want)[:5], sorted(want - keys)[:5])
    for prefix in ("fusion_backbone.backbone.body.", "fusion_backbone.backbone.fpn.", "fusion_backbone.language_backbone.body.model.", "rpn.head."):
        assert any(k.startswith(prefix) for k in keys), prefix
    assert all(k.startswith(("fusion_backbone.backbone.body.", "fusion_backbone.backbone.fpn.", "fusion_backbone.language_backbone.body.model.",
                             "rpn.head.")) for k in keys)
    assert model.state_dict()["fusion_backbone.backbone.fpn.fpn_inner2.weight"].shape == (256, 256, 1, 1)
    assert model.state_dict()["fusion_backbone.backbone.fpn.fpn_inner4.weight"].shape == (256, 1024, 1, 1)


def test_detector_freezing_rules(model):
    from fiber_amd.modules import GeneralizedVLRCNN
    model.train()
    assert not any(p.requires_grad for p in model.rpn.head.cls_logits.parameters())      # USE_DOT_PRODUCT_TOKEN_LOSS
    assert not model.rpn.head.cls_logits.training and model.fusion_backbone.backbone.fpn.training
    assert all(p.requires_grad for p in model.fusion_backbone.backbone.fpn.parameters())
    cfg = fc.model_cfg(**{"MODEL.BACKBONE.FREEZE": True, "MODEL.FPN.FREEZE": True, "MODEL.RPN.FREEZE": True, "MODEL.LANGUAGE_BACKBONE.FREEZE": True})
    m = GeneralizedVLRCNN(cfg)
    assert not any(p.requires_grad for p in m.fusion_backbone.language_backbone.parameters())     # frozen at construction (:147-151)
    assert all(p.requires_grad for p in m.fusion_backbone.backbone.fpn.parameters())              # ... the others by train()
    m.train()
    assert not any(p.requires_grad for p in m.parameters())
    fb = m.fusion_backbone
    assert not (fb.backbone.body.training or fb.backbone.fpn.training or fb.language_backbone.training or m.rpn.head.training)
    assert m.training and m.rpn.training


@pytest.mark.parametrize("path,value,match", [
    ("MODEL.SWINT.VERSION", "v2", "SWINT.VERSION"), ("MODEL.BACKBONE.FUSION_VERSION", "v1", "FUSION_VERSION"),
    ("MODEL.RPN_ONLY", False, "RPN_ONLY"), ("MODEL.RPN_ARCHITECTURE", "RPN", "RPN_ARCHITECTURE"),
    ("MODEL.DYHEAD.FUSE_CONFIG.MLM_LOSS", True, "MLM_LOSS"), ("MODEL.FPN.USE_PAN", True, "USE_PAN"),
    ("MODEL.FPN.DROP_SIZE", 2, "DROP_SIZE"), ("MODEL.BACKBONE.CONV_BODY", "SWINT-FPN", "CONV_BODY")])
def test_detector_unsupported_options_raise(path, value, match):
    from fiber_amd.modules import GeneralizedVLRCNN
    with pytest.raises(NotImplementedError, match=match):
        GeneralizedVLRCNN(fc.model_cfg(**{path: value}))


def test_detector_needs_targets_and_text(model):
    model.train()
    with pytest.raises(ValueError, match="targets"):
        model(torch.zeros(1, 3, 64, 96), tokenizer_input={})
    model.eval()
    with pytest.raises(ValueError, match="tokenizer"):
        model(torch.zeros(1, 3, 64, 96), captions=["a cat"])
    with pytest.raises(ValueError, match="tokenizer_input"):
        model(torch.zeros(1, 3, 64, 96))
