"""CPU tests of the grounding head's yardstick and module surface.

1. The fp64 restatement of tests/ground_cases.py reproduces what the REFERENCE's own functions computed (tests/golden/ground_loss_only.npz,
   ground_small*.npz, written by tools/gen_ground_golden.py) to fp32 round-off: 2^-20 * sum |terms| (fp32 against fp64 of one formula).
2. Mutations of a correct result that pass a whole-tensor rel-L2 of 5e-3 are rejected by the per-element bounds the GPU tests use.
3. VLDyHead constructs on the CPU with the reference instance's state-dict keys and shapes; unsupported switches raise."""
import numpy as np
import pytest
import torch

import ground_cases as gc


def test_restatement_reproduces_reference_loss_only(golden):
    gold = golden("ground_loss_only")
    c = gc.loss_only_case()
    rows = gold["rows"]
    for i, (gamma, alpha) in enumerate(gc.LOSS_ONLY_HYPER):
        lg = c["logits"].double().requires_grad_()
        s = lg.clamp(-gc.CLAMP, gc.CLAMP)
        el = gc.focal64(s, c["targets"], c["mask"], alpha, gamma)
        el.sum().backward()
        terms = float(el.detach().abs().sum())
        assert abs(float(el.detach().sum()) - float(gold[f"loss{i}"])) <= gc.HOST * terms, (gamma, alpha)
        ref = torch.from_numpy(gold[f"dlogits{i}"]).double()
        got = lg.grad[:, rows]
        # autograd of the restatement and its closed form agree; both reproduce the reference's autograd
        closed = gc.focal_grad64(s.detach(), c["targets"], c["mask"], alpha, gamma) * (lg.detach().abs() <= gc.CLAMP)
        assert float((closed - lg.grad).abs().max()) <= 1e-12
        # per element: fp32 evaluation of ce, p_t, (1 - p_t)^gamma and their products, a handful of roundings of terms of size <= |s| + 1
        bound = 2.0 ** -20 * (1.0 + gamma) * (s.detach()[:, rows].abs() + 1.0) * gc.alpha_t(c["targets"][:, rows], alpha)
        assert gc.within(got, ref, bound), (gamma, alpha, float(((got - ref).abs() / bound).max()))
    assert float(lg.grad[0, 5, 7]) == 0.0 and float(lg.grad[1, 700, 3]) == 0.0          # beyond the clamp: no gradient
    hole = int(np.flatnonzero(c["mask"][1].numpy() == 0)[0])
    assert float(lg.grad[1, :, hole].abs().max()) == 0.0                                 # masked token


def test_restatement_reproduces_reference_head_logits(golden):
    """The dot product of the reference run (its own tower features and projected tokens, fp32) restated in fp64 on sampled rows."""
    gold, text = golden("ground_small"), golden("ground_small_text")
    ls = torch.tensor([gc.SMALL["log_scale"]])
    s, _, mag = gc.align64(torch.from_numpy(text["q_rows"]), torch.from_numpy(text["proj"]), torch.from_numpy(text["tbias"]), ls)
    ref = torch.from_numpy(gold["dot_rows"]).double()
    assert gc.within(s, ref, gc.HOST * mag + 2.0 ** -22 * ref.abs()), float(((s - ref).abs() / (gc.HOST * mag + 2.0 ** -22 * ref.abs())).max())
    assert gc.within(mag, torch.from_numpy(gold["dot_mag_rows"]).double(), 2.0 ** -20 * mag)


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    c = gc.kernel_case("mutations", 2, 4096)
    c["tbias"][0, 5] = 50000.5                                # a column around the clamp: about half its anchors exceed it by a few units
    alpha, gamma, g = 0.25, 2.0, 0.37
    return c, gc.backward64(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], c["mask"], alpha, gamma, g), (alpha, gamma, g)


def _rejected(name, got, ref, bound):
    assert gc.rel_l2(got, ref) <= 5e-3, f"{name}: the mutation is not subtle ({gc.rel_l2(got, ref):.2e})"
    assert not gc.within(got, ref, bound), f"{name}: the per-element bound accepts the mutation"


def test_correct_results_pass(truth):
    c, r, (alpha, gamma, g) = truth
    assert gc.within(r["s"].float(), r["s"], gc.logit_bound(r["mag"], r["s"]))
    assert gc.within(r["ds"].to(torch.bfloat16), r["ds"], gc.ds_bound(r["ds"], c["targets"], alpha, g))


def test_tile_with_another_images_tokens_is_rejected(truth):
    c, r, _ = truth
    other, _, _ = gc.align64(c["x"][:1, 64:80], c["p"][1:], c["tbias"][:1], c["log_scale"])
    got = r["s"].clone()
    got[0, 64:80, 16:32] = other[0, :, 16:32]
    _rejected("foreign P", got, r["s"], gc.logit_bound(r["mag"], r["s"]))


def test_masked_token_that_contributes_is_rejected(truth):
    c, r, (alpha, gamma, g) = truth
    hole = int(np.flatnonzero(c["mask"][0].numpy() == 0)[0])
    open_mask = c["mask"].clone()
    open_mask[0, hole] = 1
    m = gc.backward64(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], open_mask, alpha, gamma, g)
    got = r["ds"].clone()
    got[0, 128:144, hole] = m["ds"][0, 128:144, hole]        # on one wave's 16 anchors
    _rejected("masked token in ds", got, r["ds"], gc.ds_bound(r["ds"], c["targets"], alpha, g))
    # the loss is one number: a masked token's column moves it by a fraction of a per cent, far outside the reduction bound
    assert abs(float(m["loss"] - r["loss"])) <= 1e-2 * float(r["loss"])
    assert abs(float(m["loss"] - r["loss"])) > gc.CONST["SUM"] * float(r["loss_el"].abs().sum()), "the sum bound accepts a masked token's loss"


def test_absent_clamp_is_rejected(truth):
    c, r, (alpha, gamma, g) = truth
    s, un, mag = gc.align64(c["x"], c["p"], c["tbias"], c["log_scale"])
    unclamped = un + c["tbias"].double()[:, None, :]
    got = r["s"].clone()
    got[0, :, 5] = unclamped[0, :, 5]                        # 50000.5 + dot instead of min(., 50000)
    assert float((got - r["s"]).abs().max()) > 1.0
    _rejected("no clamp", got, r["s"], gc.logit_bound(r["mag"], r["s"]))


def test_swapped_alpha_on_one_row_is_rejected(truth):
    c, r, (alpha, gamma, g) = truth
    got = r["ds"].clone()
    at = gc.alpha_t(c["targets"][1, 300], alpha)
    got[1, 300] = r["ds"][1, 300] * (1.0 - at) / at          # alpha and 1 - alpha exchanged between the classes on one anchor of the short text
    _rejected("alpha_t swapped", got, r["ds"], gc.ds_bound(r["ds"], c["targets"], alpha, g))


# ---- module surface --------------------------------------------------------------------------------------------------------------------
def test_vldyhead_state_dict_matches_reference(golden):
    from fiber_amd.modules import VLDyHead
    gold = golden("ground_small")
    m = VLDyHead(gc.head_cfg(convs=gc.SMALL["convs"]))
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold["state_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold["state_shapes"]]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in gold["param_names"]]


def test_first_dyconv_follows_channel_match():
    from fiber_amd.modules import VLDyHead
    m = VLDyHead(gc.head_cfg(convs=2, in_channels=128))
    assert m.dyhead_tower[0].offset is None and m.dyhead_tower[0].AttnConv is None and isinstance(m.dyhead_tower[0].relu, torch.nn.ReLU)
    assert m.dyhead_tower[1].offset is not None and m.dyhead_tower[1].AttnConv is not None


@pytest.mark.parametrize("switch", ["EARLY_FUSE_ON", "USE_TOKEN_LOSS", "USE_CONTRASTIVE_ALIGN_LOSS", "USE_SHALLOW_CONTRASTIVE_LOSS",
                                    "USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS", "MLM_LOSS"])
def test_unsupported_switches_raise(switch):
    from fiber_amd.modules import VLDyHead
    with pytest.raises(NotImplementedError, match=switch):
        VLDyHead(gc.head_cfg(**{switch: True}))


def test_token_focal_loss_module_signature():
    from fiber_amd.modules import TokenSigmoidFocalLoss
    c = gc.loss_only_case()
    fl = TokenSigmoidFocalLoss(0.25, 2.0)
    s = c["logits"].double().clamp(-gc.CLAMP, gc.CLAMP)
    ref = gc.focal64(s, c["targets"], c["mask"], 0.25, 2.0).sum()
    assert abs(float(fl(s, c["targets"], c["mask"], version="binary")) - float(ref)) <= 1e-9 * float(ref)
    assert float(fl(s[:, :0], c["targets"][:, :0])) == 0.0
    for v in ("softmax", "binaryv2"):
        with pytest.raises(NotImplementedError):
            fl(s, c["targets"], c["mask"], version=v)
