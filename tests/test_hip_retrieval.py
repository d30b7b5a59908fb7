"""GPU: the retrieval tally kernel (csrc/retrieval.hip) against the scalar restatement and the reference's recalls, shared-prefix pair
scoring against the fp32 oracle, and the two evaluations end to end on the tiny configuration.

Measured on an MI355X (tiny configuration, 3 images x 4 texts, all 12 pairs, |oracle| up to 1.78e-2): largest distance from the fp32
oracle 1.153e-4 for rank_output(infer(img=repeat)["cls_feats"]) and 1.153e-4 for score_pairs at pair_batch 12 and 5 -- the two paths agree
bit for bit on these pairs.  End to end (10 images x 2 captions) the score matrix lies 3.2e-3 (ITM, both schemes) and 8.5e-3 (ITC) rel-L2
from the reference's.  profiles/retrieval_eval.md keeps these next to the timings."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import retrieval_cases as rc
from oracle import detgen, fiber_ref as R
from tests.hip_util import DEV, load_from_oracle, rel_l2

pytestmark = pytest.mark.gpu


# ---- the tally kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_kernel_equals_the_restatement_and_repeats_bit_for_bit(name):
    from fiber_amd import ops
    scores, iids, tiids, ks = rc.torch_inputs(name, DEV)
    if name == "retr_strided":
        assert scores.stride(0) == scores.shape[1] + 9
    first = ops.retrieval_ranks(scores, iids, tiids, ks)
    again = ops.retrieval_ranks(scores, iids, tiids, ks)
    want = rc.restate(scores.cpu().numpy(), iids.cpu().numpy(), tiids.cpu().numpy(), ks)
    for what, got, rep, ref in zip(("rank_tr", "rank_ir", "hits"), first, again, want):
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), ref), (name, what, got.tolist(), ref.tolist())
        assert torch.equal(got, rep), (name, what)


def _recalls(hits, Ni, Nt):
    """hits.float() / N in fp32 on the host, where the division is the correctly rounded one (the device's fp32 division is not)"""
    hits = hits.cpu()
    return torch.cat([hits[0].float() / Nt, hits[1].float() / Ni]).numpy()


@pytest.mark.parametrize("name", list(rc.TIE_FREE))
def test_kernel_recalls_equal_the_reference_bit_for_bit(name, golden):
    from fiber_amd import ops
    scores, iids, tiids, ks = rc.torch_inputs(name, DEV)
    got = _recalls(ops.retrieval_ranks(scores, iids, tiids, ks)[2], *scores.shape)
    ref = golden("retrieval_" + name)["recalls"]
    assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), (got.tolist(), ref.tolist())


@pytest.mark.parametrize("path", ["itc", "itm"])
def test_kernel_on_the_references_score_matrices(path, golden):
    from fiber_amd import ops
    g = golden("retrieval_model")
    scores = torch.from_numpy(g[path + "_scores"]).to(DEV)
    hits = ops.retrieval_ranks(scores, torch.from_numpy(g["iids"]).to(DEV), torch.from_numpy(g[path + "_tiids"]).to(DEV))[2]
    got = _recalls(hits, *scores.shape)
    assert got.tobytes() == g[path + "_recalls"].tobytes(), (got.tolist(), g[path + "_recalls"].tolist())


# ---- shared-prefix pair scoring -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """The tiny model with the oracle's weights, the model case's inputs, and the fp32 oracle's scores of 3 images x 4 texts"""
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    ref = detgen.fill_(R.FiberRef(rc.MODEL_CONFIG).eval())
    model = load_from_oracle(FIBERTransformerSS(make_config(**rc.MODEL_CONFIG)).eval(), ref).to(DEV)
    inp = rc.model_inputs()
    perm = detgen._rng("retrieval:pairs", 0).permutation(12)
    img_idx, txt_idx = torch.from_numpy(perm // 4), torch.from_numpy(perm % 4)       # all 12 pairs, shuffled
    images, ids, masks = inp["images"][:3], inp["text_ids"][:4], inp["text_masks"][:4]
    batch = {"text_ids": ids[txt_idx], "text_masks": masks[txt_idx], "text_labels": torch.full_like(ids[txt_idx], -100)}
    with torch.no_grad():
        cls = ref.infer(batch, img=images[img_idx])["cls_feats"]
        oracle = F.linear(cls, ref.itm_score.fc.weight[1:], ref.itm_score.fc.bias[1:])[:, 0]      # fiber_module.py:112-114
    return dict(model=model, inp=inp, images=images.to(DEV), ids=ids.to(DEV), masks=masks.to(DEV), img_idx=img_idx.to(DEV),
                txt_idx=txt_idx.to(DEV), batch={k: v.to(DEV) for k, v in batch.items()}, oracle=oracle)


def _score_pairs(p, pair_batch):
    m = p["model"]
    with torch.no_grad():
        image_prefix = m.encode_image_prefix(p["images"])
        text_prefix, ext = m.encode_text_prefix(p["ids"], p["masks"])
        out = [m.score_pairs(image_prefix, text_prefix, ext, p["img_idx"][i:i + pair_batch], p["txt_idx"][i:i + pair_batch])
               for i in range(0, 12, pair_batch)]
    return torch.cat(out).cpu()


def _existing(p):
    m = p["model"]
    with torch.no_grad():                                    # the path the parent commit has: a full pass per pair
        return m.rank_score(m.infer(p["batch"], img=p["images"][p["img_idx"]])["cls_feats"]).cpu()


def test_score_pairs_is_as_close_to_the_oracle_as_the_full_pass(pair):
    """Bound: the shared-prefix scores may lie at most 1.25 x as far from the fp32 oracle as infer(img=repeat) does on the same pairs,
    plus 1e-6 (the margin covers GEMM dispatch that differs with the batch size; nothing else differs)."""
    new, old = _score_pairs(pair, 12), _existing(pair)
    assert new.dtype == torch.float32 and new.shape == (12,)
    d_new, d_old = (new - pair["oracle"]).abs().max().item(), (old - pair["oracle"]).abs().max().item()
    print(f"score_pairs: max |new - oracle| {d_new:.3e}, max |infer(img=repeat) - oracle| {d_old:.3e}, |oracle| max "
          f"{pair['oracle'].abs().max().item():.3e}, max |new - old| {(new - old).abs().max().item():.3e}")
    assert d_new <= 1.25 * d_old + 1e-6, (d_new, d_old)


def test_score_pairs_does_not_depend_on_the_batching(pair):
    old = _existing(pair)
    d_old = (old - pair["oracle"]).abs().max().item()
    for pair_batch in (12, 5):
        d = (_score_pairs(pair, pair_batch) - pair["oracle"]).abs().max().item()
        print(f"score_pairs pair_batch {pair_batch}: max distance from the oracle {d:.3e} (full pass {d_old:.3e})")
        assert d <= 1.25 * d_old + 1e-6, (pair_batch, d, d_old)


def test_pair_scoring_is_evaluation_only(pair):
    m = pair["model"]
    m.train()
    try:
        with pytest.raises(ValueError):
            m.encode_image_prefix(pair["images"])
        with pytest.raises(ValueError):
            m.encode_text_prefix(pair["ids"], pair["masks"])
        with pytest.raises(ValueError):
            m.score_pairs(None, None, None, pair["img_idx"], pair["txt_idx"])
    finally:
        m.eval()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _data(inp):
    from fiber_amd.modules.retrieval_eval import pack_retrieval_data
    return pack_retrieval_data(inp["images"], inp["img_index"], inp["text_ids"], inp["text_masks"], inp["text_img_index"],
                               image_batch=inp["image_batch"], text_batch=inp["text_batch"])


def _check_end_to_end(tag, scores, iids, tiids, got, gold, key, caption=None):
    """caption: which caption each column of `scores` is, where that differs from the fixture's columns"""
    ref = torch.from_numpy(gold[key + "_scores"])
    if caption is not None:
        ref = ref[:, np.argsort(gold[key + "_caption"])[caption]]
    e = rel_l2(scores, ref)
    print(f"{tag}: score matrix rel-L2 from the reference's {e:.3e}")
    assert np.array_equal(iids.cpu().numpy(), gold["iids"]) and np.array_equal(tiids.cpu().numpy(), gold[key + "_tiids"])
    assert e <= 2.5e-2, (tag, e)
    hits = rc.restate(scores.cpu().numpy(), iids.cpu().numpy(), tiids.cpu().numpy())[2]
    want = rc.recalls(hits, *scores.shape)
    assert np.array([float(v) for v in got], np.float32).tobytes() == want.tobytes(), (tag, [float(v) for v in got], want.tolist())
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in got)


@pytest.mark.parametrize("shared_prefix", [True, False])
def test_itm_recall_end_to_end(pair, shared_prefix, golden):
    from fiber_amd.modules import retrieval_eval as re_
    m, data = pair["model"], _data(pair["inp"])
    scores, iids, tiids = re_.itm_scores(m, data, pair_batch=7, shared_prefix=shared_prefix, image_batch=3)
    got = re_.compute_itm_recall(m, data, pair_batch=7, shared_prefix=shared_prefix, image_batch=3)
    _check_end_to_end(f"itm shared_prefix={shared_prefix}", scores, iids, tiids, got, golden("retrieval_model"), "itm")


def test_itc_recall_end_to_end(pair, golden):
    from fiber_amd.modules import retrieval_eval as re_
    m, data = pair["model"], _data(pair["inp"])
    scores, iids, tiids = re_.itc_scores(m, data, image_batch=3)
    got = re_.compute_itc_recall(m, data, image_batch=3)
    mine = np.argsort(np.array(pair["inp"]["text_img_index"]), kind="stable")      # the captions of an image keep their order here; the
    _check_end_to_end("itc", scores, iids, tiids, got, golden("retrieval_model"), "itc", caption=mine)   # reference's sort is not stable


def test_validation_epoch_logs_the_recalls(pair):
    """Trainer.validate on a module with get_recall_metric and retrieval_data attached logs recalls/* and val/the_metric"""
    from fiber_amd.modules import retrieval_eval as re_
    from fiber_amd.trainer import Trainer
    m = pair["model"]
    cfg = m.hparams.config
    old = {k: cfg.get(k) for k in ("get_recall_metric", "get_recall_metric_itc")}
    cfg.update(get_recall_metric=True, get_recall_metric_itc=False)
    m.retrieval_data = _data(pair["inp"])
    logits, target = torch.tensor([[0.0, 1.0], [1.0, 0.0]], device=DEV), torch.tensor([1, 1], device=DEV)
    for metric in (m.val_itm_accuracy, m.val_itc_i2t_accuracy, m.val_itc_t2i_accuracy):       # an empty loader: the running accuracies
        metric(logits, target)                                                                # get one batch by hand (1 of 2 right)
    try:
        value = Trainer().validate(m, [])
        want = re_.compute_itm_recall(m, m.retrieval_data)
    finally:
        cfg.update(old)
        del m.retrieval_data
    for tag, ref in zip(("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10"), want):
        assert torch.equal(m.logged["recalls/" + tag], ref), tag
    assert value == float(want[0] + want[3] + 0.5 + 0.5) and float(m.logged["val/the_metric"]) == value
