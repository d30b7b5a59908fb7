"""Host-side pieces of CIDEr-optimised caption training (caption_cider) that need no GPU: the CIDEr-D scorer against the reference's recorded
scores, the df pickle, the torch restatements behind ops.sample_rows / ops.seq_logprob, the model wiring, and compute_caption_cider itself.

The product model has no CPU path (its ops are HIP only), so the objective runs here on a small plain-torch captioner with the attributes it
needs (infer_caption, mlm_score, the metrics, a tokenizer, a scorer); the comparison of the loss terms with the reference model's
(tests/golden/caption_cider_*.npz) is in tests/test_hip_caption_cider.py.  What the reference's objective does on the host -- decode, strip,
wrap, score -- is compared here: the recorded CIDEr-D scores of the sampled captions."""
import copy
import pickle
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cases
from tests import caption_cider_cases as ccc


# ------------------------------------------------------------------------------------------------------------------------ the scorer
@pytest.mark.parametrize("mode", ["corpus", "table"])
def test_scorer_matches_reference(mode, golden, tmp_path):
    """Both sides are fp64 evaluations of the same formula: 1e-12 absolute."""
    from fiber_amd.modules.cider import CiderD
    gold = golden("caption_cider_scorer")
    df = "corpus" if mode == "corpus" else ccc.write_df_table(tmp_path / "df.p", ccc.scorer_df_table())
    scorer = CiderD(df=df)
    for i, (gts, res) in enumerate(ccc.SCORER_SETS):
        mean, scores = scorer.compute_score(gts, res)
        ref = gold[f"{mode}/{i}/scores"]
        assert isinstance(scores, np.ndarray) and scores.shape == ref.shape
        assert np.abs(scores - ref).max() <= 1e-12, (mode, i, scores, ref)
        assert abs(mean - float(gold[f"{mode}/{i}/mean"])) <= 1e-12
    assert float(gold[f"{mode}/0/scores"].max()) > 1.0                      # (the sets do score)


def test_df_pickle_round_trip(tmp_path):
    from fiber_amd.modules.cider import CiderD
    table = {"ref_len": 7, "document_frequency": {("a",): 3.0, ("a", "dog"): 2.0, ("<eos>",): 7.0}}   # a plain dict: unseen n-grams count as 1
    with open(tmp_path / "t.p", "wb") as f:
        pickle.dump(table, f, protocol=2)
    s = CiderD(df=str(tmp_path / "t.p"))
    assert s.ref_len == pytest.approx(np.log(7.0), abs=0) and s.document_frequency == table["document_frequency"]
    gts, res = {0: ["a dog runs <eos>"]}, [{"image_id": 0, "caption": ["a dog <eos>"]}]
    mean, scores = s.compute_score(gts, res)
    assert scores.shape == (1,) and 0.0 < scores[0] < 10.0 and mean == scores[0]
    assert s.compute_score({0: ["a dog <eos>"]}, res)[1][0] == pytest.approx(7.5, abs=1e-12)     # identical, but three words have no 4-gram
    same = s.compute_score(gts, [{"image_id": 0, "caption": ["a dog runs <eos>"]}])[1][0]
    assert same == pytest.approx(10.0, abs=1e-12)                           # identical: cosine 1 for every n
    assert s.compute_score({0: ["cat"]}, [{"image_id": 0, "caption": ["zebra"]}])[1][0] == 0.0


@pytest.mark.parametrize("name", list(ccc.CIDER_CASES))
def test_sampled_caption_scores_match_reference(name, golden, tmp_path):
    """decode / strip / _wrap_sentence / CIDEr-D of the cases' sampled captions against what the reference's objective scored."""
    from fiber_amd.modules import objectives
    from fiber_amd.modules.cider import CiderD
    gold = golden(name)
    pc, c = ccc.CIDER_CASES[name], ccc.full_config(name)
    scorer = CiderD(df=ccc.write_df_table(tmp_path / "df.p", ccc.df_table(name)))
    ids = torch.from_numpy(ccc.sampled_ids(name))
    assert tuple(ids.shape) == (pc["B"] * pc["beam"], c["max_text_len"])
    scores = objectives._caption_cider_scores(scorer, ccc.StubTokenizer(c["vocab_size"]), ids, ccc.gt_txt(name), pc["beam"])
    assert np.abs(scores - gold["cider"]).max() <= 1e-12, (scores, gold["cider"])
    assert 0.0 < gold["cider"].min() and gold["cider"].max() < 10.0 and gold["cider"].max() - gold["cider"].min() > 2.0


# ------------------------------------------------------------------------------------------------ the torch restatements of the two ops
def _np_hash_u32(seed, idx):
    from tests import ew_cases as ec
    return ec.hash_u32(seed, idx)


def test_sample_rows_host_restatement():
    from fiber_amd import ops
    rows, K, V, key = 6, 3, 19, 0x1234
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((rows, V)).astype(np.float32)) * 2
    tok, logp, ended = ops.sample_rows(x, K, V - 1, key=key, pad_id=1, sep_id=2)
    idx = (np.arange(rows * K, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None]).reshape(rows, K, V)
    u = (_np_hash_u32(key, idx).astype(np.float64) + 0.5) * 2.0 ** -32
    z = x.double().numpy().copy()
    z[:, V - 1] = -10000.0
    want = (z[:, None, :] - np.log(-np.log(u))).argmax(-1)
    assert tok.dtype == torch.int64 and np.array_equal(tok.numpy(), want)
    lse = np.log(np.exp(z).sum(1))
    assert np.abs(logp.numpy() - (np.take_along_axis(z, want, 1) - lse[:, None])).max() < 1e-5
    assert not bool((tok == V - 1).any())
    assert torch.equal(ended.bool(), (tok == 1) | (tok == 2))
    tok2, _, _ = ops.sample_rows(x, K, V - 1, key=key)
    tok3, _, _ = ops.sample_rows(x, K, V - 1, key=key + 1)
    assert torch.equal(tok, tok2) and not torch.equal(tok, tok3)
    e = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.bool)
    tok4, logp4, end4 = ops.sample_rows(x, K, V - 1, key=key, ended=e)
    assert bool((tok4[e] == 1).all()) and bool((logp4[e] == 0).all()) and bool((end4[e] == 1).all())
    assert torch.equal(tok4[~e], tok[~e])


def test_seq_logprob_host_restatement():
    from fiber_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(8, 23, generator=g) * 3).requires_grad_(True)
    lab = torch.tensor([4, 1, 22, 0, 1, 1, 7, 9])
    with torch.no_grad():
        x[2, 22] = x[2].max() - 30.0                                        # p ~ 1e-13 << 1e-9
    lp = ops.seq_logprob(x, lab, 1)
    xr = x.detach().double().requires_grad_(True)
    ref = torch.log(F.softmax(xr, -1) + 1e-9).gather(1, lab[:, None])[:, 0]
    ref = torch.where(lab == 1, torch.zeros_like(ref), ref)
    assert torch.allclose(lp.double(), ref, atol=1e-5) and bool((lp[lab == 1] == 0).all())
    assert abs(lp[2].item() - np.log(1e-9)) < 1e-3
    w = torch.arange(1.0, 9.0)
    (lp * w).sum().backward()
    (ref * w.double()).sum().backward()
    assert torch.allclose(x.grad.double(), xr.grad, atol=1e-6) and bool((x.grad[lab == 1] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------- model wiring
def _model(base, **over):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    torch.manual_seed(0)
    return FIBERTransformerSS(make_config(**dict(base, **over)))


def test_caption_cider_model_constructs(tmp_path):
    from fiber_amd.modules.cider import CiderD
    m = _model(cases.TINY, loss_names={"caption_cider": 1}, cider_path="corpus")
    assert isinstance(m.cider_scorer, CiderD) and m.cider_scorer.df_mode == "corpus"
    mle = _model(cases.TINY, loss_names={"caption_mle": 1})
    assert sorted(m.state_dict()) == sorted(mle.state_dict())
    assert m.unused_parameter_names() == mle.unused_parameter_names()
    for ph in ("train", "val"):
        assert hasattr(m, f"{ph}_caption_cider_loss") and hasattr(m, f"{ph}_caption_cider_accuracy")
    path = ccc.write_df_table(tmp_path / "df.p", ccc.df_table("caption_cider_tiny"))
    assert _model(cases.TINY, loss_names={"caption_cider": 1}, cider_path=path).cider_scorer.ref_len == pytest.approx(np.log(50.0))
    with pytest.raises(NotImplementedError):                               # no document-frequency table named: refused, not guessed
        _model(cases.TINY, loss_names={"caption_cider": 1})
    with pytest.raises(NotImplementedError):
        _model(cases.TINY, loss_names={"caption_gold": 1})


@pytest.mark.parametrize("name", list(ccc.CIDER_CASES))
def test_unused_list_matches_reference(name, golden):
    m = _model(ccc.CIDER_CASES[name]["config"], cider_path="corpus")
    assert m.unused_parameter_names() == sorted(golden(name)["unused_params"].tolist())


def test_named_caption_cider_config():
    from fiber_amd.config import named_config
    c = named_config("task_finetune_caption_cider_coco")
    assert c["loss_names"]["caption_cider"] == 1 and sum(c["loss_names"].values()) == 1
    assert (c["exp_name"], c["datasets"], c["batch_size"], c["max_epoch"], c["max_steps"]) == ("finetune_caption_cider_coco", ["coco"], 512, 10, None)
    assert (c["warmup_steps"], c["learning_rate"], c["lr_mult_cross_modal"], c["lr_mult_head"]) == (0.1, 1e-6, 5, 5)
    assert (c["max_text_len"], c["image_size"], c["resolution_before"], c["pretrained_vit"]) == (50, 576, 576, False)
    assert c["cider_path"] == "coco-train-words.p" and c["caption_cider_share_image"] is False
    assert c["train_transform_keys"] == ["albef_randaug"] and c["val_transform_keys"] == ["albef"]


# ------------------------------------------------------------------------------------------- the objective on a plain-torch captioner
V, L, HS, IMG = 41, 10, 16, 8


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.decoder = nn.Linear(HS, V)
        self.last_hidden = None

    def forward(self, x):
        return self.decoder(x)


class _Captioner(nn.Module):
    """An image 'tower' (two tokens per image) and a causal text model (running mean of the embeddings so far, plus the image tokens)."""

    def __init__(self, share=False):
        super().__init__()
        from fiber_amd.modules import fiber_utils
        from fiber_amd.modules.cider import CiderD
        torch.manual_seed(1)
        self.tower = nn.Linear(3 * IMG * IMG, 2 * HS)
        self.emb = nn.Embedding(V, HS)
        self.mix = nn.Linear(HS, HS)
        self.mlm_score = _Head()
        with torch.no_grad():
            self.mlm_score.decoder.weight.mul_(6.0)                       # peaked enough for some beams to end early
        cfg = {"max_text_len": L, "vocab_size": V, "caption_cider_share_image": share, "loss_names": {"caption_cider": 1}}
        self.hparams = types.SimpleNamespace(config=cfg)
        self.cider_scorer = CiderD()
        ccc.attach_tokenizer(self, V)
        fiber_utils.set_metrics(self)
        self.tower_samples = 0

    def log(self, *a, **k):
        pass

    def infer_caption(self, batch, mask_text=False, mask_image=False, image_embeds=None):
        if image_embeds is None:
            img = batch["image"][0]
            self.tower_samples += img.shape[0]
            image_embeds = torch.tanh(self.tower(img.flatten(1))).view(img.shape[0], 2, HS)
        ids = batch["text_ids"]
        e = self.emb(ids)
        run = e.cumsum(1) / torch.arange(1, ids.shape[1] + 1)[None, :, None]
        feats = torch.tanh(self.mix(run + image_embeds.mean(1, keepdim=True)))
        return {"text_feats": feats, "image_embeds": image_embeds, "text_ids": ids, "text_masks": batch["text_masks"]}


def _stub_batch(B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V - 1, (B, L), generator=g)
    ids[:, 0] = 0
    ids[0, 6] = 2
    ids[0, 7:] = 1
    ids[1, L - 1] = 2
    gt = [[" ".join(str(int(t)) for t in ids[s, 1:5]), " ".join(str(int(t)) for t in ids[s, 2:7])] for s in range(B)]
    return {"image": [torch.randn(B, 3, IMG, IMG, generator=g)], "text_ids": ids, "text_labels": None, "text_masks": (ids != 1).long(),
            "gt_txt": gt, "iid": list(range(B))}


def _stub_samples(b, beam):
    rows = []
    for s in range(b["text_ids"].shape[0]):
        for k in range(beam):
            r = b["text_ids"][s].clone()
            if k:
                r[1 + k] = 3 + k
                r[L - 1 - k:] = 1
                r[L - 2 - k] = 2
            rows.append(r)
    out = torch.stack(rows)
    out[beam - 1, 1:] = 1                                                 # one sequence without any non-pad label
    return out


def _reference_terms(m, b, ids, beam):
    """objectives.py:813-877 restated in plain torch on the captioner: (caption_loss, rl_loss)"""
    from fiber_amd.modules import objectives
    bs = b["text_ids"].shape[0]
    o = m.infer_caption({"image": [b["image"][0].repeat_interleave(beam, 0)], "text_ids": ids, "text_masks": ids != 1})
    lab = torch.cat([ids[:, 1:], torch.ones_like(ids[:, :1])], 1)
    pad = lab == 1
    lg = torch.log(F.softmax(m.mlm_score(o["text_feats"]), -1) + 1e-9).gather(-1, lab[..., None])[..., 0]
    lg = lg.masked_fill(pad, 0).sum(-1) / ((~pad).float().sum(-1) + 1e-9)
    scores = objectives._caption_cider_scores(m.cider_scorer, m.trainer.datamodule.dms[0].tokenizer, ids, b["gt_txt"], beam)
    rl = (lg * (100.0 - 100.0 * torch.tensor(scores))).sum() / bs
    o = m.infer_caption(b)
    lab = torch.cat([b["text_ids"][:, 1:], torch.ones_like(b["text_ids"][:, :1])], 1)
    ce = F.cross_entropy(m.mlm_score(o["text_feats"]).view(-1, V), lab.masked_fill(lab == 1, -100).view(-1), ignore_index=-100)
    return ce, rl


def test_objective_terms_against_plain_torch():
    from fiber_amd.modules import objectives
    m, b, beam = _Captioner().train(), _stub_batch(), 3
    ids = _stub_samples(b, beam)
    ret = objectives.compute_caption_cider(m, b, beam_size=beam, alpha=0.3, sampled_ids=ids)
    assert set(ret) == {"caption_cider_loss", "caption_cider_logits", "caption_cider_labels", "caption_cider_ids"}
    ce, rl = _reference_terms(m, b, ids, beam)
    assert torch.isfinite(ret["caption_cider_loss"])                      # the all-pad sequence adds 0, not NaN
    assert ret["caption_cider_loss"].item() == pytest.approx((0.3 * ce + 0.7 * rl).item(), rel=1e-5)
    assert abs(rl.item()) > 1.0
    m.eval()
    ev = objectives.compute_caption_cider(m, b, beam_size=beam, alpha=0.3, sampled_ids=ids)
    assert ev["caption_cider_loss"].item() == pytest.approx(0.3 * ce.item(), rel=1e-6)
    assert torch.equal(ev["caption_cider_labels"][0, :6], b["text_ids"][0, 1:7]) and bool((ev["caption_cider_labels"][0, 6:] == -100).all())


def test_free_running_sampling_ends_and_leaves_the_batch_alone():
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    m, b = _Captioner().train(), _stub_batch()
    keep = copy.deepcopy(b)
    ops.manual_seed(7)
    seen = []
    inner = objectives._caption_sample
    try:
        objectives._caption_sample = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]
        ret = objectives.compute_caption_cider(m, b, beam_size=3)
    finally:
        objectives._caption_sample = inner
    assert torch.isfinite(ret["caption_cider_loss"])
    ret["caption_cider_loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    ids = seen[0]
    assert tuple(ids.shape) == (6, L) and bool((ids[:, 0] == 0).all()) and not bool((ids == V - 1).any())
    for r in ids.tolist():                                                # after the first sep / pad only pads follow
        end = next((i for i, t in enumerate(r[1:], 1) if t in (1, 2)), L)
        assert all(t == 1 for t in r[end + 1:]), r
    assert set(b) == set(keep)
    for k in b:
        same = torch.equal(b[k], keep[k]) if torch.is_tensor(b[k]) else (torch.equal(b[k][0], keep[k][0]) if k == "image" else b[k] == keep[k])
        assert same, k


def test_share_image_equals_separate_passes():
    from fiber_amd.modules import objectives
    b, beam = _stub_batch(), 3
    ids = _stub_samples(b, beam)
    out = []
    for share in (False, True):
        m = _Captioner(share=share).train()
        loss = objectives.compute_caption_cider(m, b, beam_size=beam, sampled_ids=ids)["caption_cider_loss"]
        loss.backward()
        out.append((loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}, m.tower_samples))
    assert out[0][2] == 2 * beam + 2 and out[1][2] == 2                   # tower samples: beam + 1 per image against 1 (sampling pinned)
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-5)
    for n, g in out[0][1].items():
        assert torch.allclose(out[1][1][n], g, rtol=1e-5, atol=1e-5 * float(g.abs().max())), n
