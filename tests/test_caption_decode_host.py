"""Host-side pieces of KV-cached caption decoding that need no GPU: the torch restatements behind ops.mha_decode_self /
ops.mha_decode_cross against the fp64 reference, the ancestry table against a physically reordered cache, the two decoding loops of
objectives.py driven by a plain-torch stepper, the C ABI, and the default (cache off) path.

The product model has no CPU path, so the loops run on a small plain-torch captioner whose text model is trivially cacheable (a running
sum of the embeddings so far), in the style of _Captioner in tests/test_caption_cider_host.py; the model itself is compared with the
reference's record in tests/test_hip_caption_decode.py."""
import os
import re
import types

import pytest
import torch
import torch.nn as nn

from tests import caption_cases as cc
from tests import decode_cases as dc


# ------------------------------------------------------------------------------------------------ the torch restatements of the two ops
@pytest.mark.parametrize("ancestry", [False, True, "masked"])
@pytest.mark.parametrize("t", dc.SELF_T)
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_self_host_restatement(D, t, ancestry):
    """fp64 operands: both sides evaluate the same formula in fp64 (1e-12), the append is exact and nothing else in the cache changes"""
    from fiber_amd import ops
    c = dc.make_self(5, 2, D, t, ancestry, dtype=torch.float64)
    ref, _ = dc.self_reference(c)                             # (before the call: it reads the cache as it was)
    before = c["cache"].clone()
    o = ops.mha_decode_self(c["qkv"], c["cache"], c["anc"], t, 2, c["scale"])
    assert o.dtype == torch.float64 and (o - ref).abs().max() <= 1e-12
    assert torch.equal(c["cache"][:, t], c["qkv"][:, 2 * D:])
    rest = torch.ones(before.shape[:2], dtype=torch.bool)
    rest[:, t] = False                                        # (NaN marks the positions never written: compare the bits)
    assert torch.equal(c["cache"][rest].view(torch.int64), before[rest].view(torch.int64))


def test_self_host_restatement_bf16_is_inside_the_kernel_bound():
    from fiber_amd import ops
    for ancestry in (True, "masked"):
        c = dc.make_self(6, 12, 64, 17, ancestry)
        ref, bound = dc.self_reference(c)
        o = ops.mha_decode_self(c["qkv"], c["cache"], c["anc"], 17, 12, c["scale"])
        assert o.dtype == torch.bfloat16 and bool(((o.double() - ref).abs() <= bound).all())
    c["anc"][2, :18] = -1                                     # a row without any key gives 0, the other rows what they gave
    o2 = ops.mha_decode_self(c["qkv"], c["cache"], c["anc"], 17, 12, c["scale"])
    assert bool((o2[2] == 0).all()) and torch.equal(o2[[0, 1, 3, 4, 5]], o[[0, 1, 3, 4, 5]])


@pytest.mark.parametrize("Lk", dc.CROSS_LK)
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_cross_host_restatement(D, Lk):
    from fiber_amd import ops
    for spike in (None, "first", "last"):
        c = dc.make_cross(3, 5, Lk, D, heads=2, spike=spike, dtype=torch.float64)
        o = ops.mha_decode_cross(c["q"], c["kv"], 5, 2, c["scale"])
        ref, _ = dc.cross_reference(c)
        assert (o - ref).abs().max() <= 1e-12, spike
    one = ops.mha_decode_cross(c["q"][5:6], c["kv"][1:2], 1, 2, c["scale"])         # a row depends on its own query and its image only
    assert torch.equal(one[0], o[5])


def test_ops_refuse_what_the_kernels_refuse():
    from fiber_amd import ops
    c = dc.make_self(5, 2, 32, 3, True)
    with pytest.raises(ValueError):
        ops.mha_decode_self(c["qkv"], c["cache"], c["anc"], 50, 2, c["scale"])     # t >= Lmax
    with pytest.raises(ValueError):
        ops.mha_decode_self(c["qkv"], torch.zeros(5, 65, 128, dtype=torch.bfloat16), None, 3, 2, c["scale"])   # Lmax > 64
    with pytest.raises(ValueError):
        ops.mha_decode_self(c["qkv"], c["cache"], c["anc"].long(), 3, 2, c["scale"])
    with pytest.raises(ValueError):
        ops.mha_decode_self(c["qkv"][:, :3 * 48], c["cache"][..., :96].contiguous(), None, 3, 2, c["scale"])   # head width 24
    x = dc.make_cross(2, 3, 9, 32, heads=2)
    with pytest.raises(ValueError):
        ops.mha_decode_cross(x["q"][:5], x["kv"], 3, 2, x["scale"])                # N != G * R
    with pytest.raises(ValueError):
        ops.mha_decode_cross(torch.cat([x["q"]] * 6)[:34], x["kv"], 17, 2, x["scale"])   # R > 16


# -------------------------------------------------------------------------------------------- ancestry against a physically moved cache
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_ancestry_equals_a_gathered_cache(D):
    """Seven steps with a random `parent` reorder before each: following the ancestry table gives the bits a cache that is physically
    gathered at every reorder gives, and a step changes no cache byte but its own [n, t]."""
    from fiber_amd import ops
    N, heads, L = 6, 2, 8
    C = heads * D
    g = dc.gen(N, D, 77)
    by_anc = torch.full((N, L, 2 * C), float("nan"), dtype=torch.bfloat16)
    moved = by_anc.clone()
    anc = torch.zeros(N, L, dtype=torch.int32)
    own = torch.arange(N, dtype=torch.int32)
    for t in range(7):
        qkv = torch.randn(N, 3 * C, generator=g).to(torch.bfloat16)
        if t:
            parent = torch.randint(0, N, (N,), generator=g)
            anc = anc.index_select(0, parent)                 # the reorder of the ancestry form: an [N, L] int32 gather
            moved = moved.index_select(0, parent).contiguous()
        anc[:, t] = own
        before = by_anc.clone()
        a = ops.mha_decode_self(qkv, by_anc, anc, t, heads, D ** -0.5)
        b = ops.mha_decode_self(qkv, moved, None, t, heads, D ** -0.5)
        assert torch.equal(a, b), t
        assert torch.equal(by_anc[:, t], qkv[:, C:]) and torch.equal(moved[:, t], qkv[:, C:])
        rest = torch.ones(N, L, dtype=torch.bool)
        rest[:, t] = False
        assert torch.equal(by_anc[rest].view(torch.int16), before[rest].view(torch.int16)), t
        assert torch.equal(dc.gathered_cache(dict(cache=by_anc, anc=anc, t=t + 1))[:, :t + 1].view(torch.int16),
                           moved[:, :t + 1].view(torch.int16))


# --------------------------------------------------------------------------------------------- the two loops on a plain-torch stepper
V, L, HS, IMG = 41, 10, 16, 8


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.decoder = nn.Linear(HS, V)

    def forward(self, x):
        return self.decoder(x)


class _Stepper:
    """The cache of _Captioner's text model: the running sum of the embeddings so far, reordered by `parent`"""

    def __init__(self, model, image_embeds, rows):
        self.m, self.img = model, image_embeds.repeat_interleave(rows, 0).mean(1)
        self.sum, self.t = torch.zeros(self.img.shape[0], HS, dtype=torch.float64), 0

    def step(self, tokens, parent=None):
        if parent is not None and self.t:
            self.sum = self.sum.index_select(0, parent)
        self.sum = self.sum + self.m.emb(tokens)
        self.t += 1
        self.m.steps += 1
        return torch.tanh(self.m.mix(self.sum / self.t + self.img))


class _Captioner(nn.Module):
    """An image 'tower' (two tokens per image) and a causal text model: the running mean of the embeddings so far plus the image tokens"""

    def __init__(self, cache=None):
        super().__init__()
        torch.manual_seed(1)
        self.tower = nn.Linear(3 * IMG * IMG, 2 * HS)
        self.emb = nn.Embedding(V, HS)
        self.mix = nn.Linear(HS, HS)
        self.mlm_score = _Head()
        with torch.no_grad():
            self.mlm_score.decoder.weight.mul_(6.0)                       # peaked enough for some beams to end early
            self.mlm_score.decoder.bias[2] += 3.0                         # ... a little more often
        self.double()
        cfg = {"max_text_len": L, "vocab_size": V}
        if cache is not None:
            cfg["caption_decode_cache"] = cache
        self.hparams = types.SimpleNamespace(config=cfg)
        cc.attach_tokenizer(self, V)
        self.full_passes = self.steps = self.decoders = 0

    def caption_image_embeds(self, img):
        return torch.tanh(self.tower(img.flatten(1))).view(img.shape[0], 2, HS)

    def caption_decoder(self, image_embeds, rows_per_image):
        self.decoders += 1
        return _Stepper(self, image_embeds, rows_per_image)

    def infer_caption(self, batch, mask_text=False, mask_image=False, image_embeds=None):
        self.full_passes += 1
        if image_embeds is None:
            image_embeds = self.caption_image_embeds(batch["image"][0])
        ids = batch["text_ids"]
        run = self.emb(ids).cumsum(1) / torch.arange(1, ids.shape[1] + 1)[None, :, None]
        feats = torch.tanh(self.mix(run + image_embeds.mean(1, keepdim=True)))
        return {"text_feats": feats, "image_embeds": image_embeds, "text_ids": ids, "text_masks": batch["text_masks"]}


def _batch(B=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V - 1, (B, L), generator=g)
    ids[:, 0] = 0
    return {"image": [torch.randn(B, 3, IMG, IMG, generator=g, dtype=torch.float64)], "text_ids": ids, "text_labels": None,
            "text_masks": torch.ones_like(ids), "iid": list(range(B))}


@pytest.mark.parametrize("beam", [1, 3])
def test_beam_search_with_the_cache_gives_the_full_recompute_ids(beam):
    from fiber_amd.modules import objectives
    ended_early = False
    for seed in range(3):
        b = _batch(seed=seed)
        full, cached = _Captioner().eval(), _Captioner(cache=True).eval()
        want = objectives.caption_test_step(full, dict(b), None, beam_size=beam)
        got = objectives.caption_test_step(cached, dict(b), None, beam_size=beam)
        assert torch.equal(got["caption_ids"], want["caption_ids"]), (seed, got["caption_ids"], want["caption_ids"])
        assert got["captions"] == want["captions"]
        ids = want["caption_ids"]
        ended_early |= bool(((ids[:, :-1] == 2).any(1)).any()) and not bool(((ids[:, :-1] == 2).any(1)).all())
        assert cached.full_passes == 0 and cached.decoders == 1 and cached.steps == full.full_passes     # one single-token step per full pass
    assert ended_early, "no case in which some beams end before the others"


def test_sampling_with_the_cache_gives_the_full_recompute_ids():
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    b = _batch(seed=4)
    out = []
    for m in (_Captioner().train(), _Captioner(cache=True).train()):
        tok = m.trainer.datamodule.dms[0].tokenizer
        ops.manual_seed(7)
        out.append(objectives._caption_sample(m, tok, b["image"][0], None, 3, L))
        ops.manual_seed(7)
        shared = objectives._caption_sample(m, tok, b["image"][0], m.caption_image_embeds(b["image"][0]), 3, L)
        assert torch.equal(shared, out[-1])                  # image tokens handed in: the same draws
    assert torch.equal(out[0], out[1]), out
    ids = out[1]
    assert tuple(ids.shape) == (9, L) and bool((ids[:, 0] == 0).all()) and not bool((ids == V - 1).any())
    for r in ids.tolist():                                    # after the first sep / pad only pads follow
        end = next((i for i, t in enumerate(r[1:], 1) if t in (1, 2)), L)
        assert all(t == 1 for t in r[end + 1:]), r
    ops.manual_seed(8)
    m = _Captioner(cache=True).train()
    assert not torch.equal(objectives._caption_sample(m, m.trainer.datamodule.dms[0].tokenizer, b["image"][0], None, 3, L), ids)


def test_cache_off_by_default_takes_the_full_recompute():
    """caption_decode_cache unset (and the named configs' default False): infer_caption once per step, no decoder built"""
    from fiber_amd.config import make_config, named_config
    from fiber_amd.modules import objectives
    assert make_config()["caption_decode_cache"] is False
    assert named_config("task_finetune_caption_cider_coco")["caption_decode_cache"] is False
    m = _Captioner().eval()
    out = objectives.caption_test_step(m, dict(_batch()), None, beam_size=3)
    steps = int((out["caption_ids"] != 1).any(0).sum())       # columns generated before every beam had ended
    assert m.decoders == 0 and m.steps == 0 and 2 <= m.full_passes <= L - 1 and m.full_passes >= steps
    m = _Captioner().train()
    objectives._caption_sample(m, m.trainer.datamodule.dms[0].tokenizer, _batch()["image"][0], None, 3, L)
    assert m.decoders == 0 and m.full_passes >= 2


# ------------------------------------------------------------------------------------------------------------------------ wiring
def test_model_offers_a_decoder_and_refuses_the_fp32_stream():
    from fiber_amd import ops
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from fiber_amd.modules.caption_decode import CaptionDecoder
    from oracle import cases
    assert callable(FIBERTransformerSS.caption_decoder) and callable(FIBERTransformerSS.caption_image_embeds)
    assert callable(CaptionDecoder.step)
    try:
        m = FIBERTransformerSS(make_config(**dict(cases.TINY, loss_names={"caption_mle": 1}, residual_dtype="fp32")))
        with pytest.raises(NotImplementedError, match="fp32"):
            m.caption_decoder(torch.zeros(1, 9, m.config["input_image_embed_size"]), 1)
    finally:
        ops.set_residual_dtype("bf16")


def test_c_abi_exports_the_decode_entries():
    from fiber_amd import lib
    l = lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fiber_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long)\s+(fiber_\w+)\s*\(", hdr))
    for name, nargs in (("fiber_mha_decode_self_bf16", 12), ("fiber_mha_decode_cross_bf16", 11)):
        assert hasattr(l, name) and name in declared and name in lib.exported_symbols()
        assert len(lib.SIGNATURES[name]) == nargs
