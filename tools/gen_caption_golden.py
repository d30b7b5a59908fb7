"""Generate tests/golden/caption_*.npz by running the REFERENCE's caption path (runs where the reference tree is present):

    python tools/gen_caption_golden.py [case ...]

The reference modules are executed unmodified under oracle.shim; oracle.gen_golden.RefFused carries the module tree and is extended
here with the caption modules (mlm_score, the ten cross_modal_att_layers of fiber_module.py:116-128).  infer_caption is compiled out of
the reference's fiber_module.py (with _prepare_decoder_attention_mask taken from the shim-loaded roberta module), compute_caption_mle and
caption_test_step are the reference objectives module's own functions.  Weights come from oracle.detgen.fill_ (deterministic per
parameter name), batches from tests/caption_cases.py, so the product can be filled identically; the fixtures hold outputs only.

Per case: the loss, summaries of text_feats / logits / image_embeds, the gradient norm of every used parameter, the list of unused
parameters, the sorted state-dict keys.  With `decode_beam`: the beam search's ids per sample and, per step, the gap between the last kept
and the first dropped (length-normalised) beam score."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases, detgen, shim                       # noqa: E402
from oracle.gen_golden import RefFused, _Metric, _reference_functions, save   # noqa: E402
from tests import caption_cases as cc                        # noqa: E402


def caption_model(sw, rb, heads, config):
    torch.manual_seed(0)
    m = RefFused(sw, rb, heads, config)
    c = m.c
    m.mlm_score = heads.MLMHead(shim.roberta_config(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], layer_norm_eps=1e-12))
    m.cross_modal_att_layers = nn.ModuleList([nn.Linear(c["input_image_embed_size"], int(c["input_image_embed_size"] / 2))
                                              for _ in range(c["num_layers"] - 2)])
    m.num_text_layer, m.num_fuse_block = c["num_layers"], c["num_fuse_block"]
    detgen.fill_(m)
    m.hparams = type("H", (), {"config": c})()
    m.log = lambda *a, **k: None
    for ph in ("train", "val"):
        setattr(m, f"{ph}_caption_mle_loss", _Metric())
        setattr(m, f"{ph}_caption_mle_accuracy", _Metric())
    cc.attach_tokenizer(m, c["vocab_size"])
    return m.eval()


def main():
    torch.set_num_threads(8)
    sw, rb = shim.load_reference()
    heads = shim._load("heads", os.path.join(shim.MODS, "heads.py"), "_fiber_reference_modules")
    obj = shim._load("objectives", os.path.join(shim.MODS, "objectives.py"), "_fiber_reference_modules")
    fm = _reference_functions(os.path.join(shim.MODS, "fiber_module.py"), ["infer_caption"])
    fm["_prepare_decoder_attention_mask"] = rb._prepare_decoder_attention_mask
    only = set(sys.argv[1:])
    for name, pc in cc.CAPTION_CASES.items():
        if only and name not in only:
            continue
        m = caption_model(sw, rb, heads, pc["config"])
        c = m.c
        feats = {}
        m.infer_caption = lambda batch, _f=fm["infer_caption"], _m=m, **kw: feats.setdefault("o", _f(_m, batch, **kw))
        d = {"keys": np.array(sorted(m.state_dict().keys()))}
        b = cc.batch_for(c, pc["B"])
        ret = obj.compute_caption_mle(m, b)
        o = feats["o"]
        for k in ("text_feats", "image_embeds"):
            cases.flatten_summary(k, o[k], d)
        cases.flatten_summary("logits", ret["caption_mle_logits"], d)
        d["loss"] = np.float64(ret["caption_mle_loss"].item())
        ret["caption_mle_loss"].backward()
        unused = []
        for n, p in m.named_parameters():
            if p.grad is None:
                unused.append(n)
            else:
                d[f"gradnorm/{n}"] = np.float64(p.grad.double().norm().item())
        d["unused_params"] = np.array(unused)
        print(f"  {name}: loss {d['loss']:.6f}, {len(unused)} unused parameters")
        if pc.get("decode_beam"):
            m.zero_grad(set_to_none=True)
            cc.sharpen_for_decode(m)
            m.infer_caption = lambda batch, _f=fm["infer_caption"], _m=m, **kw: _f(_m, batch, **kw)
            beam = pc["decode_beam"]
            gaps = []
            orig = torch.Tensor.argsort

            def argsort(t, *a, **kw):                        # every beam-ranking sort of the search: record kept-vs-dropped gaps
                idx = orig(t, *a, **kw)
                s = t.gather(-1, idx[..., :beam + 1]).reshape(t.shape[0], beam + 1)
                gaps.append((s[:, beam - 1] - s[:, beam]).double())
                return idx
            db = cc.batch_for(c, pc["B"], seed=cc.DECODE_SEED)
            tok = m.trainer.datamodule.dms[0].tokenizer
            decoded, plain_decode = [], tok.decode
            tok.decode = lambda t: (decoded.append(t.tolist()), plain_decode(t))[1]    # the ids behind each returned caption
            torch.Tensor.argsort = argsort
            try:
                with torch.no_grad():
                    out = obj.caption_test_step(m, dict(db), None, beam_size=beam)
            finally:
                torch.Tensor.argsort = orig
            margins = torch.stack(gaps, 1).numpy()           # [B, steps]
            d["decode/margins"] = margins
            d["decode/beam"] = np.int64(beam)
            d["decode/ids"] = np.array(decoded, dtype=np.int64)   # [B, max_text_len - 1], sep / cls -> pad as the reference decodes them
            pref = [cc.decode_prefix(list(margins[s]), c["max_text_len"] - 1) for s in range(margins.shape[0])]
            print(f"  {name}: beam {beam}, decoded prefix lengths {pref}, captions {out['captions']}")
            assert max(pref) >= 4, "no sample has a decided prefix of >= 4 tokens: pick another decode seed"
        save(name, d)


if __name__ == "__main__":
    main()
