"""Generate tests/golden/caption_cider_*.npz by running the REFERENCE's CIDEr-optimisation step (runs where the reference tree is present):

    python tools/gen_caption_cider_golden.py [case ...]

As tools/gen_caption_golden.py: the reference modules run unmodified under oracle.shim, infer_caption is compiled out of the reference's
fiber_module.py, compute_caption_cider is the reference objectives module's own function and the scorer is the reference's own CiderD, reading the
df table of tests/caption_cider_cases.py from a temporary pickle.  The RL branch needs training == True, so the model runs in training mode
with dropout and DropPath at 0 (the cases' configs).  torch.multinomial is patched for the duration of the call so that the reference samples
exactly caption_cider_cases.sampled_ids; the ids it then decodes are checked against them.

Per case: the CIDEr-D scores, the total loss, the MLE term (the reference's F.cross_entropy result), the RL term (total and MLE term solved for
it), a logits summary, the gradient norm of every used parameter, the list of unused ones.  caption_cider_scorer.npz: the reference scorer's
output on caption_cider_cases.SCORER_SETS in "corpus" mode and with scorer_df_table()."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases, shim                               # noqa: E402
from oracle.gen_golden import _Metric, _reference_functions, save   # noqa: E402
from tests import caption_cider_cases as ccc                 # noqa: E402
from tools.gen_caption_golden import caption_model           # noqa: E402


def reference_ciderd():
    sys.path.insert(0, shim.MODS)
    try:
        from cider.ciderD.ciderD import CiderD
    finally:
        sys.path.remove(shim.MODS)
    return CiderD


def gen_scorer(CiderD, tmp):
    d = {}
    path = ccc.write_df_table(os.path.join(tmp, "scorer_df.p"), ccc.scorer_df_table())
    for mode, df in (("corpus", "corpus"), ("table", path)):
        scorer = CiderD(df=df)
        for i, (gts, res) in enumerate(ccc.SCORER_SETS):
            mean, scores = scorer.compute_score(gts, res)
            d[f"{mode}/{i}/mean"] = np.float64(mean)
            d[f"{mode}/{i}/scores"] = np.asarray(scores, dtype=np.float64)
    save("caption_cider_scorer", d)


def gen_case(name, pc, sw, rb, heads, obj, fm, CiderD, tmp):
    m = caption_model(sw, rb, heads, pc["config"])
    c = m.c
    for ph in ("train", "val"):
        setattr(m, f"{ph}_caption_cider_loss", _Metric())
        setattr(m, f"{ph}_caption_cider_accuracy", _Metric())
    ccc.attach_tokenizer(m, c["vocab_size"])
    m.cider_scorer = CiderD(df=ccc.write_df_table(os.path.join(tmp, name + "_df.p"), ccc.df_table(name)))
    m.infer_caption = lambda batch, _f=fm["infer_caption"], _m=m, **kw: _f(_m, batch, **kw)
    m.train()
    b = ccc.batch_for(name)
    ids = torch.from_numpy(ccc.sampled_ids(name))
    bs, beam = pc["B"], pc["beam"]
    step = [0]

    def multinomial(probs, n, replacement=False):            # the reference's draws, in its call order: step 0 [bs, beam], then [bs * beam, 1]
        i = step[0]
        step[0] += 1
        return ids.view(bs, beam, -1)[:, :, 1].clone() if i == 0 else ids[:, i + 1:i + 2].clone()

    tok = m.trainer.datamodule.dms[0].tokenizer
    decoded, plain_decode = [], tok.decode
    tok.decode = lambda t: (decoded.append(t.tolist()), plain_decode(t))[1]
    seen = {}
    inner_score = m.cider_scorer.compute_score
    m.cider_scorer.compute_score = lambda gts, res: seen.setdefault("s", inner_score(gts, res))
    ce, plain_ce = [], obj.F.cross_entropy
    orig_multinomial = torch.multinomial
    torch.multinomial = multinomial
    obj.F.cross_entropy = lambda *a, **k: (ce.append(plain_ce(*a, **k)), ce[-1])[1]
    try:
        ret = obj.compute_caption_cider(m, b, beam_size=beam, alpha=ccc.ALPHA)
    finally:
        torch.multinomial = orig_multinomial
        obj.F.cross_entropy = plain_ce
    assert decoded == ids.tolist(), "the reference did not sample caption_cider_cases.sampled_ids"
    assert len(ce) == 1
    total, mle = float(ret["caption_cider_loss"].item()), float(ce[0].item())
    d = {"cider": np.asarray(seen["s"][1], dtype=np.float64), "loss": np.float64(total), "mle": np.float64(mle),
         "rl": np.float64((total - ccc.ALPHA * mle) / (1 - ccc.ALPHA))}
    cases.flatten_summary("logits", ret["caption_cider_logits"], d)
    ret["caption_cider_loss"].backward()
    unused = []
    for n, p in m.named_parameters():
        if p.grad is None:
            unused.append(n)
        else:
            d[f"gradnorm/{n}"] = np.float64(p.grad.double().norm().item())
    d["unused_params"] = np.array(unused)
    print(f"  {name}: loss {total:.6f} = {ccc.ALPHA} * {mle:.6f} + {1 - ccc.ALPHA} * {d['rl']:.6f}; cider {np.round(d['cider'], 3).tolist()}; "
          f"{len(unused)} unused parameters")
    save(name, d)


def main():
    torch.set_num_threads(8)
    sw, rb = shim.load_reference()
    heads = shim._load("heads", os.path.join(shim.MODS, "heads.py"), "_fiber_reference_modules")
    obj = shim._load("objectives", os.path.join(shim.MODS, "objectives.py"), "_fiber_reference_modules")
    fm = _reference_functions(os.path.join(shim.MODS, "fiber_module.py"), ["infer_caption"])
    fm["_prepare_decoder_attention_mask"] = rb._prepare_decoder_attention_mask
    CiderD = reference_ciderd()
    only = set(sys.argv[1:])
    with tempfile.TemporaryDirectory() as tmp:
        if not only or "caption_cider_scorer" in only:
            gen_scorer(CiderD, tmp)
        for name, pc in ccc.CIDER_CASES.items():
            if not only or name in only:
                gen_case(name, pc, sw, rb, heads, obj, fm, CiderD, tmp)


if __name__ == "__main__":
    main()
