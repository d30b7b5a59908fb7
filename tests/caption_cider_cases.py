"""Case table of the caption_cider reference fixtures (tests/golden/caption_cider_*.npz), shared by tools/gen_caption_cider_golden.py (which runs
the reference) and the tests (which run the product on the same deterministic weights, batches, references and sampled captions)."""
import pickle
from collections import defaultdict

import numpy as np

from oracle import cases

CIDER_LOSS = {"caption_cider": 1}
ALPHA = 0.3

CIDER_CASES = {
    # D = 64 text heads at L = 12; 2 images x 3 beams
    "caption_cider_tiny": dict(config=dict(cases.TINY, loss_names=CIDER_LOSS), B=2, beam=3),
    # Swin-T (text layers 6..9 run in infer_caption), L = 40; 1 image x 2 beams
    "caption_cider_swin_t": dict(config=dict(cases.SWIN_T, loss_names=CIDER_LOSS), B=1, beam=2),
}

BATCH_SEED = 5
GT_SEED = 23


def full_config(name):
    """the case's config over the oracle's defaults (vocab_size, max_text_len, ... where the case leaves them alone)"""
    from oracle.fiber_ref import DEFAULT_CONFIG
    return dict(DEFAULT_CONFIG, **CIDER_CASES[name]["config"])


class StubTokenizer:
    """cls 0 "<s>", pad 1 "<pad>", sep 2 "</s>", mask = vocab - 1; every other id decodes to str(id)."""

    def __init__(self, vocab):
        self.cls_token_id, self.pad_token_id, self.sep_token_id, self.mask_token_id = 0, 1, 2, vocab - 1
        self.cls_token, self.sep_token, self.pad_token = "<s>", "</s>", "<pad>"
        self._special = {0: self.cls_token, 1: self.pad_token, 2: self.sep_token}

    def decode(self, ids):
        ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
        return " ".join(self._special.get(i, str(i)) for i in ids)


def attach_tokenizer(module, vocab):
    import types
    module.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=StubTokenizer(vocab))]))


def gt_ids(name):
    """Per image 2-3 reference captions as id lists: one base sentence of 6-8 ordinary ids, the others vary a token or two of it."""
    pc = CIDER_CASES[name]
    c = full_config(name)
    rng = np.random.RandomState(GT_SEED + pc["B"] * 7 + c["max_text_len"])
    lo, hi = 3, c["vocab_size"] - 1
    out = []
    for s in range(pc["B"]):
        base = rng.randint(lo, hi, size=6 + (s % 3)).tolist()
        refs = [base]
        for r in range(1 + (s + 1) % 2):                         # two more references for even samples, one for odd
            v = list(base)
            v[(2 + r) % len(v)] = int(rng.randint(lo, hi))
            if r:
                v = v[:-1] + [int(rng.randint(lo, hi)), int(rng.randint(lo, hi))]
            refs.append(v)
        out.append(refs)
    return out


def gt_txt(name):
    return [[" ".join(str(i) for i in ref) for ref in refs] for refs in gt_ids(name)]


def sampled_ids(name):
    """int64 [B * beam, max_text_len]: beam k of an image is its reference k % n with k tokens replaced and, for odd k, the last k tokens cut:
    [cls] tokens [sep] pad ...  Beam 0 equals a reference, so the CIDEr-D scores spread over (0, 10)."""
    pc = CIDER_CASES[name]
    c = full_config(name)
    L = c["max_text_len"]
    rng = np.random.RandomState(GT_SEED + 1)
    rows = []
    for refs in gt_ids(name):
        for k in range(pc["beam"]):
            v = list(refs[k % len(refs)])
            for j in range(k):
                v[(3 * j + 1) % len(v)] = int(rng.randint(3, c["vocab_size"] - 1))
            if k % 2:
                v = v[:len(v) - k]
            assert 0 < len(v) <= L - 2
            rows.append([0] + v + [2] + [1] * (L - 2 - len(v)))
    return np.array(rows, dtype=np.int64)


def df_table(name):
    """A document-frequency table in the reference's pickle layout: every n-gram of the case's references with a count in 1..7, 50 documents."""
    df = defaultdict(float)
    for refs in gt_txt(name):
        for ref in refs:
            w = (ref + " <eos>").split()
            for n in range(1, 5):
                for i in range(len(w) - n + 1):
                    g = tuple(w[i:i + n])
                    df[g] = float(1 + (sum(len(t) + ord(t[0]) for t in g) + n) % 7)
    return {"ref_len": 50, "document_frequency": df}


def write_df_table(path, table):
    with open(path, "wb") as f:
        pickle.dump(table, f)
    return str(path)


def batch_for(name):
    from oracle import detgen
    pc = CIDER_CASES[name]
    c = full_config(name)
    b = detgen.synth_batch(pc["B"], c["image_size"], c["max_text_len"], c["vocab_size"], seed=BATCH_SEED, min_len=min(8, c["max_text_len"] // 2))
    b["iid"] = list(range(100, 100 + pc["B"]))
    b["gt_txt"] = gt_txt(name)
    return b


# ---- hand-made (gts, res) sets for the scorer alone -----------------------------------------------------------------------------------
def _set(pairs):
    """pairs: [(hypothesis, [references])] -> (gts, res) as CiderD.compute_score takes them"""
    gts = {i: refs for i, (_, refs) in enumerate(pairs)}
    res = [{"image_id": i, "caption": [h]} for i, (h, _) in enumerate(pairs)]
    return gts, res


_A = "a man rides a brown horse on the beach <eos>"
_B = "a person riding a horse along the shore <eos>"
_C = "two dogs play with a red ball in the park <eos>"
_D = "a dog runs after a ball <eos>"
_E = "a plate of food with rice and vegetables on a table <eos>"

SCORER_SETS = [
    _set([(_A, [_A, _B]), (_D, [_C, _D])]),                                       # identical to a reference
    _set([(_E, [_A, _B]), (_D, [_C])]),                                           # no n-gram in common but <eos>
    _set([("zebra", [_A, _B]), (_C, [_C, _D, _B])]),                              # a single word, nothing in common at all
    _set([("horse", [_A]), ("a", [_B, _C]), (_D, [_D])]),                         # single words that do occur
    _set([("a man rides a horse <eos>", [_A, _B]), ("a dog <eos>", [_C, _D])]),   # shorter than the references
    _set([(_A + " and the sun sets behind the hills far away", [_B]), (_C, [_D])]),   # much longer
    _set([("a a a a a a <eos>", [_A, _B]), (_D, [_C, _D])]),                      # repeated word: clipping
    _set([(_B, [_A, _B, _A]), (_A, [_B]), (_C, [_C]), (_D, [_D, _C])]),           # repeated references
    _set([(_A, [_B]), (_A, [_B]), (_A, [_B])]),                                   # the same entry three times: idf 0 in corpus mode
    _set([("", [_A]), (_D, [_C, _D])]),                                           # an empty hypothesis
    _set([(_C, [_C.replace("red", "blue"), _C.replace("dogs", "cats")]), (_E, [_E.replace("rice", "beans")])]),
    _set([("12 7 301 9 <eos>", ["12 7 301 9 44 <eos>", "12 8 301 9 <eos>"]), ("5 5 6 <eos>", ["5 6 <eos>", "6 5 5 <eos>", "5 5 6 7 <eos>"])]),
]


def scorer_df_table():
    """A df table over the n-grams of SCORER_SETS' references: counts 1..9 of 40 documents, one n-gram in five left out (unseen: counted as 1)."""
    df = defaultdict(float)
    for gts, _ in SCORER_SETS:
        for refs in gts.values():
            for ref in refs:
                w = ref.split()
                for n in range(1, 5):
                    for i in range(len(w) - n + 1):
                        g = tuple(w[i:i + n])
                        k = sum(len(t) for t in g) + n
                        if k % 5:
                            df[g] = float(1 + k % 9)
    return {"ref_len": 40, "document_frequency": df}
