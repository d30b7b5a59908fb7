"""Case table of the caption_mle reference fixtures (tests/golden/caption_*.npz), shared by tools/gen_caption_golden.py (which runs
the reference) and the tests (which run the product on the same deterministic weights and batches)."""
from oracle import cases

CAPTION_LOSS = {"caption_mle": 1}

CAPTION_CASES = {
    # D = 64 text heads at L = 12 (one-pass causal kernels), plus a beam-3 decode record
    "caption_tiny": dict(config=dict(cases.TINY, loss_names=CAPTION_LOSS), B=2, decode_beam=3),
    # Swin-T (text layers 6..9 run here although infer() skips them), L = 40: one-pass causal kernels
    "caption_swin_t": dict(config=dict(cases.SWIN_T, loss_names=CAPTION_LOSS), B=2),
    # the named config's shape: Swin-B at 576^2 (324 image tokens), L = 50: generic causal kernels
    "caption_swin_b_576": dict(config=dict(cases.SWIN_B, image_size=576, max_text_len=50, loss_names=CAPTION_LOSS), B=1),
}

BATCH_SEED = 5
DECODE_SEED = 11
MARGIN = 0.05          # decode ids are compared up to the first step whose kept / dropped beam-score gap is below this
# detgen's fill gives the MLM decoder logits of std ~0.16 (near-uniform over the vocabulary: every beam step a near tie); the decode record
# runs with the decoder weight and bias scaled by this factor, in the generator and in the product alike
DECODE_LOGIT_SCALE = 40.0


def sharpen_for_decode(module):
    import torch
    with torch.no_grad():
        module.mlm_score.decoder.weight.mul_(DECODE_LOGIT_SCALE)
        module.mlm_score.bias.mul_(DECODE_LOGIT_SCALE)


def batch_for(c, B, seed=BATCH_SEED):
    from oracle import detgen
    b = detgen.synth_batch(B, c["image_size"], c["max_text_len"], c["vocab_size"], seed=seed, min_len=min(8, c["max_text_len"] // 2))
    b["iid"] = list(range(100, 100 + B))
    return b


class StubTokenizer:
    """cls 0, pad 1, sep 2, mask = vocab - 1 (the ids oracle.detgen.synth_batch uses)."""

    def __init__(self, vocab):
        self.cls_token_id, self.pad_token_id, self.sep_token_id, self.mask_token_id = 0, 1, 2, vocab - 1
        self.pad_token = "<pad>"

    def decode(self, ids):
        ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
        return " ".join(self.pad_token if i == self.pad_token_id else str(i) for i in ids)


def attach_tokenizer(module, vocab):
    import types
    module.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=StubTokenizer(vocab))]))


def decode_prefix(margins, max_steps):
    """Steps before the first one whose margin (per sample) is below MARGIN: the ids of those steps are determined."""
    for i, m in enumerate(margins[:max_steps]):
        if m < MARGIN:
            return i
    return min(len(margins), max_steps)
