"""Case tables of chunked open-vocabulary detection: the stub tokenizer, the merge cases with their seeded inputs, the independent host
reference of ops.det_merge (plain Python lists and sorted(), as the reference's LVISResults.limit_dets_per_image ranks them), the parent
commit's unsplit backbone forward, and the measured batch-size sensitivity the pair-batch test is bounded by.  Shared by
tests/test_chunked_detection_host.py, tests/test_hip_chunked_detection.py and tools/chunked_det_bench.py.  Nothing here needs a GPU to import.
"""
import re
import zlib

import numpy as np
import torch


# ---- the stub tokenizer -----------------------------------------------------------------------------------------------------------------
class Tokenized:
    """What tokenizer(query) returns: input_ids (a list) and char_to_token, as a Hugging Face fast tokenizer's BatchEncoding has them"""

    def __init__(self, query, pieces):
        self.query, self.pieces = query, pieces              # pieces: (start, end, text) per word or punctuation mark
        self.tokens = ["<s>"] + [p[2] for p in pieces] + ["</s>"]
        self.input_ids = [0] + [StubTokenizer.word_id(p[2]) for p in pieces] + [2]

    def char_to_token(self, i):
        """the position of the token that covers character i (<s> sits at position 0); None on a blank and outside the string"""
        for pos, (start, end, _) in enumerate(self.pieces, start=1):
            if start <= i < end:
                return pos
        return None


class StubTokenizer:
    """Words and punctuation marks are one token each"""

    @staticmethod
    def word_id(word):
        return 3 + zlib.crc32(word.encode()) % 50000         # never <s> 0, <pad> 1 or </s> 2

    def __call__(self, query):
        return Tokenized(query, [(m.start(), m.end(), m.group()) for m in re.finditer(r"\w+|[^\w\s]", query)])


# ---- ops.det_merge: the cases and the independent reference -------------------------------------------------------------------------------
# name: B, K, D, Cc, counts ("random", or [B][K]), levels (distinct score values; None = all different), max_dets (None, an int, or
# "total0" = exactly the live candidates of image 0)
MERGE_CASES = {
    "k1": dict(B=2, K=1, D=5, Cc=3, counts=[[5], [2]], levels=None, max_dets=4),
    "ties": dict(B=2, K=3, D=6, Cc=4, counts=[[6, 6, 6], [4, 6, 3]], levels=2, max_dets=10),         # equal scores across and within chunks
    "empty_chunk": dict(B=1, K=3, D=4, Cc=2, counts=[[3, 0, 4]], levels=3, max_dets=12),
    "empty_image": dict(B=2, K=2, D=4, Cc=2, counts=[[2, 3], [0, 0]], levels=None, max_dets=5),
    "junk": dict(B=1, K=4, D=8, Cc=5, counts=[[2, 7, 1, 5]], levels=None, max_dets=None),            # large scores past count
    "n_gt_total": dict(B=1, K=2, D=5, Cc=3, counts=[[2, 1]], levels=None, max_dets=9),
    "n_lt_total": dict(B=1, K=3, D=5, Cc=3, counts=[[5, 4, 5]], levels=4, max_dets=6),
    "n_eq_total": dict(B=2, K=3, D=5, Cc=3, counts=[[2, 4, 1], [5, 5, 5]], levels=None, max_dets="total0"),
    "d1": dict(B=2, K=5, D=1, Cc=2, counts=[[1, 0, 1, 1, 1], [1, 1, 1, 1, 1]], levels=2, max_dets=3),
    "none": dict(B=2, K=3, D=4, Cc=3, counts=[[4, 2, 3], [1, 4, 0]], levels=None, max_dets=None),
    "b3": dict(B=3, K=4, D=7, Cc=6, counts=[[7, 0, 3, 5], [1, 1, 1, 1], [0, 7, 7, 2]], levels=5, max_dets=11),
    "one": dict(B=1, K=1, D=1, Cc=1, counts=[[1]], levels=None, max_dets=1),
}
MERGE_CASES_GPU = {
    "kd70": dict(B=2, K=7, D=10, Cc=4, counts="random", levels=None, max_dets=None),                 # below one stride of the workgroup
    "lvis": dict(B=2, K=31, D=300, Cc=40, counts="random", levels=None, max_dets=300),
    "lvis_ties": dict(B=2, K=31, D=300, Cc=40, counts="random", levels=16, max_dets=None),           # dense ties
    "lvis_full": dict(B=1, K=31, D=300, Cc=40, counts="full", levels=16, max_dets=None),
}
JUNK = 9.0


def merge_inputs(name):
    """Seeded inputs of a case -> dict(boxes, scores, labels, source, count, label_table, max_dets) of CPU tensors.  The first count
    scores of every list descend; the slots past count hold JUNK scores, a label and a source, which the merge must not read as
    candidates.  The last local class of the widest chunk is always used, and so is one label the post-processor cannot emit (Cc + 1)."""
    c = dict(MERGE_CASES, **MERGE_CASES_GPU)[name]
    B, K, D, Cc = c["B"], c["K"], c["D"], c["Cc"]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    if isinstance(c["counts"], str):
        count = np.full((B, K), D) if c["counts"] == "full" else g.integers(0, D + 1, size=(B, K))
    else:
        count = np.asarray(c["counts"])
    count = count.astype(np.int32)
    if c["levels"] is None:
        raw = g.permutation(B * K * D).reshape(B, K, D).astype(np.float32) / np.float32(B * K * D)   # all different, exact in fp32
    else:
        raw = g.integers(1, c["levels"] + 1, size=(B, K, D)).astype(np.float32) / np.float32(c["levels"])
    scores = -np.sort(-raw, axis=2)
    live = np.arange(D)[None, None, :] < count[:, :, None]
    scores = np.where(live, scores, np.float32(JUNK)).astype(np.float32)
    labels = g.integers(1, Cc + 1, size=(B, K, D)).astype(np.int32)
    if count[0, 0] > 0:
        labels[0, 0, 0] = Cc                                 # the last local class of the (equally wide) first chunk
    if (B > 1 or K > 1) and count[B - 1, K - 1] > 0:
        labels[B - 1, K - 1, 0] = Cc + 1                     # cannot be emitted: must yield label 0 and read nothing
    source = g.integers(0, 1 << 30, size=(B, K, D)).astype(np.int32)
    boxes = g.random((B, K, D, 4)).astype(np.float32) * 100
    table = (g.permutation(K * Cc).reshape(K, Cc) + 1).astype(np.int32)
    max_dets = int(count[0].sum()) if c["max_dets"] == "total0" else c["max_dets"]
    t = torch.from_numpy
    return dict(boxes=t(boxes), scores=t(scores), labels=t(labels), source=t(source), count=t(count), label_table=t(table), max_dets=max_dets)


def merge_ref(boxes, scores, labels, source, count, label_table, max_dets=None):
    """The independent reference on plain Python lists: per image the first count slots of every chunk, in chunk order then slot order,
    through sorted(key=score, reverse=True)[:N] (which keeps equal scores in arrival order), then padded.
    -> (boxes, scores, labels, source, chunk, count) as tensors"""
    bx, sc, lb, sr, cn, tab = (x.tolist() for x in (boxes, scores, labels, source, count, label_table))
    B, K, D = len(sc), len(cn[0]) if cn else 0, int(scores.shape[2])
    Cc = int(label_table.shape[1])
    N = K * D if max_dets is None else min(int(max_dets), K * D)
    out = [[], [], [], [], [], []]
    for b in range(B):
        cands = [(sc[b][k][s], k, s) for k in range(K) for s in range(min(max(cn[b][k], 0), D))]
        kept = sorted(cands, key=lambda cand: cand[0], reverse=True)[:N]
        pad = N - len(kept)
        out[0].append([bx[b][k][s] for _, k, s in kept] + [[0.0] * 4] * pad)
        out[1].append([v for v, _, _ in kept] + [-1.0] * pad)
        out[2].append([tab[k][lb[b][k][s] - 1] if 1 <= lb[b][k][s] <= Cc else 0 for _, k, s in kept] + [0] * pad)
        out[3].append([sr[b][k][s] for _, k, s in kept] + [-1] * pad)
        out[4].append([k for _, k, _ in kept] + [-1] * pad)
        out[5].append(len(kept))
    i32 = torch.int32
    return (torch.tensor(out[0], dtype=torch.float32).reshape(B, N, 4), torch.tensor(out[1], dtype=torch.float32).reshape(B, N),
            torch.tensor(out[2], dtype=i32).reshape(B, N), torch.tensor(out[3], dtype=i32).reshape(B, N),
            torch.tensor(out[4], dtype=i32).reshape(B, N), torch.tensor(out[5], dtype=i32).reshape(B))


MERGE_FIELDS = ("boxes", "scores", "labels", "source", "chunk", "count")


def merge_args(x):
    return x["boxes"], x["scores"], x["labels"], x["source"], x["count"], x["label_table"], x["max_dets"]


# ---- the backbone before it was split ----------------------------------------------------------------------------------------------------
def forward_unsplit(fb, tokenizer_input, images):
    """FusionSwinTransformer.forward as it stood before image_prefix / text_prefix / fuse were cut out of it, operation for operation
    (both modalities in one loop nest): what the split forward must reproduce bit for bit."""
    import torch.nn as nn
    from fiber_amd import ops
    sw, tm = fb.backbone.body, fb.language_backbone.body.model
    x = images.tensors if hasattr(images, "tensors") else images
    x, Wh, Ww = sw.patch_embed(x)
    text = tm.embeddings(input_ids=tokenizer_input["input_ids"])
    ext = tm.get_extended_attention_mask(tokenizer_input["attention_mask"])
    for layer in tm.encoder.layer[:6]:
        text = layer(text, ext)[0]
    outs = []
    fpn = fb.backbone.fpn
    nhwc = hasattr(fpn, "forward_nhwc")

    def emit(i, t, H, W):
        if f"stage{i + 2}" in sw.out_features:
            n = getattr(sw, f"norm{i}")
            t = t if isinstance(n, nn.Identity) else ops.layernorm(t, n.weight, n.bias, n.eps)
            t = t.view(-1, H, W, sw.num_features[i])
            outs.append(t if nhwc else t.permute(0, 3, 1, 2).contiguous())
    for i in (0, 1):
        x_out, H, W, x, Wh, Ww = sw.layers[i](x, Wh, Ww)
        emit(i, x_out, H, W)
    stage = sw.layers[2]
    for j, blk in enumerate(stage.blocks):
        blk.H, blk.W = Wh, Ww
        if j < 14:
            x = blk(x)
        else:
            fused = blk(x, None, text, ext)
            text = tm.encoder.layer[j - 14 + 6](text, ext, encoder_hidden_states=x)[0]
            x = fused
    emit(2, x, Wh, Ww)
    if stage.downsample is not None:
        x = stage.downsample(x, Wh, Ww)
        Wh, Ww = (Wh + 1) // 2, (Ww + 1) // 2
    stage = sw.layers[3]
    for j in (0, 1):
        blk = stage.blocks[j]
        blk.H, blk.W = Wh, Ww
        fused = blk(x, None, text, ext)
        text = tm.encoder.layer[10 + j](text, ext, encoder_hidden_states=x)[0]
        x = fused
    emit(3, x, Wh, Ww)
    lang = fb.get_aggregated_output(text, tokenizer_input["input_ids"], tokenizer_input["attention_mask"])
    if nhwc:
        visual = tuple(t.permute(0, 3, 1, 2).float() for t in fpn.forward_nhwc(outs))
    else:
        visual = fpn(outs) if fpn is not None else outs
    return visual, lang, None


# ---- the pair batch ----------------------------------------------------------------------------------------------------------------------
# B = 2 images (64 x 96 padded; sizes (64, 96) and (60, 90)), K = 3 prompts of 2, 2 and 1 categories, passes of P = 2 and 1 prompts.
PAIR = dict(B=2, H=64, W=96, sizes=((64, 96), (60, 90)), chunk=2, P=2,
            categories=[dict(id=4, name="traffic_light", frequency="f"), dict(id=9, name="dog (animal)", frequency="c"),
                        dict(id=10, name="hot  dog", frequency="r"), dict(id=21, name="cup", frequency="f"),
                        dict(id=22, name="bird", frequency="c")])
# The existing forward's own sensitivity to the batch it runs in, MEASURED on the parent commit at the pair-batch test's very shapes
# (tools/chunked_det_bench.py --sensitivity; profiles/chunked_detection.md): the largest rel-L2 distance, per FPN level and on `embedded`,
# between forward on the replicated batch (every image next to every prompt of a pass: 4 and 2 samples) and forward on the plain batch of
# B = 2 (rows compared with the rows they replicate).  The GEMM, attention and LayerNorm kernels pick tiles by row count, so a sample's
# values may depend on its neighbours.  Zero means the pair-batch test asserts torch.equal; otherwise it allows GPU_FACTOR times this.
BATCH_SENSITIVITY = {"p3": 0.0, "p4": 0.0, "p5": 0.0, "p6": 0.0, "p7": 0.0, "embedded": 0.0}   # measured: a sample's bits do not depend on its batch


def pair_inputs(device):
    """The seeded images of the pair-batch tests -> (images [B, 3, H, W], sizes)"""
    g = np.random.default_rng(5)
    images = torch.from_numpy(g.standard_normal((PAIR["B"], 3, PAIR["H"], PAIR["W"])).astype(np.float32)).to(device)
    return images, list(PAIR["sizes"])


def make_detector(depths, device):
    """GeneralizedVLRCNN at fpn_cases.model_cfg(depths), seeded, in eval mode.  bias0 (initialised for training to a prior of 0.01, below
    INFERENCE_TH) is zeroed so that the untrained head emits detections."""
    import fpn_cases as fc
    from fiber_amd.modules import GeneralizedVLRCNN
    torch.manual_seed(0)
    model = GeneralizedVLRCNN(fc.model_cfg(depths=depths))
    with torch.no_grad():
        model.rpn.head.bias0.zero_()
    return model.to(device).eval()


def pair_prompts():
    from fiber_amd.modules import build_detection_prompts
    return build_detection_prompts(PAIR["categories"], StubTokenizer(), chunk=PAIR["chunk"])


def passes(K, P):
    return [(k0, min(P, K - k0)) for k0 in range(0, K, P)]


def pair_indices(B, k0, p, device):
    """sample b * p + j of a pass = (image b, prompt k0 + j)"""
    return torch.arange(B, device=device)[:, None].expand(B, p).reshape(-1), torch.arange(k0, k0 + p, device=device).repeat(B)


def named(visual, lang):
    out = {f"p{3 + i}": v for i, v in enumerate(visual)}
    out["embedded"] = lang["embedded"]
    return out


def batch_sensitivity(forward, images, prompts, P):
    """`forward(tokenizer_input, images)`: a backbone forward.  Per pass, its outputs on the replicated batch (every image beside every
    prompt of the pass) against its outputs on plain batches of B (image b beside prompt k0 + (b + shift) % p, all shifts, so that every
    pair occurs), assembled in the replicated order.  -> {name: the largest rel-L2 over the passes}"""
    from fpn_cases import rel_l2
    B, dev = images.shape[0], images.device
    worst = {}
    for k0, p in passes(len(prompts), P):
        ii, ti = pair_indices(B, k0, p, dev)
        big = named(*forward({"input_ids": prompts.input_ids[ti], "attention_mask": prompts.attention_mask[ti]}, images[ii])[:2])
        plain = {k: torch.empty_like(v) for k, v in big.items()}
        for shift in range(p):
            col = (torch.arange(B, device=dev) + shift) % p
            small = named(*forward({"input_ids": prompts.input_ids[k0 + col], "attention_mask": prompts.attention_mask[k0 + col]}, images)[:2])
            rows = torch.arange(B, device=dev) * p + col
            for k, v in small.items():
                plain[k][rows] = v
        for k in big:
            worst[k] = max(worst.get(k, 0.0), rel_l2(big[k], plain[k]))
    return worst
