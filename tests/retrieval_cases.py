"""Cases of the retrieval evaluation (ops.retrieval_ranks, modules/retrieval_eval.py) and a scalar restatement of what it computes.

The restatement is numpy, one query at a time: a stable descending order of the query's candidates, then the position of the first
candidate with the query's id.  It shares no code with the package.  tools/gen_retrieval_golden.py reads the same cases by name; the
fixtures under tests/golden/ hold outputs only.

Tally cases (the smallest shapes at which the kernel can still go wrong):
  retr_small    70 images x 5 captions: one full group of 64 rows + 6, five full strips of 64 columns + 30.  Tie-free.  Ranks 0, 4, 5,
                9 and 10 occur in both directions, so each of @1 / @5 / @10 is decided from both sides.
  retr_edge     3 x 7, ks = (1, 5, 10): k > N, an image without a caption, a caption whose image is absent, a duplicated image id (the
                sampler's padding), exact ties between a match and an earlier / a later non-match, two matches with equal score.
  retr_strided  retr_small as a view of a [70, 359] matrix whose padding columns hold scores that would win.
  retr_tall     300 x 64: every wave of a column strip owns several rows; equal-scoring best match and non-match lie in different waves.
Model case: MODEL (10 images x 2 captions on oracle.cases.TINY, captions out of image order), for the end-to-end paths.  10 is the fewest
images the reference runs on: its scores.topk(10, dim=0) raises below that.
"""
import numpy as np
import torch

from oracle import cases as ocases, detgen

KS = (1, 5, 10)
BOUNDARY_RANKS = (0, 4, 5, 9, 10)


def restate(scores, iids, tiids, ks=KS):
    """-> (rank_tr int32 [Ni], rank_ir int32 [Nt], hits int32 [2, nk]); row 0 of hits = image retrieval, row 1 = text retrieval"""
    scores, iids, tiids = np.asarray(scores, np.float32), np.asarray(iids), np.asarray(tiids)

    def rank(s, qid, cid):
        order = np.argsort(-s, kind="stable")                # descending, equal scores in index order
        for pos, c in enumerate(order):
            if cid[c] == qid:
                return pos
        return len(s)
    Ni, Nt = scores.shape
    rank_tr = np.array([rank(scores[i], iids[i], tiids) for i in range(Ni)], np.int32).reshape(Ni)
    rank_ir = np.array([rank(scores[:, c], tiids[c], iids) for c in range(Nt)], np.int32).reshape(Nt)
    hits = np.array([[int((r < k).sum()) for k in ks] for r in (rank_ir, rank_tr)], np.int32).reshape(2, len(ks))
    return rank_tr, rank_ir, hits


def recalls(hits, Ni, Nt):
    """(ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10) in fp32, the reference's order"""
    h = np.asarray(hits)
    return np.concatenate([h[0].astype(np.float32) / np.float32(Nt), h[1].astype(np.float32) / np.float32(Ni)])


def _distinct(n, name):
    """n distinct fp32 values in [0, 1): a permutation of 0..n-1 over a power of two (exact)"""
    assert n < 1 << 15
    return (detgen._rng("retrieval:" + name, 0).permutation(n).astype(np.float32) / np.float32(1 << 15))


def _small():
    Ni, per = 70, 5
    Nt = Ni * per
    iids = (100 + 3 * np.arange(Ni)).astype(np.int32)
    tiids = np.repeat(iids, per)
    s = _distinct(Ni * Nt, "small").reshape(Ni, Nt)
    match = iids[:, None] == tiids[None, :]
    s = s + np.where(match, np.float32(2), np.float32(0))     # every match ahead of the background: rank 0 unless raised below
    for t, r in enumerate(BOUNDARY_RANKS[1:], start=1):      # text retrieval: image t sees r foreign captions ahead
        for j in range(10, 10 + r):
            s[t, per * j] += np.float32(3)
    for t, r in enumerate(BOUNDARY_RANKS[1:], start=0):      # image retrieval: caption 1 of image 40 + t sees r foreign images ahead
        for i in range(50, 50 + r):
            s[i, per * (40 + t) + 1] += np.float32(3)
    return dict(scores=s.astype(np.float32), iids=iids, tiids=tiids, ks=KS)


def _edge():
    iids = np.array([5, 9, 5], np.int32)                     # 5 twice (padding), 9 has no caption
    tiids = np.array([5, 7, 5, 5, 7, 5, 5], np.int32)        # 7: the image is absent
    s = np.array([[0.5, 0.9, 0.9, 0.1, 0.2, 0.9, 0.3],       # row 0: matches 2 and 5 tie at 0.9, the foreign caption 1 ties ahead of them
                  [0.6, 0.6, 0.9, 0.8, 0.05, 0.95, 0.3],
                  [0.1, 0.2, 0.3, 0.8, 0.8, 0.0, 0.3]],      # row 2: match 3 ties with the foreign caption 4 behind it
                 np.float32)
    return dict(scores=s, iids=iids, tiids=tiids, ks=KS)


def _tall():
    Ni, Nt = 300, 64
    iids = (np.arange(Ni) % 150).astype(np.int32)            # every id twice, 150 rows apart: in different waves of a strip
    tiids = ((np.arange(Nt) * 7) % 150).astype(np.int32)
    s = _distinct(Ni * Nt, "tall").reshape(Ni, Nt).copy()
    for c in range(Nt):
        r1, r2 = int(tiids[c]), int(tiids[c]) + 150
        top = max(s[r1, c], s[r2, c])
        if c % 4 == 0:                                       # two equal matches, in different waves: the lower row is the best match
            s[r1, c] = s[r2, c] = top
        elif c % 4 == 1 and r1 >= 1:                         # an equal foreign row just ahead of the best match: counted
            s[r1, c], s[r2, c], s[r1 - 1, c] = top, np.float32(0), top
        elif c % 4 == 2:                                     # an equal foreign row behind the best match: not counted
            s[r1, c], s[r2, c], s[r1 + 3, c] = top, np.float32(0), top
    return dict(scores=s.astype(np.float32), iids=iids, tiids=tiids, ks=KS)


def _strided():
    c = _small()
    wide = np.full((c["scores"].shape[0], c["scores"].shape[1] + 9), 10.0, np.float32)
    wide[:, :c["scores"].shape[1]] = c["scores"]
    return dict(c, scores=wide[:, :c["scores"].shape[1]], wide=wide)


CASES = {"retr_small": _small, "retr_edge": _edge, "retr_strided": _strided, "retr_tall": _tall}
TIE_FREE = ("retr_small", "retr_strided")                    # the reference's topk lines are defined on these


def case_inputs(name):
    c = CASES[name]()
    if name in ("retr_small", "retr_strided"):
        rank_tr, rank_ir, _ = restate(c["scores"], c["iids"], c["tiids"], c["ks"])
        for r in BOUNDARY_RANKS:
            assert (rank_tr == r).any() and (rank_ir == r).any(), f"{name}: rank {r} does not occur in both directions"
        flat = np.ascontiguousarray(c["scores"]).ravel()
        assert len(np.unique(flat)) == flat.size, f"{name}: built tie-free"
    return c


def torch_inputs(name, device="cpu"):
    """-> (scores, iids, tiids, ks) as tensors; retr_strided keeps its row stride of 359"""
    c = case_inputs(name)
    if "wide" in c:
        scores = torch.from_numpy(c["wide"].copy()).to(device)[:, :c["scores"].shape[1]]
    else:
        scores = torch.from_numpy(np.ascontiguousarray(c["scores"])).to(device)
    return scores, torch.from_numpy(c["iids"]).to(device), torch.from_numpy(c["tiids"]).to(device), c["ks"]


# ---- the model case: 10 images x 2 captions on the tiny configuration ------------------------------------------------------------------
MODEL_CONFIG = dict(ocases.TINY, loss_names={"itm": 1, "itc": 1}, itc_queue_size=6)
MODEL = dict(images=10, per_image=2, image_batch=1, text_batch=8)


def model_inputs():
    """images fp32 [10, 3, 96, 96], img_index (10 ids), text_ids / text_masks int64 [20, 12], text_img_index (20 ids, NOT in image order:
    the evaluation sorts them, objectives.py:353-355)"""
    c = MODEL_CONFIG
    n, per = MODEL["images"], MODEL["per_image"]
    b = detgen.synth_batch(n * per, c["image_size"], c["max_text_len"], c["vocab_size"], seed=7, min_len=6)
    img_index = [11, 3, 29, 17, 5, 23, 2, 41, 8, 31]
    order = detgen._rng("retrieval:model", 0).permutation(n * per)
    text_img_index = [img_index[int(j) // per] for j in order]
    return dict(images=b["image"][0][:n].clone(), img_index=img_index, text_ids=b["text_ids"], text_masks=b["text_masks"],
                text_img_index=text_img_index, image_batch=MODEL["image_batch"], text_batch=MODEL["text_batch"])
