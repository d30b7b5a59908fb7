"""Time the retrieval evaluation on one GPU at Swin-B 384^2, 50 text tokens, 8 images x 320 captions (random weights; time does not depend
on them):

  (a) ITM grid, the reference's scheme on this package's kernels: a full infer(img=image.repeat(64, ..)) per (image, batch of 64 captions)
      -- compute_itm_recall(shared_prefix=False), which is what the code before the shared-prefix methods could already run;
  (b) ITM grid with the shared prefix (text prefixes once, an image's prefix once, the fusion blocks per pair) at pair_batch 64 / 128 / 256;
  (c) the ITC path (image-only and text-only features, one fp32 GEMM);
  (d) ops.retrieval_ranks at 1000 x 5000 and 5000 x 25000 against the reference's six-topk formula (objectives.py:363-383) in torch.

    python tools/retrieval_bench.py [--rounds 5] [--images 8] [--texts 320]

Every variant is warmed up once, then the variants are run in turn `rounds` times (interleaved, same process, same box) with a host clock
around work that ends in a device synchronise; median, minimum and maximum per variant.  (b) is also compared with (a) on the scores: the
largest absolute difference of the two score matrices is printed.  Prints one JSON line.  Nothing here is asserted as a ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiber_amd import ops                                     # noqa: E402
from fiber_amd.config import named_config                     # noqa: E402
from fiber_amd.modules import FIBERTransformerSS              # noqa: E402
from fiber_amd.modules import retrieval_eval as re_           # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), runs=len(ms))


def topk_formula(scores, iids, tiids):
    """objectives.py:363-383 restated for timing only"""
    out = []
    for dim, q, c in ((0, tiids, iids), (1, iids, tiids)):
        for k in (1, 5, 10):
            idx = scores.topk(k, dim=dim).indices
            out.append(((q.unsqueeze(dim) == c[idx]).float().max(dim=dim)[0]).mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--texts", type=int, default=320)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "retrieval_bench needs a HIP device"
    dev = "cuda"
    cfg = named_config("task_finetune_irtr_itm_f30k", loss_names={"itm": 1, "itc": 1}, itc_queue_size=8)
    torch.manual_seed(0)
    model = FIBERTransformerSS(cfg).eval().to(dev)
    S, V = cfg["max_text_len"], cfg["vocab_size"]
    g = torch.Generator().manual_seed(0)
    images = torch.randn(a.images, 3, cfg["image_size"], cfg["image_size"], generator=g)
    ids = torch.randint(3, V - 2, (a.texts, S), generator=g)
    lens = torch.randint(8, S + 1, (a.texts,), generator=g)
    masks = (torch.arange(S)[None, :] < lens[:, None]).long()
    ids = torch.where(masks.bool(), ids, torch.ones_like(ids))
    ids[:, 0] = 0
    per = a.texts // a.images
    data = re_.pack_retrieval_data(images.to(dev), list(range(a.images)), ids.to(dev), masks.to(dev),
                                   [min(t // per, a.images - 1) for t in range(a.texts)], image_batch=1, text_batch=64)
    variants = {"itm_full_pass": lambda: re_.compute_itm_recall(model, data, shared_prefix=False)}
    for pb in (64, 128, 256):
        variants[f"itm_shared_prefix_pb{pb}"] = (lambda pb=pb: re_.compute_itm_recall(model, data, pair_batch=pb, shared_prefix=True))
    variants["itc"] = lambda: re_.compute_itc_recall(model, data)
    with torch.no_grad():
        ref = re_.itm_scores(model, data, shared_prefix=False)[0]
        diff = {pb: float((re_.itm_scores(model, data, pair_batch=pb)[0] - ref).abs().max()) for pb in (64, 128, 256)}
        spread = float(ref.max() - ref.min())
        for fn in variants.values():                          # warm-up: every shape once more
            fn()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
    res = {"workload": dict(images=a.images, texts=a.texts, image_size=cfg["image_size"], max_text_len=S, vit=cfg["vit"]),
           "score_range": round(spread, 5), "max_abs_diff_vs_full_pass": {f"pb{k}": v for k, v in diff.items()}}
    res.update({k: summary(v) for k, v in times.items()})
    del model, data
    torch.cuda.empty_cache()
    for Ni, Nt in ((1000, 5000), (5000, 25000)):
        gen = torch.Generator(device=dev).manual_seed(1)
        scores = torch.randn(Ni, Nt, device=dev, generator=gen)
        iids = torch.arange(Ni, device=dev, dtype=torch.int32)
        tiids = torch.arange(Nt, device=dev, dtype=torch.int32) // (Nt // Ni)
        il, tl = iids.long(), tiids.long()
        both = {"kernel": lambda: ops.retrieval_ranks(scores, iids, tiids), "topk_formula": lambda: topk_formula(scores, il, tl)}
        hits = ops.retrieval_ranks(scores, iids, tiids)[2]
        want = topk_formula(scores, il, tl)
        agree = bool(torch.allclose(torch.cat([hits[0].double() / Nt, hits[1].double() / Ni]).float(), torch.stack(want), atol=1e-6))
        for fn in both.values():
            fn()
        t = {k: [] for k in both}
        for _ in range(max(a.rounds, 7)):
            for k, fn in both.items():
                t[k].append(timed(lambda: [fn() for _ in range(5)]) / 5)
        res[f"ranks_{Ni}x{Nt}"] = dict(agree_with_topk=agree, bytes_read_twice_per_direction=4 * Ni * Nt * 4,
                                       **{k: summary(v) for k, v in t.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
