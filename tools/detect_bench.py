"""Time grounding inference at the detection geometry (B = 2, pyramid 100x167 ... 7x11, T = 256): the HIP path (ATSSPostProcessor) against
tests/detect_cases.postprocess_torch on the device, and against the same restatement with the reference's host-side mask walk
(ml_nms.cu:112-140: the mask copied to the host and walked there).

    python tools/detect_bench.py [--setting detection|refcoco] [--iters 20] [--once PATH]

--once PATH runs each chosen path --repeat times (after a warm-up) between torch.cuda.synchronize() calls and is meant to run under
rocprofv3: two runs that differ only in --repeat give, by difference, the kernels and the HIP API calls (hipStreamSynchronize,
hipMemcpy...) of ONE call, free of set-up and warm-up.  It also counts torch's Python-level synchronising calls (Tensor.item / tolist /
cpu / nonzero, torch.cuda.synchronize) made inside the calls; that count cannot see a synchronisation made inside C++.
Timing: device events around `iters` back-to-back calls after warm-up (windows of 0.1 s and more for the HIP path), 7 such windows:
median, minimum and maximum per call (no host timer, no first call)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_cases as dc                                     # noqa: E402
from fiber_amd.modules.grounding_inference import AnchorGenerator, ATSSPostProcessor, BoxCoder   # noqa: E402

SIZES = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]
SETTINGS = {"detection": dict(C=80, thresh=0.05, top_n=1000, v2=False, agg="MEAN"),
            "refcoco": dict(C=100, thresh=0.0, top_n=3000, v2=True, agg="MEAN")}
_SYNCS = [0]


def count_syncs():
    for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "cpu"), (torch.Tensor, "nonzero"), (torch.cuda, "synchronize")):
        orig = getattr(owner, name)

        def wrap(*a, _o=orig, **k):
            _SYNCS[0] += 1
            return _o(*a, **k)
        setattr(owner, name, wrap)


def make(setting, dev="cuda"):
    s = SETTINGS[setting]
    g = torch.Generator().manual_seed(0)
    B, C = 2, s["C"]
    x = dict(logits=[], reg=[], ctr=[])
    for h, w in SIZES:
        A = h * w
        x["logits"].append((-2.2 + 1.3 * torch.randn(B, A, 1, generator=g) + 1.1 * torch.randn(B, A, dc.T, generator=g)).to(dev))
        x["reg"].append((torch.randn(B, 4, h, w, generator=g) * torch.tensor([6.0, 6.0, 3.0, 3.0]).view(1, 4, 1, 1)).to(dev))
        x["ctr"].append((0.5 + 1.5 * torch.randn(B, 1, h, w, generator=g)).to(dev))
    pm = {c + 1: [(3 * c + j) % dc.T for j in range(1 + c % 3)] for c in range(C if setting == "detection" else 3)}
    gen = AnchorGenerator(((64,), (128,), (256,), (512,), (1024,)), (1.0,), (8, 16, 32, 64, 128))
    anchors = gen.grid_anchors(SIZES, dev)
    sizes = torch.tensor([[1333.0, 800.0], [1200.0, 750.0]], device=dev)
    post = ATSSPostProcessor(s["thresh"], s["top_n"], 0.6, 100, 0, C + 1, BoxCoder(), score_agg=s["agg"],
                             mdetr_style_aggregate_class_num=C if s["v2"] else -1)
    return s, x, pm, anchors, sizes, post


def host_walk(sup_words, scores, D):
    """the reference's walk: the whole mask to the host, then ml_nms.cu:122-140 there"""
    m = sup_words.cpu().numpy()
    live = (scores >= 0).cpu().numpy()
    keep = torch.zeros(scores.shape, dtype=torch.bool)
    B, N, NB = m.shape
    for b in range(B):
        remv = [0] * NB
        kept = 0
        for i in range(N):
            if kept >= D or not live[b, i]:
                break
            if not (remv[i >> 6] >> (i & 63)) & 1:
                keep[b, i] = True
                kept += 1
                row = m[b, i]
                for j in range(i >> 6, NB):
                    remv[j] |= int(row[j]) & 0xFFFFFFFFFFFFFFFF
    return keep.to(scores.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", default="detection", choices=list(SETTINGS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--paths", default=None, help="comma-separated subset of hip,torch_host_walk,torch_device")
    ap.add_argument("--once", default=None)
    ap.add_argument("--skip-torch-walk", action="store_true", help="skip the all-device torch restatement (N launches-bound iterations)")
    a = ap.parse_args()
    s, x, pm, anchors, sizes, post = make(a.setting)
    args = (x["logits"], x["reg"], x["ctr"], anchors, sizes, pm, s["C"], s["agg"], s["thresh"], s["top_n"], 0.6, 100)

    def hip():
        return post(x["reg"], x["ctr"], sizes, anchors, x["logits"], pm)

    def torch_device():
        return dc.postprocess_torch(*args, dtype=torch.float32)

    def torch_host_walk():
        saved = dc.greedy_keep
        dc.greedy_keep = lambda sup, sc, D: host_walk(dc.mask_words(sup), sc, D)
        try:
            return dc.postprocess_torch(*args, dtype=torch.float32)
        finally:
            dc.greedy_keep = saved

    paths = {"hip": hip, "torch_host_walk": torch_host_walk}
    if not a.skip_torch_walk:
        paths["torch_device"] = torch_device
    if a.paths:
        paths = {k: v for k, v in {"hip": hip, "torch_host_walk": torch_host_walk, "torch_device": torch_device}.items() if k in a.paths.split(",")}
    res = {"setting": a.setting, "N": sum(post.level_k(h * w, s["C"]) for h, w in SIZES)}
    if a.once:
        count_syncs()
        for name, fn in paths.items():
            fn()
            torch.cuda.synchronize()
            _SYNCS[0] = 0
            for _ in range(a.repeat):
                fn()
            res[name + "_host_syncs"] = _SYNCS[0]
            res["repeat"] = a.repeat
            torch.cuda.synchronize()
        with open(a.once, "w") as f:
            json.dump(res, f)
        print(json.dumps(res))
        return
    d = hip()
    r = torch_device() if not a.skip_torch_walk else torch_host_walk()
    n = d.count.tolist()
    res["same_detections"] = all(d.source[b, :n[b]].tolist() == r["source"][b, :n[b]].tolist() for b in range(2)) and n == r["count"].tolist()
    for name, fn in paths.items():
        iters = a.iters if name == "hip" else max(1, a.iters // 40)
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / iters)
        res[name + "_ms"] = round(statistics.median(ts), 4)
        res[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
