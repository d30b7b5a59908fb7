"""Time grounding training's assignment + box / centerness losses at the 800 x 1344 geometry (A = 22 400 on five levels, B = 4, 40 gts
per image): ops.atss_assign + ops.atss_box_losses forward and backward (csrc/atss.hip) against the same work done by the plain-torch
restatement of tests/atss_cases.py (assign_torch + losses_torch in fp32) on the same device.  The restatement synchronises (it reads num_gt
and loops over images), as the reference does.  Prints one JSON line; nothing gates on it.

    python tools/ground_train_bench.py [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import atss_cases as ac
    from fiber_amd import ops
    from fiber_amd.modules.grounding_inference import make_anchor_generator_complex
    from fiber_amd.modules.grounding_train import pack_targets
    dev = "cuda"
    B, G = 4, 40
    g = np.random.default_rng(0)
    anchors = [a.to(dev) for a in make_anchor_generator_complex(ac.cfg()).grid_anchors(SIZES)]
    boxes = []
    for _ in range(B):
        w, h = g.uniform(20, 600, G), g.uniform(20, 400, G)
        x, y = g.uniform(0, 1343 - w), g.uniform(0, 799 - h)
        boxes.append(torch.from_numpy(np.stack([x, y, x + w, y + h], 1).astype(np.float32)))
    labels = [torch.from_numpy(g.integers(1, 80, size=G)) for _ in range(B)]
    pmap = torch.from_numpy((g.random((B * G, 256)) < 0.02).astype(np.uint8))
    t = pack_targets(boxes, labels, pmap, device=dev)
    regs = [torch.randn(B, 4, h, w, device=dev).requires_grad_(True) for h, w in SIZES]
    ctrs = [torch.randn(B, 1, h, w, device=dev).requires_grad_(True) for h, w in SIZES]

    def kernels():
        a = ops.atss_assign(anchors, t, 9)
        s = ops.atss_box_losses(regs, ctrs, anchors, a)
        torch.autograd.grad(s[0] + s[2], regs + ctrs)

    def restated():
        a = ac.assign_torch(anchors, t, 9, dtype=torch.float32)
        ac.losses_torch(regs, ctrs, anchors, a["labels"], a["reg_targets"], dtype=torch.float32, grads=(1.0, 0.0, 1.0))

    out = {"A": sum(h * w for h, w in SIZES), "B": B, "gts_per_image": G}
    for name, fn in (("atss_hip_ms", kernels), ("atss_torch_restatement_ms", restated)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / args.steps * 1e3, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
