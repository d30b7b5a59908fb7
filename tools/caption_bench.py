"""Caption fine-tuning measurements (one GPU):

    python tools/caption_bench.py [--steps 5] [--warmup 3] [--batches 8,32] [--out FILE.json]

1. causal vs non-causal text self-attention (fiber_mha_causal_* vs fiber_mha_*): forward and backward at B * heads = 64 * 12, L = 50,
   D = 64 (the named config's text shape; 48 < L <= 64 takes the generic kernels with tile skipping), HIP-event timed;
2. the step time of task_finetune_caption_mle_coco (576^2 images, 50 tokens, dropout on, random weights) at per-GPU batch 8 and 32:
   forward (infer_caption + caption_mle loss), backward and the AdamW step.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def attention(steps=50, warmup=10):
    from fiber_amd import ops
    B, heads, L, D = 64, 12, 50, 64
    C = heads * D
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B * L, 3 * C, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    lens = torch.randint(L // 2, L + 1, (B,), device="cuda", generator=g)
    km = torch.zeros(B, L, device="cuda").masked_fill(torch.arange(L, device="cuda")[None] >= lens[:, None], torch.finfo(torch.float32).min)
    do = torch.randn(B * L, C, device="cuda", generator=g).to(torch.bfloat16)
    out = {}
    for name, causal in (("plain", False), ("causal", True)):
        def fwd():
            with torch.no_grad():
                return ops.mha_qkv_packed(qkv, km, B, heads, D ** -0.5, causal=causal)

        def fwd_bwd():
            o = ops.mha_qkv_packed(qkv, km, B, heads, D ** -0.5, causal=causal)
            o.backward(do)
        f = _time(fwd, steps, warmup)
        fb = _time(fwd_bwd, steps, warmup)
        out[name] = {"fwd_us": round(1e3 * f, 1), "bwd_us": round(1e3 * (fb - f), 1)}
    return {"shape": {"B": B, "heads": heads, "L": L, "D": D}, **out}


def step_time(B, steps, warmup):
    from fiber_amd.config import named_config
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils
    from oracle import detgen
    import types
    cfg = named_config("task_finetune_caption_mle_coco", per_gpu_batchsize=B, max_steps=1000)   # (max_steps: the schedule needs a length)
    model = FIBERTransformerSS(cfg).cuda().train()
    tok = types.SimpleNamespace(cls_token_id=0, pad_token_id=1, sep_token_id=2, mask_token_id=cfg["vocab_size"] - 1, pad_token="<pad>")
    model.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=tok)]))
    (opt,), _ = fiber_utils.set_schedule(model)
    b = detgen.synth_batch(B, cfg["image_size"], cfg["max_text_len"], cfg["vocab_size"], seed=3)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
             for k, v in b.items()}

    def one():
        loss = model.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    ms = _time(one, steps, warmup)
    del model, opt
    torch.cuda.empty_cache()
    return {"B": B, "step_ms": round(ms, 2), "images_per_s": round(1e3 * B / ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from fiber_amd import lib
    lib.load()
    t0 = time.time()
    res = {"device": torch.cuda.get_device_name(0), "attention": attention()}
    res["caption_step"] = [step_time(int(B), a.steps, a.warmup) for B in a.batches.split(",")]
    res["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
