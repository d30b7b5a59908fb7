"""Caption fine-tuning measurements (one GPU):

    python tools/caption_bench.py [--steps 5] [--warmup 3] [--batches 8,32] [--out FILE.json]
    python tools/caption_bench.py --mode cider [--batches 8,32] [--beam 5] [--out FILE.json]

1. causal vs non-causal text self-attention (fiber_mha_causal_* vs fiber_mha_*): forward and backward at B * heads = 64 * 12, L = 50,
   D = 64 (the named config's text shape; 48 < L <= 64 takes the generic kernels with tile skipping), HIP-event timed;
2. the step time of task_finetune_caption_mle_coco (576^2 images, 50 tokens, dropout on, random weights) at per-GPU batch 8 and 32:
   forward (infer_caption + caption_mle loss), backward and the AdamW step.
--mode cider, the CIDEr-optimisation stage at task_finetune_caption_cider_coco's shape (576^2 images, 50 tokens, beam 5, random weights:
near-uniform logits, so no sampled caption ends early and every decode step runs -- the longest step the stage can take):
3. compute_caption_cider forward + backward with caption_cider_share_image off and on, and the image tower alone (forward without gradient at
   bs, forward + backward at bs and at bs * beam): the share of the step spent in the tower before and after sharing;
4. fiber_sample_rows_bf16 and fiber_seqlogp_{fwd,bwd}_bf16 against the ATen chains they replace (objectives.py:756-766 and :818-827 with
   autograd, restated on the device below, reading the head's bf16 logits), with the peak allocated bytes of each.
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


def _peak(fn):
    """peak bytes allocated by one call of fn above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def cider_kernels(bs, beam, steps=20, warmup=5, L=50, V=50265):
    """The two kernels against their ATen chains at rows = bs * beam (one decode step) and bs * beam * L (the RL pass)."""
    from fiber_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    n = bs * beam
    out = {"rows_sample": n, "rows_seqlogp": n * L, "V": V}
    x = (torch.randn(n, V, device="cuda", generator=g) * 4).to(torch.bfloat16)

    def aten_sample():                                       # objectives.py:756-758, 781-786 (+ the gather of :766)
        z = x.float()
        z[:, V - 1] = -10000
        lp = torch.log_softmax(z, dim=-1)
        tok = torch.multinomial(lp.exp_(), 1, replacement=True)
        return tok, lp.gather(-1, tok)
    out["sample_hip_us"] = round(1e3 * _time(lambda: ops.sample_rows(x, 1, V - 1), steps, warmup), 1)
    out["sample_aten_us"] = round(1e3 * _time(aten_sample, steps, warmup), 1)
    out["sample_hip_peak_bytes"], out["sample_aten_peak_bytes"] = _peak(lambda: ops.sample_rows(x, 1, V - 1)), _peak(aten_sample)
    del x
    x = (torch.randn(n * L, V, device="cuda", generator=g) * 4).to(torch.bfloat16).requires_grad_(True)
    lab = torch.randint(3, V - 1, (n, L), device="cuda", generator=g)
    lens = torch.randint(8, L, (n,), device="cuda", generator=g)
    lab = lab.masked_fill(torch.arange(L, device="cuda")[None] >= lens[:, None], 1)
    w = torch.randn(n, device="cuda", generator=g) * 100

    def reduce(lp):
        pad = lab == 1
        return ((lp.view(n, L).sum(-1) / ((~pad).float().sum(-1) + 1e-9)) * w).sum() / bs

    def hip_seq():
        x.grad = None
        reduce(ops.seq_logprob(x, lab.view(-1), 1)).backward()

    def aten_seq():                                          # objectives.py:818-827, :858-861 and their autograd
        x.grad = None
        lg = torch.log(torch.nn.functional.softmax(x.float(), dim=-1) + 1e-9)
        lp = lg.gather(dim=-1, index=lab.view(-1, 1)).view(n, L).clone()
        lp[lab == 1] = 0
        reduce(lp).backward()
    out["seqlogp_hip_us"] = round(1e3 * _time(hip_seq, steps, warmup), 1)
    out["seqlogp_aten_us"] = round(1e3 * _time(aten_seq, steps, warmup), 1)
    x.grad = None
    out["seqlogp_hip_peak_bytes"], out["seqlogp_aten_peak_bytes"] = _peak(hip_seq), _peak(aten_seq)
    return out


def cider_step(bs, beam, steps, warmup):
    from fiber_amd.config import named_config
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils, objectives
    from oracle import detgen
    import types
    res = {"B": bs, "beam": beam}
    b = None
    for share in (False, True):
        cfg = named_config("task_finetune_caption_cider_coco", per_gpu_batchsize=bs, max_steps=1000, cider_path="corpus",
                           caption_cider_share_image=share)
        model = FIBERTransformerSS(cfg).cuda().train()
        tok = types.SimpleNamespace(cls_token_id=0, pad_token_id=1, sep_token_id=2, mask_token_id=cfg["vocab_size"] - 1, cls_token="<s>",
                                    sep_token="</s>", pad_token="<pad>", decode=lambda ids: " ".join(str(i) for i in ids))
        model.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=tok)]))
        fiber_utils.set_task(model)
        if b is None:
            sb = detgen.synth_batch(bs, cfg["image_size"], cfg["max_text_len"], cfg["vocab_size"], seed=3)
            b = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
                 for k, v in sb.items()}
            b["gt_txt"] = [[" ".join(str(int(t)) for t in row[1:9]), " ".join(str(int(t)) for t in row[3:12])] for row in sb["text_ids"]]

        def one():
            model.zero_grad(set_to_none=True)
            objectives.compute_caption_cider(model, b, beam_size=beam)["caption_cider_loss"].backward()
        key = "share" if share else "separate"
        try:
            res[f"{key}_step_ms"] = round(_time(one, steps, warmup), 1)
            res[f"{key}_peak_bytes"] = _peak(one)
            if not share:                                     # the image tower alone, for its share of the step
                vit, img = model.vit_model, b["image"][0]

                def tower(x, grad):
                    with torch.set_grad_enabled(grad):
                        y = vit.patch_embed(x)
                        for layer in vit.layers:
                            y = layer(y)
                    if grad:
                        model.zero_grad(set_to_none=True)
                        y.backward(torch.ones_like(y))
                rep = img.repeat_interleave(beam, 0)
                res["tower_fwd_bs_ms"] = round(_time(lambda: tower(img, False), steps, warmup), 1)
                res["tower_fwdbwd_bs_ms"] = round(_time(lambda: tower(img, True), steps, warmup), 1)
                res["tower_fwdbwd_bs_beam_ms"] = round(_time(lambda: tower(rep, True), steps, warmup), 1)
                del rep
        except torch.cuda.OutOfMemoryError:
            res[f"{key}_step_ms"] = "out of memory"
        del model
        torch.cuda.empty_cache()
    if isinstance(res.get("separate_step_ms"), float):
        t = res["tower_fwd_bs_ms"] + res["tower_fwdbwd_bs_ms"] + res["tower_fwdbwd_bs_beam_ms"]
        res["separate_tower_share"] = round(t / res["separate_step_ms"], 3)
        if isinstance(res.get("share_step_ms"), float):
            res["share_tower_share"] = round(res["tower_fwdbwd_bs_ms"] / res["share_step_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="mle", choices=["mle", "cider"])
    ap.add_argument("--beam", type=int, default=5)
    a = ap.parse_args()
    from fiber_amd import lib
    lib.load()
    t0 = time.time()
    if a.mode == "cider":
        batches = [int(B) for B in a.batches.split(",")]
        res = {"device": torch.cuda.get_device_name(0), "kernels": cider_kernels(max(batches), a.beam)}
        res["cider_step"] = [cider_step(B, a.beam, a.steps, a.warmup) for B in batches]
    else:
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
