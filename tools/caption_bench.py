"""Caption fine-tuning measurements (one GPU):

    python tools/caption_bench.py [--steps 5] [--warmup 3] [--batches 8,32] [--out FILE.json]
    python tools/caption_bench.py --mode cider [--batches 8,32] [--beam 5] [--out FILE.json]
    python tools/caption_bench.py --mode decode [--batches 8,32] [--beam 5] [--reps 3] [--out FILE.json]

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
--mode decode, KV-cached decoding (config["caption_decode_cache"], modules/caption_decode.py) at Swin-B 576^2, 50 tokens, random weights (so all
49 steps run), everything in one process, off / on alternating, HIP-event timed, --reps repetitions each:
5. caption_test_step (evaluation, beam search) with the cache off and on;
6. the caption_cider step (forward + backward, caption_cider_share_image) with the sampling half's cache off and on;
7. fiber_mha_decode_self_bf16 / fiber_mha_decode_cross_bf16 in isolation with the bytes they move per second, and one cached decoder step
   split by entry point (every launch bracketed by two events): the share spent in the GEMMs.
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


def _stub_trainer(model, cfg):
    import types
    tok = types.SimpleNamespace(cls_token_id=0, pad_token_id=1, sep_token_id=2, mask_token_id=cfg["vocab_size"] - 1, cls_token="<s>",
                                sep_token="</s>", pad_token="<pad>", decode=lambda ids: " ".join(str(i) for i in ids))
    model.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=tok)]))


def _cuda_batch(sb):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
            for k, v in sb.items()}


def _alternate(fns, reps, warmup=1):
    """HIP-event time of each fn in turn, `reps` rounds off / on / off / on ... in one process -> {name: [ms per repetition]}"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(round(_time(fn, 1, 0), 2))
    return out


def _summary(ms):
    s = sorted(ms)
    return {"ms": ms, "median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1]}


def decode_kernels(bs, beam, steps=50, warmup=10, L=50, Li=324, heads=12, D=64, positions=(1, 25, 49)):
    """The two decode kernels in isolation at the named config's text shape, with the bytes each call moves (K / V read once, q / o, the
    append) and the rate that makes.  The times here are HIP events around back-to-back calls through ops: at 10-20 us a call they hold the
    host's issue rate as much as the kernel, so the rates are lower bounds; kernel time proper comes from a kernel trace of
    --kernels-only (one position per run, so that a kernel name is one shape)"""
    from fiber_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    N, C = bs * beam, heads * D
    out = {"N": N, "R": beam, "heads": heads, "D": D, "Lmax": L, "Lk": Li}
    cache = torch.randn(N, L, 2 * C, device="cuda", generator=g).to(torch.bfloat16)
    qkv = torch.randn(N, 3 * C, device="cuda", generator=g).to(torch.bfloat16)
    anc = torch.randint(0, N, (N, L), device="cuda", generator=g, dtype=torch.int32)
    for t in positions:
        us = 1e3 * _time(lambda: ops.mha_decode_self(qkv, cache, anc, t, heads, D ** -0.5), steps, warmup)
        nbytes = 2 * N * (t * 2 * C + 3 * C + 2 * C + C) + 4 * N * (t + 1)
        out[f"self_t{t}"] = {"us": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
    del cache
    for G, R in ((bs, beam), (bs, 1), (bs, 16)):
        kv = torch.randn(G, Li, 2 * C, device="cuda", generator=g).to(torch.bfloat16)
        q = torch.randn(G * R, C, device="cuda", generator=g).to(torch.bfloat16)
        us = 1e3 * _time(lambda: ops.mha_decode_cross(q, kv, R, heads, D ** -0.5), steps, warmup)
        nbytes = 2 * (G * Li * 2 * C + 2 * G * R * C)
        out[f"cross_G{G}_R{R}"] = {"us": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
        if R == beam:                                        # what the full recompute runs per step and layer instead: K / V repeated per beam
            kvr, B = kv.repeat_interleave(R, 0).view(G * R * Li, 2 * C), G * R
            us = 1e3 * _time(lambda: ops.mha_kv_packed(q, kvr, None, B, heads, D ** -0.5), steps, warmup)
            out[f"mha_kv_packed_B{B}_Lq1"] = {"us": round(us, 2)}
            del kvr
    return out


def _step_breakdown(model, image_embeds, beam, at=25, steps=5):
    """One cached decoder step around position `at`: the HIP-event time of the whole step, and of every entry point inside it (each call
    bracketed by two events: a second, instrumented run) -> the share of the GEMMs"""
    from fiber_amd import lib
    dec = model.caption_decoder(image_embeds, beam)
    N = image_embeds.shape[0] * beam
    g = torch.Generator(device="cuda").manual_seed(1)
    tokens = lambda: torch.randint(3, 1000, (N,), device="cuda", generator=g)
    parent = lambda: torch.randint(0, N, (N,), device="cuda", generator=g)
    for _ in range(at):
        dec.step(tokens(), parent())
    tk, pr = tokens(), parent()
    whole = _time(lambda: dec.step(tk, pr), steps, 0)
    marks, inner = [], lib.call

    def traced(name, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        inner(name, *args)
        b.record()
        marks.append((name, a, b))
    lib.call = traced
    try:
        for _ in range(steps):
            dec.step(tk, pr)
        torch.cuda.synchronize()
    finally:
        lib.call = inner
    per = {}
    for name, a, b in marks:
        per[name] = per.get(name, 0.0) + a.elapsed_time(b) / steps
    kern = sum(per.values())
    gemm = sum(v for k, v in per.items() if k.startswith("fiber_gemm"))
    return {"position": at, "N": N, "step_ms": round(whole, 3), "launches": len(marks) // steps, "kernel_ms": round(kern, 3),
            "gemm_ms": round(gemm, 3), "gemm_share_of_kernel_time": round(gemm / kern, 3), "gemm_share_of_step": round(gemm / whole, 3),
            "per_entry_ms": {k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}}


def decode_step(bs, beam, reps):
    """caption_test_step (eval, random weights: near-uniform logits, so every beam runs all 49 steps) with caption_decode_cache off and on,
    alternating in one process on one model; the ids of the two paths are compared over the first steps"""
    from fiber_amd.config import named_config
    from fiber_amd.modules import FIBERTransformerSS, objectives
    from oracle import detgen
    cfg = named_config("task_finetune_caption_mle_coco", per_gpu_batchsize=bs, max_steps=1000)
    model = FIBERTransformerSS(cfg).cuda().eval()
    _stub_trainer(model, cfg)
    b = _cuda_batch(detgen.synth_batch(bs, cfg["image_size"], cfg["max_text_len"], cfg["vocab_size"], seed=3))
    b["iid"] = list(range(bs))
    hp = model.hparams.config
    ids = {}

    def run(on):
        hp["caption_decode_cache"] = on
        ids[on] = objectives.caption_test_step(model, dict(b), None, beam_size=beam)["caption_ids"]
    res = {"B": bs, "beam": beam, "L": cfg["max_text_len"], "image_size": cfg["image_size"]}
    try:
        t = _alternate({"off": lambda: run(False), "on": lambda: run(True)}, reps)
        res["cache_off"], res["cache_on"] = _summary(t["off"]), _summary(t["on"])
        res["speedup_median"] = round(res["cache_off"]["median_ms"] / res["cache_on"]["median_ms"], 2)
        res["steps_run"] = int((ids[False] != 1).any(0).sum())
        res["ids_equal_first_steps"] = int((ids[False] == ids[True]).all(0).long().cumprod(0).sum())
        with torch.no_grad():
            img = model.caption_image_embeds(b["image"][0])
            res["image_pass_ms"] = round(_time(lambda: model.caption_image_embeds(b["image"][0]), 3, 1), 2)
            res["cached_step"] = _step_breakdown(model, img, beam)
    except torch.cuda.OutOfMemoryError:
        res["error"] = "out of memory"
    hp["caption_decode_cache"] = False
    del model
    torch.cuda.empty_cache()
    return res


def decode_cider_step(bs, beam, reps):
    """compute_caption_cider forward + backward (train mode, dropout on, caption_cider_share_image) with the sampling half's cache off and on"""
    from fiber_amd.config import named_config
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils, objectives
    from oracle import detgen
    cfg = named_config("task_finetune_caption_cider_coco", per_gpu_batchsize=bs, max_steps=1000, cider_path="corpus",
                       caption_cider_share_image=True)
    model = FIBERTransformerSS(cfg).cuda().train()
    _stub_trainer(model, cfg)
    fiber_utils.set_task(model)
    sb = detgen.synth_batch(bs, cfg["image_size"], cfg["max_text_len"], cfg["vocab_size"], seed=3)
    b = _cuda_batch(sb)
    b["gt_txt"] = [[" ".join(str(int(t)) for t in row[1:9]), " ".join(str(int(t)) for t in row[3:12])] for row in sb["text_ids"]]
    hp = model.hparams.config

    def run(on):
        hp["caption_decode_cache"] = on
        model.zero_grad(set_to_none=True)
        objectives.compute_caption_cider(model, b, beam_size=beam)["caption_cider_loss"].backward()
    res = {"B": bs, "beam": beam}
    try:
        t = _alternate({"off": lambda: run(False), "on": lambda: run(True)}, reps)
        res["cache_off"], res["cache_on"] = _summary(t["off"]), _summary(t["on"])
        res["speedup_median"] = round(res["cache_off"]["median_ms"] / res["cache_on"]["median_ms"], 2)
    except torch.cuda.OutOfMemoryError:
        res["error"] = "out of memory"
    del model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="mle", choices=["mle", "cider", "decode"])
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="--mode decode: the two kernels alone (for a kernel trace)")
    ap.add_argument("--positions", default="1,25,49", help="--mode decode: the positions t the self kernel is timed at")
    a = ap.parse_args()
    from fiber_amd import lib
    lib.load()
    t0 = time.time()
    if a.mode == "cider":
        batches = [int(B) for B in a.batches.split(",")]
        res = {"device": torch.cuda.get_device_name(0), "kernels": cider_kernels(max(batches), a.beam)}
        res["cider_step"] = [cider_step(B, a.beam, a.steps, a.warmup) for B in batches]
    elif a.mode == "decode":
        batches = [int(B) for B in a.batches.split(",")]
        res = {"device": torch.cuda.get_device_name(0),
               "kernels": decode_kernels(max(batches), a.beam, positions=[int(t) for t in a.positions.split(",")])}
        if not a.kernels_only:
            res["test_step"] = [decode_step(B, a.beam, a.reps) for B in batches]
            res["cider_step"] = [decode_cider_step(B, a.beam, a.reps) for B in batches]
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
