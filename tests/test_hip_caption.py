"""Causal self-attention for the caption decoder (fiber_mha_causal_{fwd,bwd}_bf16 through ops.mha_qkv_packed(causal=True)):
parity with an fp32 torch restatement, dropout keyed like the non-causal kernels, and an exact no-look-ahead property."""
import json

import pytest
import torch

from tests.hip_util import DEV, assert_close, bf, rel_l2

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * sum(shape))
    return torch.randn(*shape, generator=g)


def _causal_ref(qkv, kmask, B, heads, scale):
    """softmax(q.k^T*scale + kmask[b, j] + (j > i ? -inf : 0)).v in fp32; qkv [B*L, 3C] = [q | k | v]."""
    C = qkv.shape[1] // 3
    D, L = C // heads, qkv.shape[0] // B
    q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(B, L, heads, D).transpose(1, 2) for i in range(3))
    a = q @ k.transpose(-1, -2) * scale
    if kmask is not None:
        a = a + kmask[:, None, None, :]
    a = a.masked_fill(torch.ones(L, L, dtype=torch.bool, device=a.device).triu(1), float("-inf"))
    return (a.softmax(-1) @ v).transpose(1, 2).reshape(B * L, C)


def _kmask(kind, B, L, seed):
    """Additive key mask: None, or padding at the end of each sample (-10000 or finfo.min); sample 0 unpadded, key 0 always valid."""
    if kind == "none":
        return None
    lens = torch.randint(1, L + 1, (B,), generator=torch.Generator().manual_seed(seed))
    lens[0] = L
    pad = -10000.0 if kind == "m10000" else FMIN
    return torch.zeros(B, L).masked_fill(torch.arange(L)[None] >= lens[:, None], pad).to(DEV)


@pytest.mark.parametrize("kind", ["m10000", "finfo", "none"])
@pytest.mark.parametrize("L", [1, 7, 12, 33, 40, 48, 49, 50, 64])
@pytest.mark.parametrize("D", [32, 64])
def test_causal_mha(ops, D, L, kind):
    B, heads = 3, (12 if D == 64 else 4)
    C = heads * D
    qkv = bf(rnd(B * L, 3 * C, seed=L + D)).requires_grad_(True)
    km = _kmask(kind, B, L, seed=L * 31 + D)
    scale = D ** -0.5
    o = ops.mha_qkv_packed(qkv, km, B, heads, scale, causal=True)
    ref_in = qkv.detach().float().requires_grad_(True)
    oref = _causal_ref(ref_in, km, B, heads, scale)
    assert_close("o", o, oref, 5e-3)
    do = bf(rnd(B * L, C, seed=3))
    o.backward(do)
    oref.backward(do.float())
    g, r = qkv.grad, ref_in.grad
    assert torch.isfinite(g.float()).all()
    for i, name in enumerate(("dq", "dk", "dv")):
        gi, ri = g[:, i * C:(i + 1) * C], r[:, i * C:(i + 1) * C]
        if float(ri.norm()) < 1e-6 * float(do.float().norm()):   # L = 1: softmax = 1, dq / dk are zero up to the bf16 rounding of O in delta
            assert float(gi.float().abs().max()) < 5e-2, name
        else:
            assert_close(name, gi, ri, 1e-2)


def test_causal_differs_from_plain(ops):
    """The causal entry point is really masked (the plain kernel on the same input gives another answer)."""
    B, heads, L, D = 2, 12, 40, 64
    qkv = bf(rnd(B * L, 3 * heads * D, seed=5))
    a = ops.mha_qkv_packed(qkv, None, B, heads, D ** -0.5)
    c = ops.mha_qkv_packed(qkv, None, B, heads, D ** -0.5, causal=True)
    assert rel_l2(c, a) > 1e-2
    assert rel_l2(c.view(B, L, -1)[:, -1], a.view(B, L, -1)[:, -1]) < 1e-2      # the last query sees every key either way


def test_causal_rejects_dense_mask(ops):
    B, heads, L, D = 2, 4, 12, 32
    qkv = bf(rnd(B * L, 3 * heads * D))
    with pytest.raises(ValueError):
        ops.mha_qkv_packed(qkv, torch.zeros(B, 1, L, L, device=DEV), B, heads, D ** -0.5, causal=True)


@pytest.mark.parametrize("D,L", [(64, 40), (64, 50), (32, 12), (32, 40)])
def test_causal_no_look_ahead_exact(ops, D, L):
    """Changing q / k / v / dO rows after position i leaves o and dq of rows <= i BIT-identical (tiles above the diagonal contribute nothing,
    the diagonal one exact zeros) -- what a KV-cached incremental decoder will rely on."""
    B, heads = 2, (12 if D == 64 else 4)
    C = heads * D
    km = _kmask("m10000", B, L, seed=9)
    base = rnd(B * L, 3 * C, seed=11)
    dob = rnd(B * L, C, seed=12)
    for cut in (0, L // 3, L - 2):
        outs = []
        for trial in range(2):
            x, dx = base.clone().view(B, L, -1), dob.clone().view(B, L, -1)
            if trial:
                x[:, cut + 1:] = rnd(B, L - cut - 1, 3 * C, seed=100 + cut)
                dx[:, cut + 1:] = rnd(B, L - cut - 1, C, seed=200 + cut)
            qkv = bf(x.view(B * L, -1)).requires_grad_(True)
            o = ops.mha_qkv_packed(qkv, km, B, heads, D ** -0.5, causal=True)
            o.backward(bf(dx.view(B * L, -1)))
            outs.append((o.view(B, L, -1)[:, :cut + 1].clone(), qkv.grad.view(B, L, -1)[:, :cut + 1, :C].clone()))
        assert torch.equal(outs[0][0], outs[1][0]), f"o rows <= {cut} changed"
        assert torch.equal(outs[0][1], outs[1][1]), f"dq rows <= {cut} changed"


@pytest.mark.parametrize("D,L", [(64, 40), (64, 50), (32, 12)])
def test_causal_dropout_adjoint(ops, D, L):
    """Attention-prob dropout on the causal path: the same seed gives the same mask in the forward and in both backward passes (the adjoint
    identity <O(V), dO> = <V, dV> holds only then), and the mean over seeds is the undropped output."""
    B, heads = 2, (12 if D == 64 else 4)
    C = heads * D
    from fiber_amd.ops import _MHAPacked
    qkv0 = bf(rnd(B * L, 3 * C, seed=21))
    vmask = torch.zeros(1, 3 * C, device=DEV, dtype=qkv0.dtype)
    vmask[:, 2 * C:] = 1

    def run(seed, p=0.1, grad=False):
        x = qkv0.clone().requires_grad_(grad)
        return x, _MHAPacked.apply(x, None, None, 0, B, heads, D ** -0.5, p, seed, True)

    _, o1 = run(1234)
    _, o2 = run(1234)
    _, o3 = run(99)
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)
    x, o = run(1234, grad=True)
    do = bf(rnd(B * L, C, seed=3))
    o.backward(do)
    lhs = (o.float() * do.float()).sum().item()
    rhs = (qkv0.float() * x.grad.float() * vmask.float()).sum().item()
    assert abs(lhs - rhs) <= 2e-2 * (abs(lhs) + 1.0), (lhs, rhs)
    base = ops.mha_qkv_packed(qkv0, None, B, heads, D ** -0.5, causal=True)
    acc = torch.zeros_like(base, dtype=torch.float32)
    n = 48
    for s in range(n):
        acc += run(1000 + s)[1].float()
    assert rel_l2(acc / n, base) < 0.08


@pytest.mark.parametrize("D,L", [(64, 40), (64, 50), (32, 12)])
def test_causal_dropout_mask_is_the_same_in_all_passes(ops, D, L):
    """Recover the keep mask from a forward with one-hot value rows (o[i, head, j] = P[i, j] * keep[i, j] / (1 - p)), then check dq / dk / dv
    against torch autograd through the causal softmax times that mask: forward, dQ and dK / dV must agree on it."""
    B, heads, p = 2, (12 if D == 64 else 4), 0.1
    C = heads * D
    from fiber_amd.ops import _MHAPacked
    qkv = bf(rnd(B * L, 3 * C, seed=31))
    eye = torch.zeros(B, L, heads, D, device=DEV)
    n = min(D, L)
    eye[:, torch.arange(n), :, torch.arange(n)] = 1.0
    probe_in = qkv.clone()
    probe_in[:, 2 * C:] = bf(eye.view(B * L, C))
    keep = torch.zeros(B, heads, L, L, device=DEV)
    probe = _MHAPacked.apply(probe_in, None, None, 0, B, heads, D ** -0.5, p, 4321, True)
    keep[..., :n] = (probe.view(B, L, heads, D)[..., :n] != 0).permute(0, 2, 1, 3).float()
    keep = keep + torch.ones(L, L, device=DEV).triu(1)        # (masked keys read as dropped; their probability is 0 anyway)
    assert n == L, "the probe covers every key"
    x = qkv.clone().requires_grad_(True)
    o = _MHAPacked.apply(x, None, None, 0, B, heads, D ** -0.5, p, 4321, True)
    do = bf(rnd(B * L, C, seed=3))
    o.backward(do)
    xr = qkv.float().requires_grad_(True)
    qr, kr, vr = (xr[:, i * C:(i + 1) * C].reshape(B, L, heads, D).transpose(1, 2) for i in range(3))
    a = (qr @ kr.transpose(-1, -2) * D ** -0.5).masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    oref = ((a.softmax(-1) * keep / (1 - p)) @ vr).transpose(1, 2).reshape(B * L, C)
    oref.backward(do.float())
    assert_close("o", o, oref, 1e-2)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert_close(name, x.grad[:, i * C:(i + 1) * C], xr.grad[:, i * C:(i + 1) * C], 2e-2)


# ---------------------------------------------------------------------------------------------------------------- the caption model
class _Tok:
    """Stub tokenizer: cls 0, pad 1, sep 2, mask = vocab - 1 (the ids detgen.synth_batch uses)."""

    def __init__(self, vocab):
        self.cls_token_id, self.pad_token_id, self.sep_token_id, self.mask_token_id = 0, 1, 2, vocab - 1
        self.pad_token = "<pad>"

    def decode(self, ids):
        return " ".join(self.pad_token if i == self.pad_token_id else str(i) for i in ids)


def _caption_model(dropout=0.0):
    import types
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from oracle import cases, detgen
    cfg = make_config(**dict(cases.TINY, loss_names={"caption_mle": 1}, text_dropout=dropout))
    model = detgen.fill_(FIBERTransformerSS(cfg)).to(DEV)
    model.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=_Tok(cfg["vocab_size"]))]))
    return model


def _batch(model, B=2, seed=1):
    from oracle import detgen
    c = model.config
    b = detgen.synth_batch(B, c["image_size"], c["max_text_len"], c["vocab_size"], seed=seed, min_len=6)
    out = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
           for k, v in b.items()}
    out["iid"] = list(range(100, 100 + B))
    return out


@pytest.fixture(scope="module")
def cap():
    from fiber_amd import lib
    lib.load()
    return _caption_model().eval()


def test_infer_caption_no_look_ahead_exact(cap):
    """text_feats of positions <= i do not change, bit for bit, when the tokens after i change (with and without a padding mask)."""
    b = _batch(cap)
    L = cap.config["max_text_len"]
    with torch.no_grad():
        for masks in (None, torch.ones_like(b["text_masks"])):
            b1 = dict(b, text_masks=masks)
            base = cap.infer_caption(b1)
            img = base["image_embeds"]
            for cut in (0, 4, L - 2):
                ids = b["text_ids"].clone()
                ids[:, cut + 1:] = torch.randint(3, cap.config["vocab_size"] - 2, ids[:, cut + 1:].shape, device=DEV)
                got = cap.infer_caption(dict(b1, text_ids=ids), image_embeds=img)
                assert torch.equal(got["text_feats"][:, :cut + 1], base["text_feats"][:, :cut + 1]), cut
                assert not torch.equal(got["text_feats"][:, cut + 1:], base["text_feats"][:, cut + 1:])


def test_caption_mle_gradients_reach_exactly_the_used_parameters():
    from fiber_amd.modules import fiber_utils, objectives
    model = _caption_model()
    model.train()
    fiber_utils.set_task(model)
    b = _batch(model)
    ret = objectives.compute_caption_mle(model, b)
    loss = ret["caption_mle_loss"]
    assert torch.isfinite(loss)
    lab = ret["caption_mle_labels"]
    ids = b["text_ids"]
    assert torch.equal(lab[:, :-1][ids[:, 1:] != 1], ids[:, 1:][ids[:, 1:] != 1]) and bool((lab[:, -1] == -100).all())
    loss.backward()
    torch.cuda.synchronize()
    unused = set(model.unused_parameter_names())
    for n, p in model.named_parameters():
        has = p.grad is not None and bool(p.grad.float().abs().sum() > 0)
        assert has == (n not in unused), (n, has)
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), n


def test_beam1_decode_matches_teacher_forcing(cap):
    """Greedy decoding (beam 1): each step's logits equal those of ONE teacher-forced infer_caption over the final sequence, and
    the decoded tokens are their arg max."""
    from fiber_amd.modules import objectives
    b = _batch(cap)
    steps = []
    h = cap.mlm_score.register_forward_hook(lambda m, i, o: steps.append(o.detach().float()))
    try:
        out = objectives.caption_test_step(cap, dict(b), None, beam_size=1)
    finally:
        h.remove()
    ids = out["caption_ids"]
    full = torch.cat([torch.zeros_like(ids[:, :1]), ids], 1)
    n = len(steps)
    with torch.no_grad():
        tf = cap.infer_caption(dict(b, text_ids=full, text_masks=None))
        logits = cap.mlm_score(tf["text_feats"]).float()
    for i, s in enumerate(steps):
        if i == 0:
            continue                                          # (step 0 runs on the batch's own text; position 0 is [CLS] either way)
        assert_close(f"step {i}", s[:, 0], logits[:, i], 2e-3)
        s = s[:, 0].clone()
        s[:, cap.config["vocab_size"] - 1] = -10000
        tok = s.argmax(-1)
        keep = ((full[:, 1:i + 1] != 1) & (full[:, 1:i + 1] != 2)).all(1)     # (a sequence that has ended is padded instead)
        assert torch.equal(tok[keep], ids[:, i][keep]), i
    assert n >= 1


def test_caption_test_step_and_wrapup(cap, tmp_path, monkeypatch):
    from fiber_amd.modules import objectives
    monkeypatch.chdir(tmp_path)
    b = _batch(cap)
    out = objectives.caption_test_step(cap, dict(b), None, beam_size=3)
    assert out["caption_ids"].shape == (2, cap.config["max_text_len"] - 1) and len(out["captions"]) == 2
    assert torch.equal(b["text_ids"], _batch(cap)["text_ids"])             # the caller's batch is left alone
    objectives.caption_test_wrapup([out], "m")
    got = json.loads((tmp_path / "result" / "caption.json").read_text())
    assert [g["image_id"] for g in got] == b["iid"] and [g["caption"] for g in got] == out["captions"]


def test_caption_training_steps_update_used_parameters_only():
    """Two optimizer steps with dropout on: finite loss and gradients; every used parameter moves, no unused one does."""
    from fiber_amd.modules import fiber_utils
    model = _caption_model(dropout=0.1)
    model.train()
    (opt,), _ = fiber_utils.set_schedule(model)
    for g in opt.param_groups:
        g["lr"] = 1e-3
    before = {n: p.detach().float().clone() for n, p in model.named_parameters()}
    unused = set(model.unused_parameter_names())
    for step in range(2):
        b = _batch(model, seed=10 + step)
        loss = model.training_step(b, step)
        assert torch.isfinite(loss)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        for n, p in model.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad.float()).all(), n
        opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        moved = not torch.equal(p.detach().float(), before[n])
        assert moved == (n not in unused), (n, moved)


# ---------------------------------------------------------------------------------------------------- parity with the reference model
def _fixture_model(name, train=False):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from oracle import detgen
    from tests import caption_cases as cc
    pc = cc.CAPTION_CASES[name]
    model = detgen.fill_(FIBERTransformerSS(make_config(**pc["config"])))      # the generator's fill: deterministic per parameter name
    cc.attach_tokenizer(model, model.config["vocab_size"])
    return model.to(DEV).train(train), pc


@pytest.mark.parametrize("name", ["caption_tiny", "caption_swin_t", "caption_swin_b_576"])
def test_caption_mle_path_matches_reference(name, golden):
    """compute_caption_mle on infer_caption against the reference's (tests/golden/caption_*.npz, eval mode): loss, logits, text_feats and image
    tokens, the gradient norm of every used parameter (test_vqa_finetune_path's bands), no gradient for the unused ones."""
    from fiber_amd.modules import objectives
    from tests import caption_cases as cc
    from tests.test_hip_modules import _gradnorm_bad, _sub_close
    gold = golden(name)
    model, pc = _fixture_model(name)
    feats = {}
    inner = model.infer_caption
    model.infer_caption = lambda batch, **kw: feats.setdefault("o", inner(batch, **kw))
    b = _to_dev(cc.batch_for(model.config, pc["B"]))
    ret = objectives.compute_caption_mle(model, b)
    gl = float(gold["loss"])
    assert abs(ret["caption_mle_loss"].item() - gl) < 5e-3 * gl, (ret["caption_mle_loss"].item(), gl)
    _sub_close("logits", ret["caption_mle_logits"], gold, "logits", 3e-2)
    _sub_close("text_feats", feats["o"]["text_feats"], gold, "text_feats", 3e-2)
    _sub_close("image_embeds", feats["o"]["image_embeds"], gold, "image_embeds", 3e-2)
    ret["caption_mle_loss"].backward()
    unused = set(gold["unused_params"].tolist())
    bad = []
    for n, p in model.named_parameters():
        if n in unused:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{n} should get no gradient"
            continue
        assert p.grad is not None, f"{n} gets no gradient"
        gn, got = float(gold[f"gradnorm/{n}"]), p.grad.double().norm().item()
        if gn < 1e-6:
            assert got < 1e-2 * max(1.0, gl), (n, got)
        elif _gradnorm_bad(n, got, gn, gold):
            bad.append((n, round(got / gn - 1, 4), float("%.3e" % gn)))
    assert not bad, bad


def test_beam3_decode_matches_reference(golden):
    """caption_test_step (beam 3) on caption_tiny: beam 0's ids equal the reference's up to the first step whose recorded kept / dropped
    beam-score gap is below caption_cases.MARGIN (past it, bf16 rounding may legitimately reorder beams)."""
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    from tests import caption_cases as cc
    gold = golden("caption_tiny")
    model, pc = _fixture_model("caption_tiny")
    cc.sharpen_for_decode(model)
    ops.mark_weights_dirty()
    b = _to_dev(cc.batch_for(model.config, pc["B"], seed=cc.DECODE_SEED))
    out = objectives.caption_test_step(model, b, None, beam_size=int(gold["decode/beam"]))
    ids = out["caption_ids"].clone()
    ids[(ids == 2) | (ids == 0)] = 1                                            # as the reference decodes them
    ref = torch.from_numpy(gold["decode/ids"])
    margins = gold["decode/margins"]
    prefixes = [cc.decode_prefix(list(margins[s]), ids.shape[1]) for s in range(ids.shape[0])]
    assert max(prefixes) >= 4
    for s, n in enumerate(prefixes):
        assert torch.equal(ids[s, :n].cpu(), ref[s, :n]), (s, n, ids[s].tolist(), ref[s].tolist())


def _to_dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else v)
            for k, v in b.items()}
