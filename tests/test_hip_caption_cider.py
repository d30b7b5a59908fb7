"""CIDEr-optimised caption training on the GPU: the sequence log-probability kernels (fiber_seqlogp_{fwd,bwd}_bf16) and the Gumbel-max sampling
kernel (fiber_sample_rows_bf16) element by element against fp64 on the kernels' own bf16 inputs, and compute_caption_cider against the reference
model's recorded loss terms (tests/golden/caption_cider_*.npz, tools/gen_caption_cider_golden.py).

Bounds have the form tests/ew_cases.py uses for the cross-entropy kernels, with its constants: lp, lse and the sampled log-probabilities
CONST["LSE"] (1 + |lse| + |x[l]|); dx  BF16_STORE |ref| + CONST["EXP"] |ref| (1 + |x| + |lse|) + EXP_FLOOR |rowscale|."""
import numpy as np
import pytest
import torch

from tests import caption_cider_cases as ccc
from tests import ew_cases as ec
from tests.hip_util import BF, DEV, assert_elementwise

pytestmark = pytest.mark.gpu

PAD, SEP = 1, 2
FORCED = -10000.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


# -------------------------------------------------------------------------------------------------------------------------- seq_logprob
def seqlogp_inputs(V, seqs=3, L=5):
    """bf16 logits [seqs * L, V] (std 3), labels with pad rows, one all-pad sequence (the last), labels in the unaligned head, the tail and at
    V - 1, and one label 30 below its row's maximum: p ~ 1e-13 << 1e-9, where the epsilon inside the logarithm decides value and gradient."""
    rows = seqs * L
    rs = np.random.RandomState(V)
    x = torch.from_numpy(rs.standard_normal((rows, V)).astype(np.float32) * 3).to(BF)
    lab = torch.from_numpy(rs.randint(0, V, size=rows)).long()
    lab[lab == PAD] = 0
    lab[0], lab[1], lab[2] = 0, V - 1, V - 2
    lab[3] = PAD                                             # a pad row inside a sequence
    lab[L + 4] = PAD
    lab[(seqs - 1) * L:] = PAD                               # an all-pad sequence
    r_low = L + 1
    x[r_low, lab[r_low]] = (x[r_low].float().max() - 30.0).to(BF)
    rowscale = torch.from_numpy(rs.standard_normal(rows).astype(np.float32) * 40)    # d loss / d lp: (100 - 100 cider) / len / bs
    return x.to(DEV), lab.to(DEV), rowscale.to(DEV), r_low


@pytest.mark.parametrize("V", [17, 4099, 50265])
def test_seq_logprob(lib, V):
    from fiber_amd import ops
    x, lab, rowscale, r_low = seqlogp_inputs(V)
    rows = x.shape[0]
    pad = lab == PAD
    lp = torch.full((rows,), float("nan"), device=DEV)
    lse = torch.full((rows,), float("nan"), device=DEV)
    lib.call("fiber_seqlogp_fwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(lp), lib.ptr(lse), rows, V, PAD)
    xd = x.double()
    lse_ref = torch.logsumexp(xd, 1)
    xl = xd.gather(1, lab[:, None])[:, 0]
    lp_ref = torch.log(torch.exp(xl - lse_ref) + 1e-9)
    assert bool((lp[pad] == 0).all()) and bool((lse[pad] == 0).all()), "pad rows must be exact zeros"
    assert abs(lp_ref[r_low].item() - np.log(1e-9)) < 1e-3 and (xl - lse_ref)[r_low].item() < -28   # the epsilon row is what it claims to be
    z = torch.zeros_like(lse_ref)
    scale = torch.where(pad, z, 1 + lse_ref.abs() + xl.abs())
    r1 = assert_elementwise(f"lse V{V}", lse[:, None], torch.where(pad, z, lse_ref)[:, None], (ec.CONST["LSE"] * scale)[:, None])
    r2 = assert_elementwise(f"lp V{V}", lp[:, None], torch.where(pad, z, lp_ref)[:, None], (ec.CONST["LSE"] * scale)[:, None])
    dx = torch.full((rows * V + 64,), float("nan"), device=DEV).to(BF)
    lib.call("fiber_seqlogp_bwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(lse), lib.ptr(rowscale), lib.ptr(dx), rows, V, PAD)
    assert bool(torch.isnan(dx[rows * V:].float()).all()), "guard elements written"
    dx = dx[:rows * V].view(rows, V)
    assert bool((dx[pad] == 0).all()), "pad rows must be exact zeros"
    p = torch.exp(xd - lse.double()[:, None])                # with the kernel's own lse, as ew_cases.ce_bwd_ref
    pl = p.gather(1, lab[:, None])
    oh = torch.zeros_like(p).scatter_(1, lab[:, None], 1.0)
    ref = rowscale.double()[:, None] * (pl / (pl + 1e-9)) * (oh - p)
    ref[pad] = 0
    bound = (ec.BF16_STORE * ref.abs() + ec.CONST["EXP"] * ref.abs() * (1 + xd.abs() + lse.double().abs()[:, None])
             + ec.EXP_FLOOR * rowscale.double().abs()[:, None])
    r3 = assert_elementwise(f"dx V{V}", dx, ref, bound)
    print(f"seq_logprob V={V}: worst error / bound  lse {r1:.3f}  lp {r2:.3f}  dx {r3:.3f}")
    # without the epsilon the low row's gradient would be rowscale * (onehot - p): 1e4 times larger
    assert float(dx[r_low].float().abs().max()) < 1e-3 * abs(rowscale[r_low].item())
    # the autograd binding: same numbers, per-sequence reduction in torch
    xg = x.clone().requires_grad_(True)
    out = ops.seq_logprob(xg, lab, PAD)
    assert torch.equal(out, lp)
    (out * rowscale).sum().backward()
    assert torch.equal(xg.grad, dx)
    seq = out.view(3, -1).sum(-1) / ((~pad).view(3, -1).sum(-1).float() + 1e-9)
    assert seq[2].item() == 0.0 and bool(torch.isfinite(seq).all())     # a sequence with no non-pad label yields 0, not NaN


# -------------------------------------------------------------------------------------------------------------------------- sample_rows
def sample_inputs(rows, V, std):
    return torch.from_numpy((np.random.RandomState(0).standard_normal((rows, V)) * std).astype(np.float32)).to(BF)


def emulate_sample_rows(x, K, forced, key):
    """numpy fp64: (tokens [rows, K], top-two gap of z + g [rows, K], logp [rows, K], lse [rows]) of bf16 logits x (a CPU tensor)"""
    z = x.double().numpy().copy()
    rows, V = z.shape
    if forced >= 0:
        z[:, forced] = FORCED
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    tok = np.empty((rows, K), dtype=np.int64)
    gap = np.empty((rows, K))
    col = np.arange(V, dtype=np.uint64)
    for r in range(rows):
        for k in range(K):
            idx = np.uint64((r * K + k) * V) + col               # below 2^63 for every shape here; the kernel forms it in 64 bits
            u = (ec.hash_u32(key, idx).astype(np.float64) + 0.5) * 2.0 ** -32
            s = z[r] - np.log(-np.log(u))
            t = int(s.argmax())
            tok[r, k] = t
            top = s[t]
            s[t] = -np.inf
            gap[r, k] = top - s.max()
    return tok, gap, np.take_along_axis(z, tok, 1) - lse[:, None], lse


# (rows, K, V, logit std), last column forced.  Tokens must equal the emulation wherever its top-two gap of z + g is >= 1e-3 (fp32 noise on the
# device is ~1e-5), and at most 2 % of the draws may lie under it: on the host the emulation leaves 0 of 240, 0 of 192 and 0 of 320 of these inputs.
SAMPLE_SHAPES = [(48, 5, 50265, 6.0), (64, 3, 4099, 3.0), (64, 5, 17, 2.0)]
KEY = 0x1234


@pytest.mark.parametrize("rows,K,V,std", SAMPLE_SHAPES)
def test_sample_rows(lib, rows, K, V, std):
    from fiber_amd import ops
    x = sample_inputs(rows, V, std)
    forced = V - 1
    tok_ref, gap, logp_ref, lse_ref = emulate_sample_rows(x, K, forced, KEY)
    decided = gap >= 1e-3
    print(f"sample_rows {rows}x{K}x{V}: {int((~decided).sum())} of {decided.size} draws under the 1e-3 gap")
    assert (~decided).sum() <= 0.02 * decided.size
    xd = x.to(DEV)
    tok, logp, ended = ops.sample_rows(xd, K, forced, key=KEY, pad_id=PAD, sep_id=SEP)
    assert tok.dtype == torch.int64 and tuple(tok.shape) == (rows, K) and logp.dtype == torch.float32 and ended.dtype == torch.uint8
    got = tok.cpu().numpy()
    assert np.array_equal(got[decided], tok_ref[decided]), np.argwhere((got != tok_ref) & decided)[:5]
    assert not (got == forced).any() and got.min() >= 0 and got.max() < V
    z = x.double()
    z[:, forced] = FORCED
    zt = z.gather(1, tok.cpu())
    lse = torch.from_numpy(lse_ref)[:, None]
    assert_elementwise(f"logp V{V}", logp.cpu(), zt - lse, ec.CONST["LSE"] * (1 + lse.abs() + zt.abs()))
    assert torch.equal(ended.bool(), (tok == PAD) | (tok == SEP))
    if V == 17:
        assert bool(ended.any()) and not bool(ended.all())
    tok2, logp2, _ = ops.sample_rows(xd, K, forced, key=KEY, pad_id=PAD, sep_id=SEP)
    assert torch.equal(tok, tok2) and torch.equal(logp, logp2)
    tok3, _, _ = ops.sample_rows(xd, K, forced, key=KEY + 1, pad_id=PAD, sep_id=SEP)
    assert not torch.equal(tok, tok3)
    e = (torch.arange(rows, device=DEV) % 3 == 1)
    tok4, logp4, end4 = ops.sample_rows(xd, K, forced, key=KEY, ended=e, pad_id=PAD, sep_id=SEP)
    assert bool((tok4[e] == PAD).all()) and bool((logp4[e] == 0).all()) and bool((end4[e] == 1).all())
    assert torch.equal(tok4[~e], tok[~e]) and torch.equal(logp4[~e], logp[~e]) and torch.equal(end4[~e], ended[~e])
    with pytest.raises(lib.FiberHipError):
        ops.sample_rows(xd, 9, forced, key=KEY)                   # K > 8 is refused, not truncated


def frequency_inputs():
    return torch.from_numpy((np.random.RandomState(0).standard_normal(33) * 1.5).astype(np.float32)).to(BF)


def chi_square(counts, row):
    p = torch.softmax(row.double(), 0).numpy()
    n = counts.sum()
    return float(((counts - n * p) ** 2 / (n * p)).sum())


def test_sample_rows_frequencies(lib):
    """8192 identical rows, one draw each: Pearson chi-square of the counts against the fp64 softmax, 32 degrees of freedom (mean 32,
    P(chi2 > 64) = 6e-4 for a fair sampler; the host emulation of these inputs gives 17.8, with 4 of the 8192 draws under the 1e-3 gap)."""
    from fiber_amd import ops
    row = frequency_inputs()
    x = row[None].repeat(8192, 1).contiguous().to(DEV)
    tok, _, _ = ops.sample_rows(x, 1, -1, key=77)
    counts = np.bincount(tok.view(-1).cpu().numpy(), minlength=33).astype(np.float64)
    c2 = chi_square(counts, row)
    print(f"chi-square {c2:.2f}")
    assert c2 < 64, c2


# ----------------------------------------------------------------------------------------------------------------------- the objective
def _to_dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else v)
            for k, v in b.items()}


def _fixture_model(name, tmp_path, **over):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from oracle import detgen
    pc = ccc.CIDER_CASES[name]
    path = ccc.write_df_table(tmp_path / "df.p", ccc.df_table(name))
    model = detgen.fill_(FIBERTransformerSS(make_config(**dict(pc["config"], cider_path=path, **over))))
    ccc.attach_tokenizer(model, model.config["vocab_size"])
    return model.to(DEV).train(), pc


def test_caption_cider_model_constructs(lib):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from oracle import cases
    m = FIBERTransformerSS(make_config(**dict(cases.TINY, loss_names={"caption_cider": 1}, cider_path="corpus")))
    assert hasattr(m, "cider_scorer") and hasattr(m, "mlm_score") and len(m.cross_modal_att_layers) == m.num_text_layer - 2


@pytest.mark.parametrize("name", list(ccc.CIDER_CASES))
def test_caption_cider_matches_reference(name, golden, tmp_path, lib):
    """compute_caption_cider with the cases' sampled captions against the reference's (training mode, dropout and DropPath 0): total loss, MLE
    term (the eval-mode call, which returns alpha * caption_loss) and RL term within 5e-3 relative, the logits, the gradient norm of every used
    parameter (test_caption_mle_path_matches_reference's bands), no gradient for the unused ones."""
    from fiber_amd.modules import objectives
    from tests.test_hip_modules import _gradnorm_bad, _sub_close
    gold = golden(name)
    model, pc = _fixture_model(name, tmp_path)
    b = _to_dev(ccc.batch_for(name))
    ids = torch.from_numpy(ccc.sampled_ids(name)).to(DEV)
    with torch.no_grad():
        mle = objectives.compute_caption_cider(model.eval(), b, beam_size=pc["beam"], alpha=ccc.ALPHA, sampled_ids=ids)["caption_cider_loss"].item() / ccc.ALPHA
    ret = objectives.compute_caption_cider(model.train(), b, beam_size=pc["beam"], alpha=ccc.ALPHA, sampled_ids=ids)
    total = ret["caption_cider_loss"].item()
    rl = (total - ccc.ALPHA * mle) / (1 - ccc.ALPHA)
    print(f"{name}: loss {total:.4f} (ref {float(gold['loss']):.4f})  mle {mle:.5f} ({float(gold['mle']):.5f})  rl {rl:.4f} ({float(gold['rl']):.4f})")
    for k, v in (("loss", total), ("mle", mle), ("rl", rl)):
        g = float(gold[k])
        assert abs(v - g) < 5e-3 * abs(g), (k, v, g)
    _sub_close("logits", ret["caption_cider_logits"], gold, "logits", 3e-2)
    ret["caption_cider_loss"].backward()
    unused = set(gold["unused_params"].tolist())
    gl = abs(float(gold["loss"]))
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


def test_caption_cider_trains_through_trainer(tmp_path, lib):
    """Two optimizer steps through the Trainer on synthetic data with the stub tokenizer and gt_txt, free-running sampling, text dropout on:
    finite loss, every used parameter moves, no unused one does, the loader's batches are left alone."""
    import types
    from fiber_amd.trainer import Trainer
    model, pc = _fixture_model("caption_cider_tiny", tmp_path, text_dropout=0.1, learning_rate=1e-3, warmup_steps=1, max_steps=2,
                               weight_decay=0.01, end_lr=0, decay_power=1)
    tok = model.trainer.datamodule.dms[0].tokenizer
    before = {n: p.detach().float().clone() for n, p in model.named_parameters()}
    unused = set(model.unused_parameter_names())
    data = [ccc.batch_for("caption_cider_tiny") for _ in range(2)]
    data[1]["text_ids"] = data[1]["text_ids"].flip(0)
    keep = [b["text_ids"].clone() for b in data]
    tr = Trainer(max_steps=2, log_every_n_steps=0, default_root_dir=str(tmp_path / "run"),
                 datamodule=types.SimpleNamespace(dms=[types.SimpleNamespace(tokenizer=tok)]))
    last = tr.fit(model, data)
    torch.cuda.synchronize()
    assert tr.global_step == 2 and torch.isfinite(last)
    assert "caption_cider/train/loss" in model.logged
    assert all(torch.equal(b["text_ids"], k) for b, k in zip(data, keep))
    for n, p in model.named_parameters():
        assert torch.isfinite(p.detach().float()).all(), n
        moved = not torch.equal(p.detach().float(), before[n])
        assert moved == (n not in unused), (n, moved)


def test_share_image_matches_separate_passes(tmp_path, lib):
    """caption_cider_share_image (one image-tower pass with gradient for sampling, RL and MLE) against the reference's passes, dropout and
    DropPath 0, same sampled captions: loss within 5e-3 relative, gradient norms within the _gradnorm_bad bands."""
    from fiber_amd.modules import objectives
    from tests.test_hip_modules import _gradnorm_bad
    name = "caption_cider_tiny"
    ids = torch.from_numpy(ccc.sampled_ids(name)).to(DEV)
    out = []
    for share in (False, True):
        model, pc = _fixture_model(name, tmp_path, caption_cider_share_image=share)
        b = _to_dev(ccc.batch_for(name))
        loss = objectives.compute_caption_cider(model, b, beam_size=pc["beam"], alpha=ccc.ALPHA, sampled_ids=ids)["caption_cider_loss"]
        loss.backward()
        out.append((loss.item(), {n: p.grad.double().norm().item() for n, p in model.named_parameters() if p.grad is not None}))
    assert abs(out[1][0] - out[0][0]) < 5e-3 * abs(out[0][0]), (out[0][0], out[1][0])
    assert set(out[0][1]) == set(out[1][1])
    gold = {f"gradnorm/{n}": v for n, v in out[0][1].items()}
    bad = [(n, v, out[0][1][n]) for n, v in out[1][1].items() if out[0][1][n] >= 1e-6 and _gradnorm_bad(n, v, out[0][1][n], gold)]
    assert not bad, bad
