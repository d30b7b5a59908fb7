"""KV-cached caption decoding on the GPU: the two single-token attention kernels (csrc/attn_decode.hip) per element against fp64, their
written regions and refusals, and CaptionDecoder / the cached decoding loops against the reference model's record and the full recompute.

Kernel bound: decode_cases' terms["O"] of attn_cases.attention64 with attn_cases.CONST unchanged."""
import pytest
import torch

from tests import attn_cases as ac
from tests import decode_cases as dc
from tests.hip_util import DEV, assert_elementwise

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def _bits(x):
    return x.contiguous().view(torch.int16)


def _is_nan_fill(x):
    return bool((_bits(x) == ac.NAN_BF16).all())


# ------------------------------------------------------------------------------------------------------------------------ self
def _run_self(lib, c, cache=None, anc="own"):
    """fiber_mha_decode_self_bf16 on padded, NaN-guarded buffers -> (o [N, C], the cache buffer [N + 1, Lmax, 2C], o's buffer)"""
    N, C = c["qkv"].shape[0], c["heads"] * c["D"]
    cache = c["cache"] if cache is None else cache
    Lmax = cache.shape[1]
    qkv = dc.padded(c["qkv"]).to(DEV)
    cbuf = torch.full((N + 1, Lmax, 2 * C), float("nan"), dtype=BF, device=DEV)          # a guard slot; positions >= t are NaN already
    cbuf[:N] = cache.to(DEV)
    o = ac.nan_bf16(N + 1, C + dc.PAD)
    a = c["anc"] if isinstance(anc, str) else anc
    a = a.to(DEV) if a is not None else None
    lib.call("fiber_mha_decode_self_bf16", lib.ptr(qkv), lib.ptr(cbuf), lib.ptr(a), lib.ptr(o), N, c["heads"], c["D"], c["t"], Lmax,
             3 * C + dc.PAD, C + dc.PAD, c["scale"])
    torch.cuda.synchronize()
    return o[:N, :C], cbuf, o


@pytest.mark.parametrize("t", dc.SELF_T)
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_self_kernel(lib, D, t):
    """Values per element against fp64; o's guard row / columns and the cache's guard slot and positions > t still NaN (nothing past t is read:
    a NaN key or value would surface in o); cache[n, t] = the new k | v exactly and no other cache byte changed; the ancestry form equals
    the call on a physically gathered cache with anc NULL, bit for bit."""
    for N in dc.SELF_N:
        for heads in dc.SELF_HEADS:
            for ancestry in (False, True, "masked"):
                name = f"self D{D} t{t} N{N} h{heads} anc={ancestry}"
                c = dc.make_self(N, heads, D, t, ancestry)
                C = heads * D
                ref, bound = dc.self_reference(c)
                got, cbuf, obuf = _run_self(lib, c)
                assert_elementwise(name, got.cpu(), ref, bound)
                assert _is_nan_fill(obuf[N]) and _is_nan_fill(obuf[:N, C:]), f"{name}: o written outside [N, C]"
                assert torch.equal(cbuf[:N, t].cpu(), c["qkv"][:, C:]), f"{name}: cache[n, t] is not the new k | v"
                rest = torch.ones(N + 1, cbuf.shape[1], dtype=torch.bool)
                rest[:N, t] = False
                want = torch.full_like(cbuf, float("nan")).cpu()
                want[:N] = c["cache"]
                assert torch.equal(_bits(cbuf.cpu()[rest]), _bits(want[rest])), f"{name}: a cache byte outside [n, t] changed"
                if ancestry is True:
                    moved, _, _ = _run_self(lib, c, cache=dc.gathered_cache(c), anc=None)
                    assert torch.equal(_bits(moved), _bits(got)), f"{name}: ancestry form differs from the gathered cache"


def test_self_row_without_a_key_gives_zero(lib):
    c = dc.make_self(5, 2, 64, 17, "masked")
    base, _, _ = _run_self(lib, c)
    c["anc"][3, :18] = -1
    got, _, _ = _run_self(lib, c)
    assert bool((got[3] == 0).all()) and torch.equal(_bits(got[[0, 1, 2, 4]]), _bits(base[[0, 1, 2, 4]]))


def test_ops_self_matches_the_abi_run_and_appends_in_place(lib):
    from fiber_amd import ops
    c = dc.make_self(6, 12, 64, 49, True)
    want, cbuf, _ = _run_self(lib, c)
    cache = c["cache"].to(DEV)
    wide = dc.padded(c["qkv"]).to(DEV)
    got = ops.mha_decode_self(wide[:6, :3 * 768], cache, c["anc"].to(DEV), 49, 12, c["scale"])       # a strided view: no copy needed
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(cache), _bits(cbuf[:6]))


# ----------------------------------------------------------------------------------------------------------------------- cross
def _run_cross(lib, c, q=None, kv=None, R=None):
    q = c["q"] if q is None else q
    kv = c["kv"] if kv is None else kv
    R = c["R"] if R is None else R
    N, C = q.shape[0], c["heads"] * c["D"]
    G, Lk = kv.shape[0], kv.shape[1]
    qb = dc.padded(q).to(DEV)
    kb = torch.full((G + 1, Lk, 2 * C), float("nan"), dtype=BF, device=DEV)              # a guard image
    kb[:G] = kv.to(DEV)
    o = ac.nan_bf16(N + 1, C + dc.PAD)
    lib.call("fiber_mha_decode_cross_bf16", lib.ptr(qb), lib.ptr(kb), lib.ptr(o), N, R, c["heads"], Lk, c["D"], C + dc.PAD, C + dc.PAD, c["scale"])
    torch.cuda.synchronize()
    assert _is_nan_fill(o[N]) and _is_nan_fill(o[:N, C:]), "o written outside [N, C]"
    return o[:N, :C]


@pytest.mark.parametrize("Lk", dc.CROSS_LK)
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_cross_kernel(lib, D, Lk):
    for G in dc.CROSS_G:
        for R in dc.CROSS_R:
            c = dc.make_cross(G, R, Lk, D)
            ref, bound = dc.cross_reference(c)
            assert_elementwise(f"cross D{D} Lk{Lk} G{G} R{R}", _run_cross(lib, c).cpu(), ref, bound)


@pytest.mark.parametrize("spike", ["first", "last"])
@pytest.mark.parametrize("Lk", [49, 324, 333])
@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_cross_kernel_spike(lib, D, Lk, spike):
    """Scores over +-60 with the maximum on the first or the last key: the waves' partial softmaxes have maxima far apart"""
    c = dc.make_cross(3, 5, Lk, D, spike=spike)
    ref, bound = dc.cross_reference(c)
    assert_elementwise(f"cross spike-{spike} D{D} Lk{Lk}", _run_cross(lib, c).cpu(), ref, bound)


@pytest.mark.parametrize("D", dc.HEAD_DIMS)
def test_cross_rows_are_independent(lib, D):
    """A row's bits depend neither on the other rows' queries nor on R: other queries replaced; R = 5 against five R = 1 calls' worth of
    repeated K / V; and R = 16, 8, 3 (other register bounds) on the same rows"""
    c = dc.make_cross(3, 5, 324, D)
    base = _run_cross(lib, c)
    for keep in (0, 7, 14):
        q = torch.randn(c["q"].shape, generator=dc.gen(keep, D)).to(BF)
        q[keep] = c["q"][keep]
        assert torch.equal(_bits(_run_cross(lib, c, q=q)[keep]), _bits(base[keep])), keep
    single = _run_cross(lib, c, kv=c["kv"].repeat_interleave(5, 0), R=1)
    assert torch.equal(_bits(single), _bits(base))
    for R in (3, 8, 16):
        qs = c["q"].view(3, 5, -1)
        q = torch.randn(3, R, qs.shape[-1], generator=dc.gen(R, D)).to(BF)
        n = min(R, 5)
        q[:, :n] = qs[:, :n]
        got = _run_cross(lib, c, q=q.reshape(3 * R, -1), R=R).view(3, R, -1)
        assert torch.equal(_bits(got[:, :n]), _bits(base.view(3, 5, -1)[:, :n])), R


def test_ops_cross_matches_the_abi_run(lib):
    from fiber_amd import ops
    c = dc.make_cross(3, 5, 49, 64)
    got = ops.mha_decode_cross(dc.padded(c["q"]).to(DEV)[:15, :768], c["kv"].to(DEV), 5, 12, c["scale"])
    assert torch.equal(_bits(got), _bits(_run_cross(lib, c)))


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_decode_refusals(lib):
    """FIBER_EINVAL for every contract the two entry points state; nothing is launched, so o stays untouched"""
    from fiber_amd.lib import FiberHipError
    N, heads, D, Lmax = 6, 2, 32, 50
    C = heads * D
    qkv = torch.zeros(N, 3 * C + 8, dtype=BF, device=DEV)
    cache = torch.zeros(N, 64, 2 * C, dtype=BF, device=DEV)
    anc = torch.zeros(N, 64, dtype=torch.int32, device=DEV)
    o = ac.nan_bf16(N, C + 8)
    good = dict(N=N, heads=heads, D=D, t=3, Lmax=Lmax, ldqkv=3 * C + 8, ldo=C + 8)

    def call_self(qkv=qkv, **over):
        a = dict(good, **over)
        lib.call("fiber_mha_decode_self_bf16", lib.ptr(qkv), lib.ptr(cache), lib.ptr(anc), lib.ptr(o), a["N"], a["heads"], a["D"], a["t"],
                 a["Lmax"], a["ldqkv"], a["ldo"], 0.125)

    call_self()
    for over in (dict(D=48), dict(D=128), dict(t=50), dict(t=-1), dict(Lmax=65, t=3), dict(ldqkv=3 * C + 4), dict(ldo=C + 4),
                 dict(ldqkv=3 * C - 8), dict(ldo=C - 8), dict(heads=0), dict(N=-1)):
        with pytest.raises(FiberHipError, match="invalid argument"):
            call_self(**over)
    with pytest.raises(FiberHipError, match="invalid argument"):
        call_self(qkv=qkv.view(-1)[4:])                      # an 8-byte offset: misaligned for the 16-byte loads

    G, R, Lk = 2, 3, 9
    q = torch.zeros(G * R, C + 8, dtype=BF, device=DEV)
    kv = torch.zeros(G, Lk, 2 * C, dtype=BF, device=DEV)
    o = ac.nan_bf16(G * 17, C + 8)
    goodx = dict(N=G * R, R=R, heads=heads, Lk=Lk, D=D, ldq=C + 8, ldo=C + 8)

    def call_cross(**over):
        a = dict(goodx, **over)
        lib.call("fiber_mha_decode_cross_bf16", lib.ptr(q), lib.ptr(kv), lib.ptr(o), a["N"], a["R"], a["heads"], a["Lk"], a["D"], a["ldq"],
                 a["ldo"], 0.125)

    call_cross()
    for over in (dict(D=16), dict(R=17, N=34), dict(R=0), dict(N=5), dict(Lk=0), dict(ldq=C + 4), dict(ldo=C + 2), dict(ldq=C - 8), dict(heads=0)):
        with pytest.raises(FiberHipError, match="invalid argument"):
            call_cross(**over)
    torch.cuda.synchronize()
    assert _is_nan_fill(o[G * R:])


# ------------------------------------------------------------------------------------------------------------------- the model
def _fixture(name, train=False, **over):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    from oracle import detgen
    from tests import caption_cases as cc
    pc = cc.CAPTION_CASES[name]
    model = detgen.fill_(FIBERTransformerSS(make_config(**dict(pc["config"], **over))))   # the generator's fill: deterministic per parameter name
    cc.attach_tokenizer(model, model.config["vocab_size"])
    return model.to(DEV).train(train), pc


def _to_dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else v)
            for k, v in b.items()}


def _teacher_forced(model, b):
    """The batch's own ids, token by token, through a CaptionDecoder with one row per image and the batch's padding mask -> [B, L, H]"""
    ids, masks = b["text_ids"], b["text_masks"]
    with torch.no_grad():
        dec = model.caption_decoder(model.caption_image_embeds(b["image"][0]), 1)
        return torch.stack([dec.step(ids[:, t], live=masks[:, t] != 0) for t in range(ids.shape[1])], 1)


def test_teacher_forced_cached_decoding_matches_reference(lib, golden):
    """caption_tiny: the stacked single-token features against the reference's text_feats, at the tolerance
    test_caption_mle_path_matches_reference applies to the same quantity on the full path; and against the full path itself."""
    from tests import caption_cases as cc
    from tests.hip_util import rel_l2
    from tests.test_hip_modules import _sub_close
    model, pc = _fixture("caption_tiny")
    b = _to_dev(cc.batch_for(model.config, pc["B"]))
    feats = _teacher_forced(model, b)
    e = _sub_close("text_feats", feats, golden("caption_tiny"), "text_feats", 3e-2)
    with torch.no_grad():
        full = model.infer_caption(b)["text_feats"]
    print(f"teacher-forced caption_tiny: rel-L2 {e:.3e} against the reference, {rel_l2(feats, full):.3e} against infer_caption")
    assert rel_l2(feats, full) <= 3e-2


def test_teacher_forced_swin_b_shape(lib, golden):
    """caption_swin_b_576 (Li = 324, L = 50, generic causal kernels on the full path), one image: the cached pass at positions 0, 24 and 49
    against the elements of the golden's strided text_feats sample that lie in those positions"""
    import numpy as np
    from oracle import cases
    from tests import caption_cases as cc
    from tests.hip_util import rel_l2
    model, pc = _fixture("caption_swin_b_576")
    b = _to_dev(cc.batch_for(model.config, pc["B"]))
    feats = _teacher_forced(model, b)                         # (position 49 needs the 49 before it in the cache)
    gold = golden("caption_swin_b_576")
    n = feats.numel()
    assert n == int(gold["text_feats/numel"])
    idx = np.arange(n)[::max(1, n // 4096)][:4096]            # cases.summarize's sample
    assert np.array_equal(cases.summarize(feats)["sub"], feats.detach().float().cpu().reshape(-1).numpy()[idx])
    H = feats.shape[-1]
    pick = np.isin(idx // H, (0, 24, 49))
    assert pick.sum() >= 3 * (H // 16)
    got = torch.from_numpy(cases.summarize(feats)["sub"][pick])
    e = rel_l2(got, torch.from_numpy(gold["text_feats/sub"][pick]))
    print(f"teacher-forced caption_swin_b_576, positions 0 / 24 / 49: rel-L2 {e:.3e}")
    assert e <= 3e-2


def test_cached_beam3_decode_matches_reference(lib, golden):
    """caption_test_step with caption_decode_cache on caption_tiny, beam 3: beam 0's ids equal the reference's up to the first step whose
    recorded kept / dropped gap is below caption_cases.MARGIN -- test_beam3_decode_matches_reference's check on the cached path"""
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    from tests import caption_cases as cc
    gold = golden("caption_tiny")
    model, pc = _fixture("caption_tiny", caption_decode_cache=True)
    cc.sharpen_for_decode(model)
    ops.mark_weights_dirty()
    b = _to_dev(cc.batch_for(model.config, pc["B"], seed=cc.DECODE_SEED))
    calls = []
    inner = model.infer_caption
    model.infer_caption = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    out = objectives.caption_test_step(model, b, None, beam_size=int(gold["decode/beam"]))
    assert not calls, "the cached path ran infer_caption"
    ids = out["caption_ids"].clone()
    ids[(ids == 2) | (ids == 0)] = 1                                            # as the reference decodes them
    ref = torch.from_numpy(gold["decode/ids"])
    margins = gold["decode/margins"]
    prefixes = [cc.decode_prefix(list(margins[s]), ids.shape[1]) for s in range(ids.shape[0])]
    assert max(prefixes) >= 4
    for s, n in enumerate(prefixes):
        assert torch.equal(ids[s, :n].cpu(), ref[s, :n]), (s, n, ids[s].tolist(), ref[s].tolist())


def test_cached_greedy_decode_equals_full_recompute(lib):
    """Beam 1: the cached ids equal the cache-off ids over the steps where the full path's top-1 / top-2 logit gap exceeds MARGIN (a sample
    is compared up to its first step below it: past a flip the two paths decode different prefixes).  The full path's logits are taken
    from its own mlm_score calls; at most half the steps may be skipped."""
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    from tests import caption_cases as cc
    model, pc = _fixture("caption_tiny")
    cc.sharpen_for_decode(model)
    ops.mark_weights_dirty()
    b = _to_dev(cc.batch_for(model.config, pc["B"], seed=cc.DECODE_SEED))
    gaps = []

    def hook(m, i, o):
        x = o.detach().float()[:, 0].clone()
        x[:, model.config["vocab_size"] - 1] = -10000
        top = x.topk(2, -1).values
        gaps.append((top[:, 0] - top[:, 1]).cpu())
    h = model.mlm_score.register_forward_hook(hook)
    try:
        full = objectives.caption_test_step(model, dict(b), None, beam_size=1)["caption_ids"]
    finally:
        h.remove()
    model.hparams.config["caption_decode_cache"] = True
    try:
        cached = objectives.caption_test_step(model, dict(b), None, beam_size=1)["caption_ids"]
    finally:
        model.hparams.config["caption_decode_cache"] = False
    gaps = torch.stack(gaps, 1)                               # [B, steps run]
    steps = gaps.shape[1]
    compared = 0
    for s in range(full.shape[0]):
        n = next((i for i in range(steps) if gaps[s, i] <= cc.MARGIN), steps)
        compared += n
        assert torch.equal(cached[s, :n], full[s, :n]), (s, n, cached[s].tolist(), full[s].tolist())
    total = steps * full.shape[0]
    print(f"greedy decode: compared {compared} of {total} steps (skipped share {(total - compared) / total:.2f}), min gap {gaps.min():.3f}")
    assert total - compared <= total // 2


def test_cached_caption_sample(lib):
    """_caption_sample with the cache on, train mode, dropout 0: well-formed ids, the same key the same ids, [bs * beam, L], batch untouched"""
    import copy
    from fiber_amd import ops
    from fiber_amd.modules import objectives
    from tests import caption_cases as cc
    model, pc = _fixture("caption_tiny", train=True, caption_decode_cache=True, text_dropout=0.0, drop_path_rate=0.0)
    cc.sharpen_for_decode(model)
    ops.mark_weights_dirty()
    b = _to_dev(cc.batch_for(model.config, pc["B"], seed=cc.DECODE_SEED))
    keep = copy.deepcopy(b)
    tok = model.trainer.datamodule.dms[0].tokenizer
    L, beam = model.config["max_text_len"], 3
    out = []
    for seed in (7, 7, 8):
        ops.manual_seed(seed)
        out.append(objectives._caption_sample(model, tok, b["image"][0], None, beam, L))
    ids = out[0]
    assert tuple(ids.shape) == (pc["B"] * beam, L) and ids.dtype == torch.long
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    assert bool((ids[:, 0] == 0).all()) and not bool((ids == model.config["vocab_size"] - 1).any())
    for r in ids.tolist():                                    # after the first sep / pad only pads follow
        end = next((i for i, t in enumerate(r[1:], 1) if t in (1, 2)), L)
        assert all(t == 1 for t in r[end + 1:]), r
    for k in b:
        same = torch.equal(b[k], keep[k]) if torch.is_tensor(b[k]) else (torch.equal(b[k][0], keep[k][0]) if isinstance(b[k], list) and torch.is_tensor(b[k][0]) else b[k] == keep[k])
        assert same, k
