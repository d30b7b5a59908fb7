"""The per-element attention bounds of tests/attn_cases.py on the host.  The whole-tensor rel-L2 thresholds of the existing attention
tests (5e-3 on O, 1e-2 on the gradients) accept each of four local mutations of an fp64 result -- one window without its shift mask,
one 16-query strip without its last 160-key chunk, one sample's key mask ignored in one head's dK, two mirrored dbias_table entries of
one head swapped -- and assert_elementwise with the bounds the GPU tests use rejects each one.  The same bounds accept the fp64 result
rounded to bf16 and an fp32 computation of the same formulas."""
import pytest
import torch

from tests import attn_cases as ac
from tests.hip_util import assert_close, assert_elementwise

C = ac.CONST


def bound(terms):
    base, tt = terms
    return base + sum(C[c] * t for c, t in tt.items())


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


@pytest.fixture(scope="module")
def win():
    """4 x 4 windows, shift 1, one head: 40000 windows"""
    case = ac._win("host-w4", 10, 320, 200, 1, 4, 1)
    inp = ac.make_window_inputs(case, device="cpu")
    ref, trm = ac.window_reference(case, inp)
    return case, inp, ref, trm


def test_window_bounds_accept_rounding_and_fp32(win):
    case, inp, ref, trm = win
    f32, _ = ac.window_reference(case, inp, dtype=torch.float32)     # the same formulas computed in fp32
    for k in ("o", "dq", "dk", "dv"):
        assert_elementwise(f"bf16({k})", bf16(ref[k]), ref[k], bound(trm[k]))
        assert_elementwise(f"bf16(fp32 {k})", bf16(f32[k]), ref[k], bound(trm[k]))
    assert_elementwise("fp32 dtable", f32["dtable"], ref["dtable"], bound(trm["dtable"]))


def test_window_without_shift_mask(win):
    case, inp, ref, trm = win
    nW = (case["H"] // 4) * (case["W"] // 4)
    g = nW - 2                                               # a window of the last window row of image 0 (two shift regions)
    one = dict(inp, tok=inp["tok"][g:g + 1], lab=torch.zeros_like(inp["lab"][g:g + 1]))
    alt, _ = ac.window_reference(case, one)
    t = inp["tok"][g]
    bad = bf16(ref["o"]).clone()
    bad[t] = bf16(alt["o"][t])
    e = assert_close("O, one window unmasked", bad, ref["o"], 5e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("O, one window unmasked", bad, ref["o"], bound(trm["o"]))
    print(f"window without its shift mask: rel-L2 {e:.2e} accepted at 5e-3")


def _mha_case(name, B, heads, Lq, Lk, mask):
    case = ac._mha(name, B, heads, Lq, Lk, 32, [], [], mask=mask)
    inp = ac.make_mha_inputs(case, device="cpu")
    return case, inp


def test_strip_without_last_chunk():
    case, inp = _mha_case("host-strip", 4, 12, 432, 165, "none")
    out, terms = ac.mha_reference(case, inp)
    B, H, Lq, Lk = 4, 12, 432, 165
    # strip 5 of head 7 of sample 2 computed from keys [0, 160) only
    q, k, v = (inp[n][:, :H * 32].double().view(B, -1, H, 32).permute(0, 2, 1, 3) for n in ("q", "k", "v"))
    s = inp["scale"] * q[2, 7, 80:96] @ k[2, 7, :160].T
    o_cut = torch.softmax(s, -1) @ v[2, 7, :160]
    bad = bf16(out["O"]).clone()
    bad[2, 7, 80:96] = bf16(o_cut)
    e = assert_close("O, one strip lost its last chunk", bad, out["O"], 5e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("O, one strip lost its last chunk", bad, out["O"], bound(terms["O"]))
    print(f"strip without its last key chunk: rel-L2 {e:.2e} accepted at 5e-3")


def test_key_mask_ignored_in_one_head():
    case, inp = _mha_case("host-kmask", 16, 12, 40, 40, "pad")
    inp["kmask"].zero_()
    inp["kmask"][3, -1] = -10000.0                          # sample 3 pads its last key
    out, terms = ac.mha_reference(case, inp)
    inp2 = dict(inp, kmask=torch.zeros_like(inp["kmask"]))
    alt, _ = ac.mha_reference(case, inp2)
    bad = bf16(out["dK"]).clone()
    bad[3, 5] = bf16(alt["dK"][3, 5])
    e = assert_close("dK, one head ignores the mask", bad, out["dK"], 1e-2)
    with pytest.raises(AssertionError):
        assert_elementwise("dK, one head ignores the mask", bad, out["dK"], bound(terms["dK"]))
    print(f"key mask ignored in one head's dK: rel-L2 {e:.2e} accepted at 1e-2")


def test_dbias_mirrored_entries_swapped():
    case = ac._win("host-w12", 2, 48, 48, 16, 12, 6)
    inp = ac.make_window_inputs(case, device="cpu")
    ref, trm = ac.window_reference(case, inp)
    d = ref["dtable"]
    nt = d.shape[0]
    h = 9
    diff = (d[:, h] - d.flip(0)[:, h]).abs()[:nt // 2]       # entry e = (dr, dc) and nt - 1 - e = (-dr, -dc): pairs (i, j) <-> (j, i)
    e0 = int(diff.argsort()[len(diff) // 2])                 # a pair of median difference
    bad = d.float().double().clone()
    bad[e0, h], bad[nt - 1 - e0, h] = d[nt - 1 - e0, h], d[e0, h]
    e = assert_close("dbias_table, one head's (i, j) <-> (j, i)", bad, d, 1e-2)
    with pytest.raises(AssertionError):
        assert_elementwise("dbias_table swapped", bad, d, bound(trm["dtable"]))
    print(f"mirrored dbias_table entries swapped: rel-L2 {e:.2e} accepted at 1e-2")


def test_mha_bounds_accept_rounding_and_fp32():
    case, inp = _mha_case("host-fp32", 3, 4, 64, 200, "pad")
    out, terms = ac.mha_reference(case, inp)
    B, H, D = 3, 4, 32
    cv = lambda x, L: x[:, :H * D].view(B, L, H, D).permute(0, 2, 1, 3)
    add = inp["kmask"][:, None, None, :].double()
    f32, _ = ac.attention64(cv(inp["q"], 64), cv(inp["k"], 200), cv(inp["v"], 200), add, cv(inp["do"], 64), inp["scale"],
                            dtype=torch.float32)
    for k in ("O", "dQ", "dK", "dV"):
        b = bound(terms[k])
        assert_elementwise(f"bf16({k})", bf16(out[k]), out[k], b)
        assert_elementwise(f"bf16(fp32 {k})", bf16(f32[k]), out[k], b)
    assert_elementwise("fp32 lse", f32["lse"], out["lse"], bound(terms["lse"]))
