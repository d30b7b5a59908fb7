"""The per-element LayerNorm-family bounds of tests/norm_cases.py on the host.  The whole-tensor rel-L2 thresholds of the existing tests
(4e-3 on the fused LN-Mlp output and on LayerNorm y, 3e-3 on the fp32-stream LayerNorm) accept each of five local mutations of an
fp64 result -- one row of a ragged last strip wrong, one 8-channel group of a padded-lane width wrong, the next sample's DropPath scale
on the rows of a strip that spans two samples, one 16-unit hidden group in logical instead of the kernels' order, a one-pass variance
on the large-mean rows -- and assert_elementwise with the bounds the GPU tests use rejects each one.  The same bounds accept an fp32
emulation of the kernels' formulas: two-pass fp32 statistics and the same bf16 rounding points."""
import pytest
import torch

from tests import norm_cases as nc
from tests.hip_util import assert_close, assert_elementwise

K = nc.CONST


def bound(spec):
    base, terms = spec
    return base + sum(K[c] * t for c, t in terms.items())


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _mlp_host(name, C, M, rps):
    """a fused LN-Mlp case on the host with a small branch (W2 / 32), so that a local error stays under the rel-L2 thresholds"""
    case = nc._mlp(name, C, M, rps=rps)
    inp = nc.make_mlp_inputs(case, device="cpu")
    inp["w2"] = (inp["w2"].float() / 32).to(torch.bfloat16)
    inp["b2"] = inp["b2"] / 32
    return case, inp


@pytest.fixture(scope="module")
def mlp():
    case, inp = _mlp_host("host-mlp", 128, 1400, 200)
    out, bd = nc.mlp_reference(case, inp, 0, case["M"])
    return case, inp, out, bd


def _emul_mlp32(case, inp):
    """the fused kernels' formulas in fp32 with their bf16 roundings (xhat, G, dH, outputs)"""
    f = torch.float32
    x = inp["x"].to(f)
    C = x.shape[1]
    mu = x.sum(1, keepdim=True) / C
    xc = x - mu
    rstd = torch.rsqrt((xc * xc).sum(1, keepdim=True) / C + case["eps"])
    xr = (xc * rstd).to(torch.bfloat16).to(f)
    Hm = xr @ inp["w1p"].to(f).t() + inp["b1p"]
    G = torch.nn.functional.gelu(Hm).to(torch.bfloat16).to(f)
    s = inp["rowscale"][torch.arange(case["M"]) // case["rps"]][:, None]
    y = x + s * (G @ inp["w2"].to(f).t() + inp["b2"])
    dy = inp["dy"].to(f)
    dG = dy @ inp["w2"].to(f)
    t = Hm
    gp = 0.5 * (1 + torch.erf(t * 0.5 ** 0.5)) + t * torch.exp(-0.5 * t * t) * 0.3989422804014327
    dH = (s * dG * gp).to(torch.bfloat16).to(f)
    a = dH @ inp["w1p"].to(f)
    s1 = a.mean(1, keepdim=True)
    s2 = (a * xr).mean(1, keepdim=True)
    dx = dy + rstd * (a - s1 - xr * s2)
    return dict(y=bf16(y), g=bf16(G), xhat=bf16(xc * rstd), dh=bf16(dH), dx=bf16(dx))


def test_mlp_bounds_accept_fp32_emulation(mlp):
    case, inp, out, bd = mlp
    em = _emul_mlp32(case, inp)
    for k in ("y", "g", "xhat", "dh", "dx"):
        assert_elementwise(f"fp32 emulation {k}", em[k], out[k], bound(bd[k]))


def test_ragged_last_strip_row_wrong(mlp):
    case, inp, out, bd = mlp
    M = case["M"]                                           # 1400 = 43 strips + 24 rows
    bad = bf16(out["y"]).clone()
    x = inp["x"].double()
    bad[M - 1] = bf16(x[M - 1] + out["y"][M - 2] - x[M - 2])  # the last row of the ragged strip takes its neighbour's branch
    e = assert_close("y, one row of the last strip", bad, out["y"], 4e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("y, one row of the last strip", bad, out["y"], bound(bd["y"]))
    print(f"one row of a ragged last strip wrong: rel-L2 {e:.2e} accepted at 4e-3")


def test_next_sample_scale_on_a_spanning_strip(mlp):
    case, inp, out, bd = mlp
    # strip 6 = rows 192 .. 223 spans samples 0 (rows < 200, scale 1.25) and 1 (dropped): rows 192 .. 199 get sample 1's scale 0
    x = inp["x"].double()
    bad = bf16(out["y"]).clone()
    bad[192:200] = bf16(x[192:200])
    e = assert_close("y, strip spanning two samples", bad, out["y"], 4e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("y, strip spanning two samples", bad, out["y"], bound(bd["y"]))
    print(f"next sample's DropPath scale on a spanning strip: rel-L2 {e:.2e} accepted at 4e-3")


def test_hidden_group_in_logical_order(mlp):
    case, inp, out, bd = mlp
    H = 4 * case["C"]
    order = torch.arange(H)
    a = 21                                                   # hidden units 336 .. 351 (chunk 5)
    order[16 * a:16 * a + 16] = 16 * a + nc.fa_perm(16, "cpu")
    alt, _ = nc.mlp_reference(case, inp, 0, case["M"], want_bwd=False, hid_order=order)
    bad = bf16(alt["y"])
    e = assert_close("y, one hidden group in logical order", bad, out["y"], 4e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("y, one hidden group in logical order", bad, out["y"], bound(bd["y"]))
    print(f"one 16-unit hidden group in logical order: rel-L2 {e:.2e} accepted at 4e-3")


def _ln_host(name, C, rows, x32=False, dist="normal"):
    case = nc._ln(name, C, rows, x32=x32, dist=dist)
    inp = nc.make_ln_inputs(case, device="cpu")
    return case, inp


def test_ln_bounds_accept_fp32_emulation():
    for case, inp in (_ln_host("host-ln96", 96, 517), _ln_host("host-s32", 512, 300, x32=True, dist="bigmean"),
                      _ln_host("host-ln1536", 1536, 40)):
        out, bd = nc.ln_fwd_reference(inp["x"], inp["gamma"], inp["beta"], case["eps"])
        em, _ = nc.ln_fwd_reference(inp["x"], inp["gamma"], inp["beta"], case["eps"], dtype=torch.float32)
        assert_elementwise(f"{case['name']} fp32 y", bf16(em["y"]), out["y"], bound(bd["y"]))
        assert_elementwise(f"{case['name']} fp32 y32", em["y"].double(), out["y"], bound(bd["y32"]))
        assert_elementwise(f"{case['name']} fp32 mean", em["mean"].double()[:, None], out["mean"][:, None],
                           bound((bd["mean"][0][:, None], {"STAT": bd["mean"][1]["STAT"][:, None]})))
        mean, rstd = em["mean"], em["rstd"]
        ob, bb = nc.ln_bwd_reference(inp["x"], inp["dy"], inp["gamma"], mean, rstd, inp.get("dres"), case)
        eb, _ = nc.ln_bwd_reference(inp["x"], inp["dy"], inp["gamma"], mean, rstd, inp.get("dres"), case, dtype=torch.float32)
        assert_elementwise(f"{case['name']} fp32 dx", bf16(eb["dx"]), ob["dx"], bound(bb["dx"]))
        for k in ("dgamma", "dbeta"):
            assert_elementwise(f"{case['name']} fp32 {k}", eb[k].double()[:, None], ob[k][:, None],
                               bound((bb[k][0][:, None], {c: t[:, None] for c, t in bb[k][1].items()})))


def test_padded_lane_group_wrong():
    case, inp = _ln_host("host-ln96", 96, 517)               # nvec = 12 of 16 lanes per row: the last group is next to the padding
    out, bd = nc.ln_fwd_reference(inp["x"], inp["gamma"], inp["beta"], case["eps"])
    bad = bf16(out["y"]).clone()
    bad[300, 88:96] = bf16(out["y"][300, 88:96] - inp["beta"][88:96].double())   # one row's last 8-channel group without beta
    e = assert_close("y, one 8-channel group", bad, out["y"], 4e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("y, one 8-channel group", bad, out["y"], bound(bd["y"]))
    print(f"one 8-channel group of C = 96 wrong: rel-L2 {e:.2e} accepted at 4e-3")


def test_one_pass_variance_on_large_mean_rows():
    rows, C = 131072, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    # one row of large mean and small spread: variance 0.25, of which E[x^2] - E[x]^2 in fp32 keeps only a few bits (2^-24 of 1e6)
    x[777] = 1000.0 + 0.5 * torch.randn(C, generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    out, bd = nc.ln_fwd_reference(x, gamma, beta, 1e-5)
    m = x.mean(1, keepdim=True)
    var1 = ((x * x).mean(1, keepdim=True) - m * m).clamp_min(0)           # E[x^2] - E[x]^2 in fp32
    y1 = ((x - m) * torch.rsqrt(var1 + 1e-5) * gamma + beta).double()
    e = assert_close("y32, one-pass variance", y1, out["y"], 3e-3)
    with pytest.raises(AssertionError):
        assert_elementwise("y32, one-pass variance", y1, out["y"], bound(bd["y32"]))
    em, _ = nc.ln_fwd_reference(x, gamma, beta, 1e-5, dtype=torch.float32)     # the two-pass form passes
    assert_elementwise("y32, two-pass fp32", em["y"].double(), out["y"], bound(bd["y32"]))
    print(f"one-pass variance on one large-mean row: rel-L2 {e:.2e} accepted at 3e-3")
