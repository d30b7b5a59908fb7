"""Helpers shared by the GPU parity tests."""
import math

import torch

DEV = "cuda"
BF = torch.bfloat16


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def assert_close(name, got, ref, tol):
    e = rel_l2(got, ref)
    assert e <= tol, f"{name}: rel-L2 {e:.3e} > {tol:.1e} (|ref|={ref.float().norm().item():.3e})"
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite values"
    return e


def bf(x):
    """Round an fp32 tensor to bf16 and move it to the GPU (test inputs are bf16-exact so that the fp32
    reference sees the same numbers as the kernel)."""
    return x.to(BF).to(DEV)


def load_from_oracle(product, oracle):
    """Copy the oracle's weights into the product module (rank_output aliases itm_score.fc rows, skip it)."""
    sd = {k: v for k, v in oracle.state_dict().items() if not k.startswith("rank_output.")}
    missing, unexpected = product.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("rank_output.") for k in missing), missing
    return product


def assert_elementwise(name, got, ref, bound, row0=0, tile=256):
    """Per-element check |got - ref| <= bound (bound: a tensor broadcastable to ref, or a scalar), all in fp64.  Unlike a
    whole-tensor norm it cannot average a wrong row, 8-column group or tile away.  On failure: the number of violations,
    the worst element (largest |got - ref| / bound) as (row, col) -- `row0` added, for callers that check row blocks --
    and the tile of `tile` x `tile` it lies in.  Returns the largest |got - ref| / bound."""
    ref = ref.detach().to(torch.float64)
    got = got.detach().to(device=ref.device, dtype=torch.float64)
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if not torch.is_tensor(bound):
        bound = torch.tensor(float(bound), dtype=torch.float64)
    bound = bound.detach().to(device=ref.device, dtype=torch.float64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    ratio = (err / bound.clamp_min(1e-300)).reshape(-1, ref.shape[-1] if ref.dim() else 1)
    bad = int((err > bound).sum().item())
    worst = int(ratio.argmax().item())
    r, c = divmod(worst, ratio.shape[1])
    worst_ratio = ratio.view(-1)[worst].item()
    if bad:
        e2, b2 = err.reshape(ratio.shape), bound.expand_as(ref).reshape(ratio.shape)
        raise AssertionError(
            f"{name}: {bad} of {ref.numel()} elements outside the bound; worst at (row {row0 + r}, col {c}) = tile "
            f"({(row0 + r) // tile}, {c // tile}) of {tile}x{tile}: got {got.reshape(ratio.shape)[r, c].item():.6g}, "
            f"ref {ref.reshape(ratio.shape)[r, c].item():.6g}, |err| {e2[r, c].item():.3g} > bound {b2[r, c].item():.3g} "
            f"({worst_ratio:.3g}x)")
    return worst_ratio


def abs_mm64(x, w, rows=16384):
    """|X| . |W|^T in fp64 ([M, K] x [N, K] -> [M, N]), on the operands' device, `rows` rows of X at a time: the scale of the
    rounding error of an fp32 accumulation of X . W^T: |fl(sum) - sum| <= c * sum |x_k w_k|, c depending on K and the order."""
    wa = w.detach().to(torch.float64).abs().t()
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], rows):
        out[i:i + rows] = x[i:i + rows].detach().to(torch.float64).abs() @ wa
    return out


def mm64(x, w, rows=16384):
    """X . W^T in fp64 ([M, K] x [N, K] -> [M, N]) on the operands' device, `rows` rows of X at a time."""
    wt = w.detach().to(torch.float64).t()
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], rows):
        out[i:i + rows] = x[i:i + rows].detach().to(torch.float64) @ wt
    return out
