"""Cases, fp64 restatement and bounds of the grounding head's alignment + token focal loss (csrc/ground.hip, ops.ground_logits,
ops.ground_token_loss).  The restatement is vldyhead.py:857-891 and sigmoid_focal_loss.py:130-171 (version "binary") in fp64 on the
kernel's own rounded inputs (bf16 X and P, fp32 tbias / log_scale), in the stable form ce = softplus(-z), 1 - p_t = sigmoid(-z) with
z = +s for target 1 and -s for target 0.  tests/test_ground_compare_host.py holds it against fixtures the reference's own functions
produced (tools/gen_ground_golden.py); tests/test_hip_ground.py holds the kernels against it element by element.

Bounds (needed on MI355X in brackets; next power of two at or above the worst observed, FIBER_GROUND_CALIBRATE=<file> writes them):
  logits   |got - ref| <= K_ACC * sum_k |x_k p_k| * inv_scale + 2^-23 |ref|.  K_ACC may not exceed 2^-16 (256 sequential fp32 adds of
           exact bf16 x bf16 products: 256 * 2^-24); the second term is the fp32 rounding of acc * inv_scale + tbias and of the store,
           which the first cannot carry where tbias dominates a small dot product.
  ds       |got - ref| <= 2^-8 |ref| (bf16 store) + DS * |g| * alpha_t (fast exp / log / rcp of the epilogue); the kernel stores
           ds * inv_scale (the gradient of the raw dot product), so both sides of this bound are scaled by inv_scale.
  sums     |got - ref| <= SUM * sum |terms| for the loss, dtbias and dlog_scale (ew_cases.py's SUM convention).
"""
import math
import types

import numpy as np
import torch

from oracle import detgen

C = T = 256
LANG_DIM = 768
CLAMP = 50000.0

CONST = {
    "K_ACC": 2.0 ** -23,   # fp32 MFMA accumulation of 256 exact products + fp32 exp(-log_scale) (2^-23.22, full geometry); ceiling 2^-16
    "DS": 2.0 ** -24,      # v_exp / v_log / v_rcp of the epilogue, beside the bf16 store term (0: that term covered every element of every case)
    "SUM": 2.0 ** -18,     # lane -> wave -> workgroup -> fold sums incl. the fast transcendentals of their terms (2^-18.37, dtbias at A = 1: one term)
}
HOST = 2.0 ** -20          # fp32 (reference run) against fp64 of the same formula, in units of sum |terms|

SMALL = dict(B=2, sizes=[(20, 28), (10, 14), (5, 7)], convs=2, lens=[256, 37], alpha=0.25, gamma=2.0, num_pos=11.0, log_scale=0.3)
A_SMALL = sum(h * w for h, w in SMALL["sizes"])          # 735 = 11 * 64 + 31: not a tile multiple
A_LOSS_ONLY = 805                                        # rows of the logits-given case
FULL_SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
A_FULL = sum(h * w for h, w in FULL_SIZES)               # 22 400 anchors at the 800 x 1344 detection geometry
KEEP_CHANNELS, KEEP_TOKENS, KEEP_WROWS = 32, 48, 64      # what tools/gen_ground_golden.py keeps of dX, d embedding, d projection weight
LOSS_ONLY_HYPER = [(g, a) for g in (2.0, 1.5, 0.0) for a in (0.25, -1.0)]


def _randn(name, shape, std=1.0):
    g = detgen._rng("ground:" + name, 0)
    return torch.from_numpy((g.standard_normal(shape) * std).astype(np.float32))


def text_mask(B, lens, name):
    """uint8 [B, T]: live up to the text length, with zeros in the middle of every text as well as at the tail"""
    m = torch.zeros((B, T), dtype=torch.uint8)
    for b, L in enumerate(lens):
        m[b, :L] = 1
        lo = max(1, L // 3)
        m[b, lo:lo + max(2, L // 10)] = 0
    return m


def targets(B, A, lens, name, empty_image=None, frac=0.01):
    """uint8 [B, A, T]: about 1 % positives inside the text length, one anchor with several positive tokens, image `empty_image` with none"""
    g = detgen._rng("ground:targets:" + name, 0)
    t = torch.from_numpy((g.random((B, A, T)) < frac).astype(np.uint8))
    for b, L in enumerate(lens):
        t[b, :, L:] = 0
    t[0, min(3, A - 1), 2:9] = 1
    if empty_image is not None:
        t[empty_image] = 0
    return t


def kernel_case(name, B, A, lens=None, log_scale=0.3, xstd=1.0, pstd=0.25, empty_image=None):
    """Direct kernel inputs: bf16-exact X [B, A, C] and P [B, T, C], fp32 tbias, log_scale, targets, mask."""
    lens = lens or [T] + [37] * (B - 1)
    return dict(x=_randn(name + ".x", (B, A, C), xstd).to(torch.bfloat16), p=_randn(name + ".p", (B, T, C), pstd).to(torch.bfloat16),
                tbias=_randn(name + ".tb", (B, T), 1.0) - 2.0, log_scale=torch.tensor([log_scale], dtype=torch.float32),
                targets=targets(B, A, lens, name, empty_image), mask=text_mask(B, lens, name))


def loss_only_case():
    """Logits given directly [2, 805, 256] spanning +-60 (both saturated tails of softplus), a few beyond +-50000 before the clamp."""
    g = detgen._rng("ground:loss_only.logits", 0)
    lg = torch.from_numpy((g.random((2, A_LOSS_ONLY, T)) * 120.0 - 60.0).astype(np.float32))
    lg[0, 5, 7], lg[0, 5, 8], lg[1, 700, 3], lg[1, 11, 20] = 7.0e4, -6.5e4, 1.0e5, -5.0001e4
    lens = [T, 37]
    tg = targets(2, A_LOSS_ONLY, lens, "loss_only", frac=0.05)
    tg[0, 5, 7] = 1                                         # a clamped positive and clamped negatives
    return dict(logits=lg, targets=tg, mask=text_mask(2, lens, "loss_only"))


# ---- the head's configuration node tree (what VLDyHead(cfg) reads) ------------------------------------------------------------------
def head_cfg(convs=2, in_channels=C, **fuse):
    ns = types.SimpleNamespace
    fc = dict(TYPE="NONE", EARLY_FUSE_ON=False, USE_TOKEN_LOSS=False, USE_CONTRASTIVE_ALIGN_LOSS=False, USE_DOT_PRODUCT_TOKEN_LOSS=True,
              USE_SHALLOW_CONTRASTIVE_LOSS=False, USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS=False, MLM_LOSS=False,
              USE_FUSED_FEATURES_DOT_PRODUCT=False, CLAMP_DOT_PRODUCT=True, CONTRASTIVE_HIDDEN_DIM=64,
              CLAMP_BERTATTN_MIN_FOR_UNDERFLOW=True, CLAMP_BERTATTN_MAX_FOR_OVERFLOW=True)
    fc.update(fuse)
    return ns(MODEL=ns(
        LANGUAGE_BACKBONE=ns(MODEL_TYPE="roberta-fused", MAX_QUERY_LEN=T, LANG_DIM=LANG_DIM),
        DYHEAD=ns(NUM_CLASSES=2, CHANNELS=C, USE_GN=True, USE_NSYNCBN=False, USE_SYNCBN=False, USE_DYRELU=True, USE_DYFUSE=True,
                  USE_DFCONV=True, CONV_FUNC="", NUM_CONVS=convs, PRIOR_PROB=0.01, LOG_SCALE=0.0, FUSE_CONFIG=ns(**fc)),
        RPN=ns(ASPECT_RATIOS=(1.0,), SCALES_PER_OCTAVE=1, RETURN_FUSED_FEATURES=False),
        BACKBONE=ns(OUT_CHANNELS=in_channels), GROUP_NORM=ns(NUM_GROUPS=16), FOCAL=ns(LOSS_ALPHA=0.25, LOSS_GAMMA=2.0)))


def set_head_weights(model, name="ground_small"):
    """Deterministic values by parameter name (tower: as oracle/gen_dyhead_golden.py, offsets with a non-trivial spread; zero
    initialisations -- bias_lang, biases -- non-zero); GEMM operands of the tower bf16-exact."""
    with torch.no_grad():
        for k, p in model.named_parameters():
            g = detgen._rng(f"ground:{name}:{k}", 0)
            n = lambda std: torch.from_numpy((std * g.standard_normal(tuple(p.shape))).astype(np.float32))   # noqa: E731
            if k == "log_scale":
                p.fill_(SMALL["log_scale"])
            elif k == "bias0":
                p.fill_(-2.0)
            elif k == "bias_lang":
                p.copy_(n(0.5))
            elif k.startswith("scales."):
                p.copy_(1.0 + n(0.2))
            elif k.startswith("dot_product_projection_text.weight"):
                p.copy_(n(0.6))
            elif k.endswith("offset.weight"):
                p.copy_(n(0.05))
            elif k.endswith("offset.bias"):
                p.copy_(n(0.3))
            elif k.endswith(".bn.weight"):
                p.copy_(1.0 + n(0.1))
            elif k.endswith("bias"):
                p.copy_(n(0.05))
            else:
                p.copy_(n(1.0 / (p[0].numel() ** 0.5) if p.dim() > 1 else 0.1))
        for k, p in model.named_parameters():
            if k.endswith("conv.weight") or k.endswith("offset.weight"):
                p.copy_(p.to(torch.bfloat16).float())


def small_inputs():
    c = SMALL
    xs = [_randn(f"small.x{i}", (c["B"], C, h, w)).to(torch.bfloat16).float() for i, (h, w) in enumerate(c["sizes"])]
    emb = _randn("small.embedding", (c["B"], T, LANG_DIM))
    return xs, emb, targets(c["B"], A_SMALL, c["lens"], "small", empty_image=1), text_mask(c["B"], c["lens"], "small")


# ---- fp64 restatement -------------------------------------------------------------------------------------------------------------
def align64(x, p, tbias, log_scale):
    """-> (s clamped, s - tbias unclamped, sum_k |x_k p_k| * inv_scale), fp64 on the inputs' device"""
    x, p = x.detach().double(), p.detach().double()
    inv = torch.exp(-log_scale.detach().double().reshape(()))
    un = torch.matmul(x, p.transpose(1, 2)) * inv
    mag = torch.matmul(x.abs(), p.abs().transpose(1, 2)) * inv
    return (un + tbias.detach().double()[:, None, :]).clamp(-CLAMP, CLAMP), un, mag


def _softplus(v):
    return torch.nn.functional.softplus(v, threshold=700.0)     # (the default switches to the identity at 20: 2e-9 off in fp64)


def alpha_t(tg, alpha):
    pos = tg != 0
    if alpha < 0:
        return torch.ones(tg.shape, dtype=torch.float64, device=tg.device)
    return torch.where(pos, alpha, 1.0 - alpha).double()


def focal64(s, tg, mask, alpha, gamma):
    """Per-element loss of s (fp64, differentiable) with masked tokens at zero: [B, A, T]"""
    sp = _softplus
    z = torch.where(tg != 0, s, -s)
    loss = alpha_t(tg, alpha) * sp(-z) * torch.exp(-gamma * sp(z))
    return loss * (mask > 0)[:, None, :].double()


def focal_grad64(s, tg, mask, alpha, gamma):
    """dloss/ds per element: -alpha_t (1 - p_t)^gamma [(1 - p_t) + gamma p_t softplus(-z)], sign by target, zero on masked tokens"""
    sp = _softplus
    pos = tg != 0
    z = torch.where(pos, s, -s)
    dz = -alpha_t(tg, alpha) * torch.exp(-gamma * sp(z)) * (torch.sigmoid(-z) + gamma * torch.sigmoid(z) * sp(-z))
    return torch.where(pos, dz, -dz) * (mask > 0)[:, None, :].double()


def backward64(x, p, tbias, log_scale, tg, mask, alpha, gamma, g=1.0):
    """-> dict(s, mag, loss_el, ds, dtbias, dlog_scale, and the sum |terms| of each reduction); ds zero where the clamp is active"""
    s, un, mag = align64(x, p, tbias, log_scale)
    inv = torch.exp(-log_scale.detach().double().reshape(()))
    su = un + tbias.detach().double()[:, None, :]
    ds = g * focal_grad64(s, tg, mask, alpha, gamma) * ((su >= -CLAMP) & (su <= CLAMP)).double()
    le = focal64(s, tg, mask, alpha, gamma)
    return dict(s=s, mag=mag, loss_el=le, loss=le.sum(), ds=ds, dtbias=ds.sum(1), dtbias_abs=ds.abs().sum(1),
                dlog_scale=-(ds * un).sum(), dlog_scale_abs=(ds * un).abs().sum(),
                inv=inv, dq=ds * inv,                     # dq: gradient of the raw dot product, what the kernel stores (bf16) for the GEMMs
                dx=torch.matmul(ds * inv, p.detach().double()), dp=torch.matmul((ds * inv).transpose(1, 2), x.detach().double()))


def logit_bound(mag, ref, k=None):
    return (CONST["K_ACC"] if k is None else k) * mag + 2.0 ** -23 * ref.abs()


def ds_bound(ref, tg, alpha, g=1.0, k=None):
    return 2.0 ** -8 * ref.abs() + (CONST["DS"] if k is None else k) * abs(g) * alpha_t(tg, alpha)


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def within(got, ref, bound):
    return bool(((got.double() - ref.double()).abs() <= bound).all())


assert A_SMALL == 735 and A_FULL == 22400
