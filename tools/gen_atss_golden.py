"""Generate tests/golden/atss_*.npz by executing the REFERENCE's grounding-training loss on the CPU (runs where the reference tree is present):

    python tools/gen_atss_golden.py            # the committed seeds of tests/atss_cases.py; asserts the margins, prints the constants
    python tools/gen_atss_golden.py --search   # per case, the first seed (of a few hundred) whose margins hold

Executed by path behind stub parents, unmodified: modeling/rpn/loss.py (ATSSLossComputation.prepare_targets, GIoULoss,
compute_centerness_targets, __call__), modeling/box_coder.py, modeling/utils.py, structures/boxlist_ops.py and structures/bounding_box.py.
The stubs carry no arithmetic of the path under test: `transformers.AutoTokenizer` is a class whose from_pretrained returns None
(captions=None never touches it; nothing reaches for a network), the comm helpers are world size 1, custom_fwd is the identity, Matcher
and the samplers are empty, and SigmoidFocalLoss returns 0 * logits.sum() (the classification loss is out of scope: the model multiplies
it by 0.0).  The token loss is computed by tools/gen_ground_golden.py's fixtures, not here: the configuration given to the reference has
both token-loss switches off, and prepare_targets still returns the token labels.

Inputs by name from tests/atss_cases.py (the fixtures hold outputs only).  Discrete outputs are only comparable where the reference
itself is decisive, so everything is also evaluated in fp64 (atss_cases.assign_torch / losses_torch) and the margins of atss_cases.MARGINS
are asserted and stored: the distance gap across every top-k cut, |iou - (mean + std)| of every candidate, |min(l, t, r, b) - 0.01|, the
best-versus-second IoU gap of multiply-positive anchors, and the distance of every max / min / clamp argument pair of the loss from its kink.
No anchor is excluded from any comparison; where a seed violates a margin another seed is searched, never a looser margin.
`matched` is not something the reference returns: it is recovered from its reg_targets (the gt whose encode by the reference's own
BoxCoder against the anchor equals the stored code bit for bit; identical boxes: the lowest index).
The constants of atss_cases.MEASURED are printed: what the reference's fp32 outputs need against the fp64 evaluation.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import shim                                      # noqa: E402
from tests import atss_cases as ac                           # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference():
    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m
    for n in ("maskrcnn_benchmark", "maskrcnn_benchmark.structures", "maskrcnn_benchmark.modeling", "maskrcnn_benchmark.modeling.rpn",
              "maskrcnn_benchmark.utils"):
        pkg(n)

    class _Zero:
        def __init__(self, *a, **k):
            pass

        def __call__(self, logits, *a, **k):
            return 0.0 * logits.sum()

    layers = pkg("maskrcnn_benchmark.layers")
    layers.nms = layers.ml_nms = layers.smooth_l1_loss = None
    layers.SigmoidFocalLoss = layers.IOULoss = layers.TokenSigmoidFocalLoss = _Zero
    pkg("maskrcnn_benchmark.modeling.matcher").Matcher = _Zero
    pkg("maskrcnn_benchmark.modeling.balanced_positive_negative_sampler").BalancedPositiveNegativeSampler = _Zero
    comm = pkg("maskrcnn_benchmark.utils.comm")
    comm.get_world_size, comm.reduce_sum = (lambda: 1), (lambda t: t)
    amp = pkg("maskrcnn_benchmark.utils.amp")
    amp.custom_fwd = lambda **k: (lambda f: f)
    amp.custom_bwd = lambda f: f
    pkg("maskrcnn_benchmark.utils.shallow_contrastive_loss_helper").__all__ = []
    real_tf = sys.modules.get("transformers")
    tf = types.ModuleType("transformers")
    tf.AutoTokenizer = type("AutoTokenizer", (), {"from_pretrained": staticmethod(lambda *a, **k: None)})
    sys.modules["transformers"] = tf
    try:
        s, m = "maskrcnn_benchmark.structures", "maskrcnn_benchmark.modeling"
        bb = shim._load("bounding_box", os.path.join(MB, "structures", "bounding_box.py"), s)
        shim._load("boxlist_ops", os.path.join(MB, "structures", "boxlist_ops.py"), s)
        bc = shim._load("box_coder", os.path.join(MB, "modeling", "box_coder.py"), m)
        shim._load("utils", os.path.join(MB, "modeling", "utils.py"), m)
        loss = shim._load("loss", os.path.join(MB, "modeling", "rpn", "loss.py"), m + ".rpn")
    finally:
        if real_tf is not None:
            sys.modules["transformers"] = real_tf
        else:
            del sys.modules["transformers"]
    return loss, bc, bb


def ref_cfg():
    ns = types.SimpleNamespace
    c = ac.cfg()
    c.MODEL.FOCAL = ns(LOSS_GAMMA=2.0, LOSS_ALPHA=0.25, FG_IOU_THRESHOLD=0.5, BG_IOU_THRESHOLD=0.4)
    c.MODEL.LANGUAGE_BACKBONE = ns(MODEL_TYPE="roberta-fused", TOKENIZER_TYPE="roberta-base")
    c.MODEL.DYHEAD = ns(FUSE_CONFIG=ns(USE_TOKEN_LOSS=False, USE_DOT_PRODUCT_TOKEN_LOSS=False, USE_SHALLOW_CONTRASTIVE_LOSS=False,
                                       USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS=False, USE_CONTRASTIVE_ALIGN_LOSS=False, MLM_LOSS=False))
    return c


def evaluate(case, seed=None):
    """fp64 evaluation -> (inputs with the edge marks, targets, assignment, losses, margins)"""
    x = ac.inputs(case, seed)
    t = ac.packed(case, x)
    a = ac.assign_torch(ac.anchors(), t)
    try:
        x = ac.mark_edge(case, x, a["matched"])
    except AssertionError:
        return x, t, a, None, dict(a["margins"], kink=-1.0)
    l64 = ac.losses_torch(x["bbox_reg"], x["centerness"], ac.anchors(), a["labels"], a["reg_targets"], grads=grads_for(a, None))
    return x, t, a, l64, dict(a["margins"], kink=l64["kink"])


def grads_for(a, l64):
    """upstream gradients of the three sums under loss_reg + loss_centerness (world size 1); l64 None: placeholders for the margins run"""
    n = max(float(a["num_pos"].sum()), 1.0)
    if l64 is None:
        return (1.0, 0.0, 1.0 / n)
    s = float(l64["sums"][1])
    return (ac.REG_LOSS_WEIGHT / s if s > 0 else 0.0, 0.0, 1.0 / n)


def margins_ok(m):
    return all(m[k] >= v for k, v in ac.MARGINS.items())


def generate(ref, case, needs):
    loss_mod, bc, bb = ref
    x, t, a, l64, m = evaluate(case)
    print(case, {k: f"{v:.3e}" for k, v in m.items()}, "num_pos", a["num_pos"].tolist(), "multi", [a.get("multi_%d" % b, 0) for b in range(len(x["boxes"]))])
    assert margins_ok(m), f"{case}: margins {m} below {ac.MARGINS}"
    l64 = ac.losses_torch(x["bbox_reg"], x["centerness"], ac.anchors(), a["labels"], a["reg_targets"], grads=grads_for(a, l64))
    comp = loss_mod.ATSSLossComputation(ref_cfg(), bc.BoxCoder((10.0, 10.0, 5.0, 5.0)))
    assert comp.tokenizer is None
    # the reference cannot take an image without gts (its encode of an empty gt list against all anchors raises): it is given the
    # images that have gts; an image without any contributes nothing to a sum or a count, and its all-unassigned outputs are the
    # issue's specification, asserted by the tests directly
    live = [b for b in range(len(x["boxes"])) if len(x["boxes"][b])]
    x = dict(boxes=[x["boxes"][b] for b in live], labels=[x["labels"][b] for b in live],
             pmap=x["pmap"], bbox_reg=[t[live] for t in x["bbox_reg"]], centerness=[t[live] for t in x["centerness"]])
    a = {k: (v[live] if torch.is_tensor(v) and v.dim() and k != "margins" else v) for k, v in a.items()}
    l64 = {k: (v[live] if torch.is_tensor(v) and v.dim() >= 2 else [t[live] for t in v] if isinstance(v, list) else v) for k, v in l64.items()}
    B = len(live)
    targets = []
    for b in range(B):
        bl = bb.BoxList(x["boxes"][b].reshape(-1, 4), ac.IMAGE, mode="xyxy")
        bl.add_field("labels", x["labels"][b])
        targets.append(bl)
    anchors = [[bb.BoxList(al, ac.IMAGE, mode="xyxy") for al in ac.anchors()] for _ in range(B)]
    labels, regs, toks = comp.prepare_targets(targets, anchors, None, x["pmap"].float(), None)[:3]
    lab = torch.stack([l.to(torch.int64) for l in labels])
    reg = torch.stack(regs)
    tok = torch.stack(toks).to(torch.uint8)
    an = torch.cat(ac.anchors())
    matched = torch.full(lab.shape, -1, dtype=torch.int32)
    for b in range(B):
        for i in (lab[b] > 0).nonzero().flatten().tolist():
            codes = comp.box_coder.encode(x["boxes"][b], an[i][None].expand(len(x["boxes"][b]), 4))
            same = (codes == reg[b, i][None]).all(1).nonzero().flatten()
            assert len(same) and bool((x["boxes"][b][same] == x["boxes"][b][same[0]]).all()), (case, b, i)
            matched[b, i] = int(same[0])
    reg = torch.where((lab > 0)[..., None], reg, torch.zeros_like(reg))          # (the reference encodes gt 0 on unassigned anchors)
    # the reference's own fp32 evaluation against fp64: exact outputs, then what the floats need
    assert torch.equal(matched, a["matched"]) and torch.equal(lab.to(torch.int32), a["labels"]) and torch.equal(tok, a["token_targets"]), case
    pos = lab > 0
    needs["K_REG"] = max(needs["K_REG"], ac.need(reg[pos], a["reg_targets"][pos], a["reg_mag"][pos]))
    rec = dict(images=np.array(live, dtype=np.int32), matched=matched.numpy(), labels=lab.numpy().astype(np.int32), reg_targets=reg.numpy(),
               token_targets=np.packbits(tok.numpy(), axis=-1), num_pos=pos.sum(1).numpy().astype(np.int32))
    breg = [t.clone().requires_grad_(True) for t in x["bbox_reg"]]
    bctr = [t.clone().requires_grad_(True) for t in x["centerness"]]
    cls = [torch.zeros(B, 1, h, w) for h, w in ac.SIZES]
    out = comp(cls, breg, bctr, targets, anchors, None, x["pmap"].float())
    (out[1] + out[2]).backward()
    rec["loss_cls"], rec["loss_reg"], rec["loss_centerness"] = (np.float32(float(o)) for o in out[:3])
    n = max(float(pos.sum()), 1.0)
    s64 = l64["sums"]
    want_reg = ac.REG_LOSS_WEIGHT * s64[0] / s64[1] if int(pos.sum()) else torch.zeros(())
    if int(pos.sum()):
        w32 = comp.compute_centerness_targets(reg[pos], an[None].expand(B, -1, 4)[pos])
        needs["K_CTR"] = max(needs["K_CTR"], ac.need(w32, l64["w"][pos], l64["ctr_mag"][pos]))
        flat = ac.flatten_levels([t.detach() for t in breg], 4)[pos]
        g32 = comp.GIoULoss(flat, reg[pos], an[None].expand(B, -1, 4)[pos], weight=w32)
        b32 = comp.centerness_loss_func(ac.flatten_levels([t.detach() for t in bctr], 1)[pos][:, 0], w32)
        for got, j in ((g32, 0), (w32.sum(), 1), (b32, 2)):
            needs["K_SUM"] = max(needs["K_SUM"], ac.need(got.reshape(1), s64[j].reshape(1), l64["sums_abs"][j].reshape(1)))
        rec["sums"] = np.array([float(g32), float(w32.sum()), float(b32)], dtype=np.float32)
        for got, ref64, mag in zip([t.grad for t in breg], l64["d_bbox_reg"], _level_mags(l64["grad_mag"], 4)):
            needs["K_GRAD"] = max(needs["K_GRAD"], ac.need(got, ref64, mag))
        for got, ref64, mag in zip([t.grad for t in bctr], l64["d_centerness"], _level_mags(l64["ctr_grad_mag"][..., None], 1)):
            needs["K_GRAD"] = max(needs["K_GRAD"], ac.need(got, ref64, mag))
    else:
        rec["sums"] = np.zeros(3, dtype=np.float32)
    assert abs(float(out[1]) - float(want_reg)) <= 1e-4 * max(1.0, abs(float(want_reg))), (case, float(out[1]), float(want_reg))
    assert abs(float(out[2]) - float(s64[2]) / n) <= 1e-4 * max(1.0, float(s64[2]) / n), (case, float(out[2]), float(s64[2]) / n)
    for k in ac.MARGINS:
        rec["margin_" + k] = np.float64(min(m[k], 1e30))
    np.savez_compressed(os.path.join(OUT, case + ".npz"), **rec)
    print(case, "written; losses", [float(o) for o in out[:3]])


def _level_mags(mag, ch):
    """[B, A, ch] -> per level [B, ch, H, W]"""
    out, lo = [], 0
    for h, w in ac.SIZES:
        out.append(mag[:, lo:lo + h * w].permute(0, 2, 1).reshape(mag.shape[0], ch, h, w))
        lo += h * w
    return out


def search(case, tries=300):
    for seed in range(tries):
        m = evaluate(case, seed)[4]
        ok = margins_ok(m)
        print(case, "seed", seed, {k: f"{m[k]:.2e}" for k in ac.MARGINS}, "OK" if ok else "")
        if ok:
            return seed
    raise SystemExit(f"{case}: no seed below {tries} satisfies the margins")


def main():
    torch.set_num_threads(8)
    if "--search" in sys.argv:
        for case in ac.GOLDEN:
            print(case, "-> seed", search(case))
        return
    ref = load_reference()
    needs = dict(K_REG=0.0, K_CTR=0.0, K_SUM=0.0, K_GRAD=0.0)
    for case in ac.GOLDEN:
        generate(ref, case, needs)
    print("MEASURED =", {k: round(v, 2) for k, v in needs.items()})


if __name__ == "__main__":
    main()
