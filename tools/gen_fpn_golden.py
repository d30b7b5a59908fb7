"""Generate tests/golden/fpn_neck.npz by executing the REFERENCE's FPN neck on the CPU (runs where the reference tree is present):

    python tools/gen_fpn_golden.py

Executed by path behind stub parents, unmodified: modeling/backbone/fpn.py (FPN, LastLevelP6P7), layers/dropblock.py (DropBlock2D),
modeling/make_layers.py (conv_with_kaiming_uniform) with layers/misc.py (Conv2d) and layers/dyrelu.py (DYReLU) behind it; fpn.py and
dropblock.py import only torch.  The stubs stand for what make_layers imports and this wiring never calls: maskrcnn_benchmark.config.cfg
(read by group_norm only) and modeling.poolers.Pooler.  The modules are wired as build_retinanet_swint_fpn_backbone does
(modeling/backbone/__init__.py:175-192) for the default configuration: DROP_BLOCK on, 0.3, 3.

Inputs by name from tests/fpn_cases.py; the weights are the reference's own kaiming_uniform_(a=1) initialisation under a fixed seed, with
the biases (zero by initialisation) drawn small so that they are tested.  The fixture holds the weights, the eval outputs, the train-mode
outputs together with the Bernoulli draws that produced them, and the gradients of the inputs and the weights for the linear loss
sum_l <out_l, proj_l> in train mode.  The reference draws with host torch.rand after torch.manual_seed; the tool re-draws the same shapes
in the same order (the stride-16 level, then the stride-8 level) and asserts that replaying them through the reference's own block-mask
code reproduces the train-mode outputs.  It also prints the rel-L2 distance of fpn_cases.neck_ref(bf16=True) from every fixture
entry: the figures recorded in fpn_cases.BF16_DISTANCE.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import shim                                      # noqa: E402
import fpn_cases as fc                                       # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference():
    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m
    for n in ("maskrcnn_benchmark", "maskrcnn_benchmark.modeling", "maskrcnn_benchmark.modeling.backbone"):
        pkg(n)
    pkg("maskrcnn_benchmark.config").cfg = None
    pkg("maskrcnn_benchmark.modeling.poolers").Pooler = None
    layers = pkg("maskrcnn_benchmark.layers")
    layers.Conv2d = shim._load("misc", os.path.join(MB, "layers", "misc.py"), "maskrcnn_benchmark.layers").Conv2d
    layers.DYReLU = shim._load("dyrelu", os.path.join(MB, "layers", "dyrelu.py"), "maskrcnn_benchmark.layers").DYReLU
    db = shim._load("dropblock", os.path.join(MB, "layers", "dropblock.py"), "maskrcnn_benchmark.layers")
    ml = shim._load("make_layers", os.path.join(MB, "modeling", "make_layers.py"), "maskrcnn_benchmark.modeling")
    fpn = shim._load("fpn", os.path.join(MB, "modeling", "backbone", "fpn.py"), "maskrcnn_benchmark.modeling.backbone")
    return fpn, db, ml


def build(fpn, db, ml):
    c, out = fc.NECK["stage_channels"], fc.NECK["out_channels"]
    torch.manual_seed(7)
    neck = fpn.FPN(in_channels_list=[0, c[0], c[1], c[2]], out_channels=out, conv_block=ml.conv_with_kaiming_uniform(False, False),
                   top_blocks=fpn.LastLevelP6P7(out, out), drop_block=db.DropBlock2D(fc.DROP_PROB, fc.DROP_SIZE))
    with torch.no_grad():
        for k, p in neck.named_parameters():
            if k.endswith(".bias"):
                p.uniform_(-0.1, 0.1)
    assert set(neck.state_dict()) == set(fc.WEIGHT_KEYS), list(neck.state_dict())
    return neck


def main():
    torch.set_num_threads(8)
    fpn, db, ml = load_reference()
    neck = build(fpn, db, ml)
    maps, proj = fc.neck_inputs()
    rec = {"w." + k: v.detach().numpy() for k, v in neck.state_dict().items()}

    neck.eval()
    with torch.no_grad():
        ev = neck(maps)
    assert [tuple(o.shape[-2:]) for o in ev] == list(fc.LEVEL_SIZES), [o.shape for o in ev]
    for n, o in zip(fc.OUT_NAMES, ev):
        rec["eval." + n] = o.numpy()

    neck.train()
    xs = [m.clone().requires_grad_(True) for m in maps]
    torch.manual_seed(fc.DRAW_SEED)
    tr = neck(xs)
    sum((o * p).sum() for o, p in zip(tr, proj)).backward()
    # the same draws again: torch.rand of the same shapes in the same order (dropblock.py:45)
    B = fc.NECK["B"]
    gamma = fc.DROP_PROB / fc.DROP_SIZE ** 2
    torch.manual_seed(fc.DRAW_SEED)
    draws = [(torch.rand(B, *fc.NECK["sizes"][1]) < gamma), (torch.rand(B, *fc.NECK["sizes"][0]) < gamma)]
    for n, o in zip(fc.OUT_NAMES, tr):
        rec["train." + n] = o.detach().numpy()
    rec["draw.s16"], rec["draw.s8"] = draws[0].numpy().astype(np.uint8), draws[1].numpy().astype(np.uint8)
    for i, x in enumerate(xs[1:]):
        rec[f"grad.x{i + 3}"] = x.grad.numpy()
    assert xs[0].grad is None                                # the stride-4 map is never read
    for k, p in neck.named_parameters():
        rec["grad." + k] = p.grad.numpy()

    # replay: the recorded draws through the reference's own block-mask code reproduce the train-mode outputs
    class Replay(db.DropBlock2D):
        def forward(self, x):
            mask = draws_left.pop(0).float()
            block_mask = self._compute_block_mask(mask)
            out = x * block_mask[:, None, :, :]
            return out * block_mask.numel() / block_mask.sum()
    draws_left = list(draws)
    neck.drop_block = Replay(fc.DROP_PROB, fc.DROP_SIZE).train()
    with torch.no_grad():
        again = neck(maps)
    for n, a, b in zip(fc.OUT_NAMES, again, tr):
        assert torch.equal(a, b.detach()), f"replaying the draws does not reproduce train.{n}"
    # the draws also agree with the restatement's integer block mask
    for d in draws:
        keep, kept = fc.mask_ref(d.numpy().astype(np.uint8), fc.DROP_SIZE)
        bm = Replay(fc.DROP_PROB, fc.DROP_SIZE)._compute_block_mask(d.float())
        assert np.array_equal(keep, bm.numpy().astype(np.uint8)) and kept == int(bm.sum())
    print("dropped block centres:", [int(d.sum()) for d in draws], "of", [d.numel() for d in draws])
    np.savez_compressed(os.path.join(OUT, fc.GOLDEN + ".npz"), **rec)
    print("wrote", fc.GOLDEN, {k: v.shape for k, v in rec.items() if not k.startswith(("w.", "grad."))})
    print("BF16_DISTANCE =", distances(rec))


def distances(rec):
    """rel-L2 of the bf16-rounding restatement from the fixture, per entry"""
    w = {k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("w.")}
    maps, proj = fc.neck_inputs()
    out = {}
    with torch.no_grad():
        for n, o in zip(fc.OUT_NAMES, fc.neck_ref(w, maps, bf16=True)):
            out["eval." + n] = fc.rel_l2(o, rec["eval." + n])
    seeds = [rec["draw.s16"], rec["draw.s8"]]
    wg = {k: v.double().requires_grad_(True) for k, v in w.items()}
    xs = [m.double().requires_grad_(True) for m in maps]
    tr = fc.neck_ref(wg, xs, train_seeds=seeds, bf16=True)
    sum((o * p.double()).sum() for o, p in zip(tr, proj)).backward()
    for n, o in zip(fc.OUT_NAMES, tr):
        out["train." + n] = fc.rel_l2(o.detach(), rec["train." + n])
    for i, x in enumerate(xs[1:]):
        out[f"grad.x{i + 3}"] = fc.rel_l2(x.grad, rec[f"grad.x{i + 3}"])
    for k, v in wg.items():
        out["grad." + k] = fc.rel_l2(v.grad, rec["grad." + k])
    return {k: float(f"{v:.3e}") for k, v in out.items()}


if __name__ == "__main__":
    main()
