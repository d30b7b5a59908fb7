"""Generate tests/golden/ground_*.npz by executing the REFERENCE's grounding head and token loss (runs where the reference tree is present):

    python tools/gen_ground_golden.py

Loss: the reference's own layers/sigmoid_focal_loss.py (TokenSigmoidFocalLoss / token_sigmoid_binary_focal_loss), loaded by path with a
stub `maskrcnn_benchmark._C` (the token functions are pure torch).
Head: the reference's own modeling/rpn/vldyhead.py `VLDyHead`, loaded by path behind permissive stub modules for the imports the FIBER
configuration never executes (maskrcnn_benchmark.*, timm, the transformers model classes); `Scale` and `DYReLU` are the reference's own
(layers/misc.py, layers/dyrelu.py), `permute_and_flatten` is modeling/utils.py's, and -- the ONE stand-in, as in
oracle/gen_dyhead_golden.py -- `ModulatedDeformConv` is oracle/dcn_ref.py's restatement (the CUDA extension cannot be built here; that file's
parity is unpinned, so the fixture inherits that caveat for the deformable sampling only).  `RobertaConfig.from_pretrained` is patched to a
local default config: it is only consulted for branches FIBER does not take.
Cases, inputs and weights by name: tests/ground_cases.py (the product regenerates them identically; the fixtures hold outputs only).
The [A, T] tensors are kept on a seeded subset of rows, dX on a seeded subset of channels, the gradient of `embedding` on its first tokens
(live, masked-in-the-middle and tail ones) and that of the text projection on a seeded subset of rows, each with its full norm beside it:
no committed file may pass 1 MiB."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import dcn_ref, shim                             # noqa: E402
from tests import ground_cases as gc                         # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")
ROWS = 48                                                    # rows of the [A, T] tensors kept per image (seeded index)


class _Stub(types.ModuleType):
    """a module any name can be imported from: unknown attributes are empty classes"""
    __all__ = []
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {})
        setattr(self, name, cls)
        return cls


def load_loss():
    sys.modules.setdefault("maskrcnn_benchmark", _Stub("maskrcnn_benchmark"))
    sys.modules["maskrcnn_benchmark._C"] = _Stub("maskrcnn_benchmark._C")
    return shim._load("sigmoid_focal_loss", os.path.join(MB, "layers", "sigmoid_focal_loss.py"), "_fiber_reference_fg_layers")


def load_head():
    import transformers
    from transformers import RobertaConfig
    saved = dict(sys.modules)
    layers = os.path.join(MB, "layers")
    pkg = "_fiber_reference_fg_layers"
    for n in (pkg,):
        m = types.ModuleType(n)
        m.__path__ = [layers]
        sys.modules[n] = m
    dc = types.ModuleType(pkg + ".deform_conv")
    dc.ModulatedDeformConv = dcn_ref.ModulatedDeformConv
    sys.modules[pkg + ".deform_conv"] = dc
    dyrelu = shim._load("dyrelu", os.path.join(layers, "dyrelu.py"), pkg)
    for n in ("batch_norm", "nms", "roi_align", "roi_pool", "smooth_l1_loss", "sigmoid_focal_loss", "iou_loss", "dropblock", "evonorm", "se",
              "set_loss"):
        sys.modules.setdefault(f"{pkg}.{n}", _Stub(f"{pkg}.{n}"))
    sys.modules["maskrcnn_benchmark"] = _Stub("maskrcnn_benchmark")
    sys.modules["maskrcnn_benchmark._C"] = _Stub("maskrcnn_benchmark._C")
    misc = shim._load("misc", os.path.join(layers, "misc.py"), pkg)
    mb_layers = _Stub("maskrcnn_benchmark.layers")
    mb_layers.Scale, mb_layers.DYReLU, mb_layers.ModulatedDeformConv = misc.Scale, dyrelu.DYReLU, dcn_ref.ModulatedDeformConv
    sys.modules["maskrcnn_benchmark.layers"] = mb_layers
    for n in ("structures", "structures.boxlist_ops", "modeling", "modeling.backbone", "modeling.backbone.fbnet", "engine", "engine.inference",
              "utils", "utils.fuse_helper", "modeling.language_backbone", "modeling.language_backbone.clip_model", "utils.shallow_contrastive_loss_helper",
              "utils.amp", "config"):
        sys.modules["maskrcnn_benchmark." + n] = _Stub("maskrcnn_benchmark." + n)
    import math
    fb = sys.modules["maskrcnn_benchmark.modeling.backbone.fbnet"]     # vldyhead.py gets `math` through this star import
    fb.math, fb.__all__ = math, ["math"]
    for n in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(n, _Stub(n))
    bert = _Stub("transformers.models.bert.modeling_bert")
    bert.BertPreTrainedModel = type("BertPreTrainedModel", (torch.nn.Module,), {})
    sys.modules["transformers.models.bert.modeling_bert"] = bert
    mu = _Stub("transformers.modeling_utils")
    sys.modules["transformers.modeling_utils"] = mu
    rc = _Stub("transformers.models.roberta.configuration_roberta")
    rc.RobertaConfig = type("RobertaConfig", (), {"from_pretrained": staticmethod(lambda *_a, **_k: RobertaConfig())})
    sys.modules["transformers.models.roberta.configuration_roberta"] = rc
    rpn = "_fiber_reference_fg.modeling.rpn"
    for n in ("_fiber_reference_fg", "_fiber_reference_fg.modeling", rpn, rpn + ".inference", rpn + ".loss", rpn + ".anchor_generator"):
        sys.modules[n] = _Stub(n)
    shim._load("utils", os.path.join(MB, "modeling", "utils.py"), "_fiber_reference_fg.modeling")
    try:
        return shim._load("vldyhead", os.path.join(MB, "modeling", "rpn", "vldyhead.py"), rpn)
    finally:
        for k in [k for k in sys.modules if k.startswith("transformers") or k.startswith("timm")]:
            if k in saved:
                sys.modules[k] = saved[k]
            else:
                del sys.modules[k]
        del transformers


def gen_loss_only(fl):
    c = gc.loss_only_case()
    rows = np.sort(np.random.default_rng(0).choice(gc.A_LOSS_ONLY, ROWS, replace=False))
    rec = {"rows": rows}
    for i, (gamma, alpha) in enumerate(gc.LOSS_ONLY_HYPER):
        lg = c["logits"].clone().requires_grad_()
        s = torch.clamp(torch.clamp(lg, max=50000), min=-50000)             # vldyhead.py:888-890
        loss = fl.TokenSigmoidFocalLoss(alpha, gamma)(s, c["targets"].float(), c["mask"].clone(), version="binary")
        loss.backward()
        rec[f"loss{i}"] = np.float32(loss.item())
        rec[f"dlogits{i}"] = lg.grad[:, rows].numpy()
    rec["hyper"] = np.array(gc.LOSS_ONLY_HYPER, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "ground_loss_only.npz"), **rec)
    print("ground_loss_only", [float(rec[f"loss{i}"]) for i in range(len(gc.LOSS_ONLY_HYPER))])


def gen_small(vl, fl):
    c = gc.SMALL
    torch.manual_seed(0)
    model = vl.VLDyHead(gc.head_cfg(convs=c["convs"])).float()
    gc.set_head_weights(model)
    xs, emb, tg, mask = gc.small_inputs()
    xs = [x.requires_grad_() for x in xs]
    emb = emb.requires_grad_()
    out = model(xs, None, emb)
    assert [o is None for o in out] == [False, False, False, True, True, True, False, True, True, True]
    dot = torch.cat(out[6], dim=1)
    loss = fl.TokenSigmoidFocalLoss(c["alpha"], c["gamma"])(dot, tg.float(), mask.clone(), version="binary") / c["num_pos"]
    loss.backward()
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(gc.A_SMALL, ROWS, replace=False))
    chans = np.sort(rng.choice(gc.C, gc.KEEP_CHANNELS, replace=False))       # the committed-file limit: gradients kept on seeded subsets
    wrows = np.sort(rng.choice(gc.C, gc.KEEP_WROWS, replace=False))
    rec = {"rows": rows, "chans": chans, "wrows": wrows, "loss": np.float32(loss.item()), "dot_rows": dot.detach()[:, rows].numpy(),
           "state_keys": np.array(list(model.state_dict().keys())),
           "state_shapes": np.array([",".join(str(d) for d in v.shape) for v in model.state_dict().values()]),
           "param_names": np.array([k for k, _ in model.named_parameters()]),
           "grad_norms": np.array([float(p.grad.norm()) if p.grad is not None else 0.0 for _, p in model.named_parameters()], dtype=np.float64),
           "dembedding": emb.grad[:, :gc.KEEP_TOKENS].numpy(), "dembedding_norm": np.float64(emb.grad.norm())}
    # tower features and projected tokens of the reference run (for the fp64 restatement of the dot product in the host test)
    tower = model.dyhead_tower({"visual": xs, "lang": None})["visual"]
    q = torch.cat([f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, f.shape[1]) for f in tower], dim=1).detach()
    e = torch.nn.functional.normalize(emb.detach(), p=2, dim=-1)
    p = model.dot_product_projection_text(e / 2.0).detach()
    text = {"q_rows": q[:, rows].numpy(), "proj": p.numpy(), "tbias": (torch.matmul(e, model.bias_lang) + model.bias0).detach().numpy()}
    rec["dot_mag_rows"] = (torch.matmul(q[:, rows].double().abs(), p.double().abs().transpose(1, 2)) * float(torch.exp(-model.log_scale.detach()))).float().numpy()
    for l in range(len(xs)):
        rec[f"logits{l}"], rec[f"bbox_reg{l}"], rec[f"centerness{l}"] = (out[i][l].detach().numpy() for i in range(3))
        rec[f"dx{l}"] = xs[l].grad[:, chans].numpy()
        rec[f"dx_norm{l}"] = np.float64(xs[l].grad.norm())
    for k, prm in model.named_parameters():
        if k in ("log_scale", "bias0", "bias_lang"):
            rec["grad:" + k] = prm.grad.numpy()
        if k == "dot_product_projection_text.weight":
            rec["grad:" + k] = prm.grad[wrows].numpy()
    np.savez_compressed(os.path.join(OUT, "ground_small.npz"), **rec)
    np.savez_compressed(os.path.join(OUT, "ground_small_text.npz"), **text)
    print("ground_small loss", float(loss), "dot std", float(dot.std()), "positives", int(tg.sum()), "keys", len(rec["state_keys"]))


def main():
    torch.set_num_threads(8)
    fl = load_loss()
    gen_loss_only(fl)
    gen_small(load_head(), fl)


if __name__ == "__main__":
    main()
