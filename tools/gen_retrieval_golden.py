"""Generate tests/golden/retrieval_*.npz by executing the REFERENCE's retrieval evaluation on the CPU (runs where the reference tree is
present):

    python tools/gen_retrieval_golden.py

Executed by path through oracle.shim, unmodified: coarse_grained/fiber/modules/objectives.py (compute_itc_recall, compute_itm_recall) over
the reference's own Swin / RoBERTa modules wired as oracle.gen_golden.RefFused, detgen.fill_ weights, rank_output tied to the ITM head's
"match" row as the reference's constructor does (fiber_module.py:112-114).  Stand-ins, none of which carries arithmetic: the datamodule
(`trainer.datamodule.dms[0]`: two list datasets with a collate that stacks), `hparams`, `device`, and an `infer` wrapper that hands
RefFused.infer the keys it reads unconditionally.  One gloo process, file rendezvous.

Inputs by name from tests/retrieval_cases.py (the fixtures hold outputs only):
  retrieval_model.npz     MODEL (10 images x 2 captions on the tiny configuration): the six recalls and the score matrix of each of the two
                          functions, with the ids in the matrix's order (ITC: texts sorted by image id, and which caption each column is, since
                          the reference's sort is not a stable one; ITM: loader order).
  retrieval_<case>.npz    for the tie-free tally cases: the six recalls the reference's topk lines (objectives.py:363-383, compiled out of
                          the file, not copied) give on the case's matrix.
Asserted: no two scores of a row or of a column of any recorded matrix are equal (torch.topk's order among equal scores is undefined).
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import detgen, gen_golden, shim                  # noqa: E402
from tests import retrieval_cases as rc                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10")


def assert_tie_free(name, s):
    s = np.asarray(s)
    for axis, what in ((1, "row"), (0, "column")):
        srt = np.sort(s, axis=axis)
        assert (np.diff(srt, axis=axis) != 0).all(), f"{name}: two equal scores in a {what}"


def topk_lines(path):
    """The statements of compute_itc_recall from `topk10 = scores.topk(10, dim=1)` up to its return, compiled out of the reference file"""
    src = open(path).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "compute_itc_recall")
    first = next(i for i, st in enumerate(fn.body) if "scores.topk(10, dim=1)" in (ast.get_source_segment(src, st) or ""))
    body = [st for st in fn.body[first:] if not isinstance(st, ast.Return)]
    return compile(ast.Module(body=body, type_ignores=[]), path, "exec")


class _ListSet:
    def __init__(self, items, image_only):
        self.items, self.image_only = items, image_only

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def collate(self, batch, mlm_collator=None):
        if self.image_only:
            return {"image": [torch.stack([b["image"] for b in batch])], "img_index": [b["img_index"] for b in batch]}
        out = {k: torch.stack([b[k] for b in batch]) for k in ("text_ids", "text_masks", "text_labels")}
        out["img_index"] = [b["img_index"] for b in batch]
        return out


class _DataModule:
    tokenizer = None
    mlm_collator = None

    def __init__(self, inp):
        self.inp = inp

    def make_no_false_val_dset(self, image_only=False):
        i = self.inp
        if image_only:
            return _ListSet([{"image": i["images"][n], "img_index": i["img_index"][n]} for n in range(len(i["img_index"]))], True)
        return _ListSet([{"text_ids": i["text_ids"][n], "text_masks": i["text_masks"][n],
                          "text_labels": torch.full_like(i["text_ids"][n], -100), "img_index": i["text_img_index"][n]}
                         for n in range(len(i["text_img_index"]))], False)


def generate_model(obj):
    sw, rb = shim.load_reference()
    heads = shim._load("heads", os.path.join(shim.MODS, "heads.py"), "_fiber_reference_modules")
    torch.manual_seed(0)
    m = detgen.fill_(gen_golden.RefFused(sw, rb, heads, rc.MODEL_CONFIG).eval())
    m.rank_output.weight.data = m.itm_score.fc.weight.data[1:, :]           # fiber_module.py:113-114
    m.rank_output.bias.data = m.itm_score.fc.bias.data[1:]
    m.hparams = types.SimpleNamespace(config=dict(m.c, num_workers=0))
    m.device = torch.device("cpu")
    inp = rc.model_inputs()
    m.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[_DataModule(inp)]))
    inner = m.infer

    def infer(batch, **kw):                                   # RefFused.infer reads the other modality's keys before it branches
        b = dict(batch)
        if kw.get("image_only"):
            b.setdefault("text_ids", None), b.setdefault("text_masks", None)
        if kw.get("text_only"):
            kw.setdefault("img", torch.zeros(0))
        return inner(b, **kw)
    m.infer = infer
    seen = []
    real_topk = torch.Tensor.topk

    def recording(self, *a, **k):
        if not seen:
            seen.append(self.detach().clone())
        return real_topk(self, *a, **k)
    orders = []
    real_sort = torch.Tensor.sort

    def recording_sort(self, *a, **k):                        # `tiids.sort()` (objectives.py:353) is not a stable sort: which caption of an
        r = real_sort(self, *a, **k)                          # image lands in which column is the reference's choice, recorded here
        orders.append(r.indices.clone())
        return r
    d = {}
    for tag, fn in (("itc", obj.compute_itc_recall), ("itm", obj.compute_itm_recall)):
        del seen[:], orders[:]
        torch.Tensor.topk, torch.Tensor.sort = recording, recording_sort
        try:
            rec = fn(m)
        finally:
            torch.Tensor.topk, torch.Tensor.sort = real_topk, real_sort
        if tag == "itc":
            assert len(orders) == 1 and sorted(orders[0].tolist()) == list(range(len(inp["text_img_index"])))
            d["itc_caption"] = orders[0].numpy().astype(np.int32)       # column j of itc_scores is caption itc_caption[j] of the inputs
        scores = seen[0].float().numpy()
        assert scores.shape == (len(inp["img_index"]), len(inp["text_img_index"]))
        assert_tie_free("retrieval_model/" + tag, scores)
        d[tag + "_recalls"] = np.array([float(v) for v in rec], np.float32)
        d[tag + "_scores"] = scores
        print("retrieval_model", tag, dict(zip(NAMES, d[tag + "_recalls"].tolist())))
    d["iids"] = np.array(inp["img_index"], np.int32)
    d["itc_tiids"] = np.sort(np.array(inp["text_img_index"], np.int32), kind="stable")
    d["itm_tiids"] = np.array(inp["text_img_index"], np.int32)
    np.savez_compressed(os.path.join(OUT, "retrieval_model.npz"), **d)


def generate_tally(code, case):
    c = rc.case_inputs(case)
    scores = np.ascontiguousarray(c["scores"])
    assert_tie_free(case, scores)
    ns = {"torch": torch, "scores": torch.from_numpy(scores), "iids": torch.from_numpy(c["iids"]).long(),
          "tiids": torch.from_numpy(c["tiids"]).long()}
    exec(code, ns)
    rec = np.array([float(ns[n]) for n in NAMES], np.float32)
    np.savez_compressed(os.path.join(OUT, f"retrieval_{case}.npz"), recalls=rec)
    print(case, dict(zip(NAMES, rec.tolist())))


def main():
    import torch.distributed as dist
    torch.set_num_threads(8)
    shim.load_reference()
    path = os.path.join(shim.MODS, "objectives.py")
    obj = shim._load("objectives", path, "_fiber_reference_modules")
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "rdv"), rank=0, world_size=1)
        generate_model(obj)
        dist.destroy_process_group()
    code = topk_lines(path)
    for case in rc.TIE_FREE:
        generate_tally(code, case)


if __name__ == "__main__":
    main()
