"""CPU: the host path of ops.retrieval_ranks, the sampler arithmetic, evaluate_retrieval on one and on two gloo ranks with injected
feature / score producers (no backbone), the epoch_wrapup wiring, the four retrieval configurations and the C ABI entry.

Fixtures: tests/golden/retrieval_*.npz, written by tools/gen_retrieval_golden.py from the reference's own compute_itc_recall /
compute_itm_recall and its topk lines; inputs come by name from tests/retrieval_cases.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

import retrieval_cases as rc
from mp_util import free_port, spawn_bounded

NAMES = ("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", list(rc.CASES))
def test_host_path_equals_the_restatement(name):
    from fiber_amd import ops
    scores, iids, tiids, ks = rc.torch_inputs(name)
    rank_tr, rank_ir, hits = ops.retrieval_ranks(scores, iids, tiids, ks)
    want = rc.restate(scores.numpy(), iids.numpy(), tiids.numpy(), ks)
    assert rank_tr.dtype == rank_ir.dtype == hits.dtype == torch.int32 and hits.shape == (2, len(ks))
    for what, got, ref in zip(("rank_tr", "rank_ir", "hits"), (rank_tr, rank_ir, hits), want):
        assert np.array_equal(got.numpy(), ref), (name, what, got.tolist(), ref.tolist())


@pytest.mark.parametrize("name", list(rc.TIE_FREE))
def test_host_recalls_equal_the_reference_bit_for_bit(name, golden):
    from fiber_amd import ops
    scores, iids, tiids, ks = rc.torch_inputs(name)
    hits = ops.retrieval_ranks(scores, iids, tiids, ks)[2]
    got = torch.cat([hits[0].float() / scores.shape[1], hits[1].float() / scores.shape[0]]).numpy()
    ref = golden("retrieval_" + name)["recalls"]
    assert got.dtype == ref.dtype == np.float32 and got.tobytes() == ref.tobytes(), (got.tolist(), ref.tolist())


def test_retrieval_ranks_refuses_what_it_cannot_take():
    from fiber_amd import ops
    scores, iids, tiids, _ = rc.torch_inputs("retr_edge")
    with pytest.raises(ValueError):
        ops.retrieval_ranks(scores.double(), iids, tiids)
    with pytest.raises(ValueError):
        ops.retrieval_ranks(scores, iids.long(), tiids)
    with pytest.raises(ValueError):
        ops.retrieval_ranks(scores, iids, tiids[:-1])
    with pytest.raises(ValueError):
        ops.retrieval_ranks(scores, iids, tiids, ks=tuple(range(1, 10)))


@pytest.mark.parametrize("n,world", [(6, 1), (7, 2), (5, 4)])
def test_shards_are_the_distributed_samplers(n, world):
    from torch.utils.data.distributed import DistributedSampler
    from fiber_amd.modules.retrieval_eval import shard_indices
    for rank in range(world):
        ref = list(DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=False))
        assert shard_indices(n, world, rank) == ref, (n, world, rank)


# ---- evaluate_retrieval with injected producers: image n carries n in its pixels, caption t carries t in its first token ---------------
def _injected(gold, itc):
    from fiber_amd.modules import retrieval_eval as re_
    inp = rc.model_inputs()
    n, t = len(inp["img_index"]), len(inp["text_img_index"])
    images = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 2, 2).contiguous()
    text_ids = torch.arange(t).view(t, 1).repeat(1, 4)
    data = re_.pack_retrieval_data(images, inp["img_index"], text_ids, torch.ones_like(text_ids), inp["text_img_index"],
                                   image_batch=rc.MODEL["image_batch"], text_batch=rc.MODEL["text_batch"])
    module = types.SimpleNamespace(device=torch.device("cpu"), hparams=types.SimpleNamespace(config={"get_recall_metric_itc": itc}))
    if itc:                                                  # one-hot image features x the fixture's columns: the fixture's matrix, exactly
        S = torch.from_numpy(gold["itc_scores"])
        col_of = torch.from_numpy(np.argsort(gold["itc_caption"]))      # caption t sits at column col_of[t] of the fixture's matrix
        eye = torch.eye(n)
        return module, data, dict(features=(lambda img: eye[img[:, 0, 0, 0].long()], lambda b: S[:, col_of[b["text_ids"][:, 0]]].t()))
    S = torch.from_numpy(gold["itm_scores"])
    return module, data, dict(scores=lambda img: S[img[:, 0, 0, 0].long()])


@pytest.mark.parametrize("itc", [True, False])
def test_evaluate_retrieval_gives_the_references_recalls(itc, golden):
    from fiber_amd.modules.retrieval_eval import evaluate_retrieval
    gold = golden("retrieval_model")
    module, data, kw = _injected(gold, itc)
    got = evaluate_retrieval(module, data, **kw)
    assert len(got) == 6 and all(v.dim() == 0 and v.dtype == torch.float32 for v in got)
    ref = gold["itc_recalls" if itc else "itm_recalls"]
    assert np.array([float(v) for v in got], np.float32).tobytes() == ref.tobytes(), ([float(v) for v in got], ref.tolist())


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from fiber_amd import parallel
    from fiber_amd.modules.retrieval_eval import evaluate_retrieval
    import torch.distributed as dist
    parallel.init_distributed("gloo")
    gold = dict(np.load(os.path.join(GOLDEN, "retrieval_model.npz"), allow_pickle=False))
    res = {}
    for itc in (True, False):
        module, data, kw = _injected(gold, itc)
        res[itc] = [float(v) for v in evaluate_retrieval(module, data, **kw)]
    if rank == 0:
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_retrieval_over_two_ranks(tmp_path, golden):
    port = free_port()
    out = str(tmp_path / "r0.pt")
    spawn_bounded(_worker, (2, port, out), nprocs=2, deadline_s=150)
    res, gold = torch.load(out), golden("retrieval_model")
    for itc, key in ((True, "itc_recalls"), (False, "itm_recalls")):
        assert np.array(res[itc], np.float32).tobytes() == gold[key].tobytes(), (itc, res[itc], gold[key].tolist())


# ---- epoch_wrapup ---------------------------------------------------------------------------------------------------------------------
class _Module:
    """What epoch_wrapup and compute_itc_recall read of the LightningModule; infer hands back the injected features"""

    def __init__(self, gold, **cfg):
        self.training, self.logged, self.device = False, {}, torch.device("cpu")
        self.hparams = types.SimpleNamespace(config=dict(loss_names={}, get_recall_metric=True, get_recall_metric_itc=True, **cfg))
        _, self.retrieval_data, kw = _injected(gold, True)
        self.image_fn, self.text_fn = kw["features"]

    def log(self, name, value, **kw):
        self.logged[name] = value

    def infer(self, batch, image_only=False, text_only=False):
        return {"cls_feats": self.image_fn(batch["image"][0]) if image_only else self.text_fn(batch)}


def test_epoch_wrapup_logs_the_recalls_and_adds_them_to_the_metric(golden):
    from fiber_amd.modules import fiber_utils
    gold = golden("retrieval_model")
    m = _Module(gold)
    fiber_utils.epoch_wrapup(m)
    ref = gold["itc_recalls"]
    for tag, want in zip(NAMES, ref):
        assert np.float32(float(m.logged["recalls/" + tag])) == want, tag
    assert set(k for k in m.logged if k.startswith("recalls/")) == {"recalls/" + t for t in NAMES}
    assert np.float32(float(m.logged["val/the_metric"])) == np.float32(ref[0] + ref[3])
    m.training, m.logged = True, {}                          # a training epoch computes no recall
    fiber_utils.epoch_wrapup(m)
    assert list(m.logged) == ["train/the_metric"] and m.logged["train/the_metric"] == 0


def test_epoch_wrapup_without_retrieval_data_names_the_attribute(golden):
    from fiber_amd.modules import fiber_utils
    m = _Module(golden("retrieval_model"))
    del m.retrieval_data
    with pytest.raises(ValueError, match="retrieval_data"):
        fiber_utils.epoch_wrapup(m)


# ---- configuration and ABI ------------------------------------------------------------------------------------------------------------
_COMMON = dict(batch_size=1024, max_epoch=10, max_steps=None, warmup_steps=0.1, learning_rate=2e-5, lr_mult_cross_modal=5, lr_mult_head=5,
               max_text_len=50, train_transform_keys=["albef_randaug"], val_transform_keys=["albef"], pretrained_vit=False)
REFERENCE_CONFIGS = {                                        # reference config.py:153-231
    "task_finetune_irtr_itc_coco": dict(_COMMON, exp_name="finetune_irtr_itc_coco", datasets=["coco"], loss="itc", image_size=576,
                                        get_recall_metric_itc=True, resolution_before=384, draw_false_image=1),
    "task_finetune_irtr_itc_f30k": dict(_COMMON, exp_name="finetune_irtr_itc_f30k", datasets=["f30k"], loss="itc", image_size=576,
                                        get_recall_metric_itc=True, resolution_before=576, draw_false_image=1),
    "task_finetune_irtr_itm_coco": dict(_COMMON, exp_name="finetune_irtr_itm_coco", datasets=["coco"], loss="itm", image_size=384,
                                        get_recall_metric_itc=False, resolution_before=384, draw_false_image=1),
    "task_finetune_irtr_itm_f30k": dict(_COMMON, exp_name="finetune_irtr_itm_f30k", datasets=["f30k"], loss="itm", image_size=384,
                                        get_recall_metric_itc=False, resolution_before=384, draw_false_image=1),
}


@pytest.mark.parametrize("name", list(REFERENCE_CONFIGS))
def test_named_retrieval_configs_equal_the_references(name):
    from fiber_amd.config import named_config
    want = dict(REFERENCE_CONFIGS[name])
    loss = want.pop("loss")
    c = named_config(name)
    for k, v in want.items():
        assert c[k] == v, (name, k, c[k], v)
    assert {k for k, v in c["loss_names"].items() if v > 0} == {loss} and c["loss_names"][loss] == 1
    assert c["get_recall_metric"] is False                    # the command line sets it, as in the reference


def test_c_abi_exports_the_retrieval_entry():
    from fiber_amd import lib
    l = lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fiber_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long)\s+(fiber_\w+)\s*\(", hdr))
    name = "fiber_retrieval_ranks"
    assert hasattr(l, name) and name in declared and name in lib.exported_symbols()
    assert len(lib.SIGNATURES[name]) == 11
