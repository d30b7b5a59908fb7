"""CPU tests of grounding training: the plain-torch restatement of tests/atss_cases.py against the fixtures the reference's own
ATSSLossComputation produced (tools/gen_atss_golden.py), the target container, the unsupported switches, and the normalisers under gloo."""
import os

import numpy as np
import pytest
import torch

import atss_cases as ac
import ground_cases as gc
import mp_util


def _evaluate(case, dtype):
    x = ac.inputs(case)
    t = ac.packed(case, x)
    a = ac.assign_torch(ac.anchors(), t, dtype=dtype)
    x = ac.mark_edge(case, x, ac.assign_torch(ac.anchors(), t)["matched"])
    l = ac.losses_torch(x["bbox_reg"], x["centerness"], ac.anchors(), a["labels"], a["reg_targets"], dtype=dtype)
    return x, t, a, l


@pytest.mark.parametrize("case", ac.GOLDEN)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_reproduces_the_reference(golden, case, dtype):
    gold = golden(case)
    for k, v in ac.MARGINS.items():
        assert float(gold["margin_" + k]) >= v, f"{case}: the fixture is not decisive in {k}"
    x, t, a, l = _evaluate(case, dtype)
    live = gold["images"].tolist()
    assert live == [b for b, n in enumerate(ac.CASES[case]["gts"]) if n], "the fixture covers every image that has gts"
    assert np.array_equal(a["matched"][live].numpy(), gold["matched"]), f"{case}: matched"
    assert np.array_equal(a["labels"][live].numpy(), gold["labels"]), f"{case}: labels"
    assert np.array_equal(a["num_pos"][live].numpy(), gold["num_pos"])
    assert np.array_equal(np.packbits(a["token_targets"][live].numpy(), axis=-1), gold["token_targets"]), f"{case}: token targets"
    for b in set(range(ac.CASES[case]["B"])) - set(live):    # an image without gts: all unassigned
        assert bool((a["matched"][b] == -1).all()) and bool((a["labels"][b] == 0).all()) and int(a["num_pos"][b]) == 0
        assert bool((a["token_targets"][b, :, :-1] == 0).all()) and bool((a["token_targets"][b, :, -1] == 1).all())
    a64 = a if dtype == torch.float64 else ac.assign_torch(ac.anchors(), t)
    k = 2 * ac.MEASURED["K_REG"] + 1                         # two fp32 evaluations (or one), each within its measured need of fp64
    assert ac.need(torch.from_numpy(gold["reg_targets"]), a["reg_targets"][live], a64["reg_mag"][live]) <= k
    l64 = l if dtype == torch.float64 else ac.losses_torch(x["bbox_reg"], x["centerness"], ac.anchors(), a64["labels"], a64["reg_targets"])
    ks = 2 * ac.MEASURED["K_SUM"] + 1
    assert ac.need(torch.from_numpy(gold["sums"]), l["sums"], l64["sums_abs"]) <= ks, f"{case}: the three sums"
    n = max(float(a["num_pos"].sum()), 1.0)
    s = l64["sums"]
    tol = lambda v: 4 * ks * ac.EPS * max(abs(v), 1.0)       # noqa: E731  (a quotient of two such sums, stored in fp32)
    want_reg = ac.REG_LOSS_WEIGHT * float(s[0]) / float(s[1]) if float(s[1]) > 0 else 0.0
    assert abs(float(gold["loss_reg"]) - want_reg) <= tol(want_reg)
    assert abs(float(gold["loss_centerness"]) - float(s[2]) / n) <= tol(float(s[2]) / n)
    assert float(gold["loss_cls"]) == 0.0


def test_cases_hold_what_they_claim():
    x, t, a, l = _evaluate("atss_edge", torch.float64)
    assert a["num_pos"].tolist()[:2] == [0, 0] and int(a["num_pos"][2]) > 0 and int(t.num_gt[1]) == 1
    assert a["multi_2"] > 0, "anchors positive for several gts"
    reg0 = x["bbox_reg"][0][2]
    pos = (a["matched"][2, :560] >= 0).nonzero().flatten().tolist()
    assert float(reg0[2].flatten()[pos[0]]) / 5 > ac.CLIP and float(reg0[2].flatten()[pos[1]]) < -30
    x, t, a, _ = _evaluate("atss_many", torch.float64)
    assert t.boxes.shape[1] == 72 and bool(torch.isnan(t.boxes[0, 70:]).all()) and not bool(torch.isnan(a["reg_targets"]).any())
    x, t, a, _ = _evaluate("atss_ties", torch.float64)
    assert a["margins"]["cut_gap"] == 0.0 and a["margins"]["best_vs_second"] == 0.0, "the tie case ties"
    # gt 0 sits on the corner shared by the level-0 cells (5, 5), (5, 6), (6, 5), (6, 6) -> anchors 145, 146, 173, 174 at sqrt(32), then
    # eight at sqrt(160) of which the cut keeps the five lowest indices
    c = a["cand_idx"][0, 0, :9].tolist()
    assert c[:4] == [145, 146, 173, 174] and c[4:] == sorted(c[4:]) == [117, 118, 144, 147, 172]
    assert not bool((a["matched"] == 2).any()) and bool((a["matched"] == 1).any()), "identical boxes: the lower gt index wins"


def test_pack_targets_round_trip():
    from fiber_amd.modules.grounding_train import pack_targets
    x = ac.inputs("atss_edge")
    t = pack_targets(x["boxes"], x["labels"], x["pmap"])
    assert t.boxes.shape == (3, 7, 4) and t.labels.dtype == torch.int32 and t.positive_map.dtype == torch.uint8 and t.num_gt.tolist() == [0, 1, 7]
    assert t.positive_map.shape == (3, 7, ac.T) and bool((t.boxes[0] == 0).all()) and bool((t.positive_map[1, 1:] == 0).all())
    boxes, labels, rows = t.unpack()
    assert all(torch.equal(u, v) for u, v in zip(boxes, x["boxes"])) and all(torch.equal(u.long(), v) for u, v in zip(labels, x["labels"]))
    assert torch.equal(rows, x["pmap"])
    t8 = pack_targets(x["boxes"], x["labels"], x["pmap"], gmax=8)
    assert t8.boxes.shape == (3, 8, 4) and torch.equal(t8.boxes[:, :7], t.boxes)
    with pytest.raises(ValueError):
        pack_targets(x["boxes"], x["labels"], x["pmap"], gmax=3)
    with pytest.raises(ValueError):
        pack_targets(x["boxes"], x["labels"], x["pmap"][:-1])


def _train_cfg(**fuse):
    cfg = gc.head_cfg(convs=1, **fuse)
    c = ac.cfg()
    for k, v in vars(c.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, k, v)
    cfg.MODEL.ATSS, cfg.MODEL.RPN_ONLY = c.MODEL.ATSS, True
    return cfg


def test_unsupported_switches_raise():
    from fiber_amd.modules.grounding_train import ATSSLossComputation
    ok = ATSSLossComputation(_train_cfg())
    assert ok.topk == 9 and ok.reg_loss_weight == 2.0
    with pytest.raises(NotImplementedError, match="USE_CLASSIFICATION_LOSS"):
        ATSSLossComputation(_train_cfg(USE_CLASSIFICATION_LOSS=True))
    cfg = _train_cfg()
    cfg.MODEL.RPN_ONLY = False
    with pytest.raises(NotImplementedError, match="RPN_ONLY"):
        ATSSLossComputation(cfg)
    for key in ("USE_TOKEN_LOSS", "USE_CONTRASTIVE_ALIGN_LOSS", "USE_SHALLOW_CONTRASTIVE_LOSS", "MLM_LOSS"):
        with pytest.raises(NotImplementedError, match=key):
            ATSSLossComputation(_train_cfg(**{key: True}))
    cfg = _train_cfg()
    cfg.MODEL.RPN.ASPECT_RATIOS = (0.5, 1.0)
    with pytest.raises(NotImplementedError, match="ASPECT_RATIOS"):
        ATSSLossComputation(cfg)


def test_training_forward_without_targets_still_raises():
    from fiber_amd.modules import VLDyHeadModule
    import detect_cases as dc
    cfg = _train_cfg()
    d = dc.cfg_for("detect_small")
    cfg.MODEL.ATSS, cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = d.MODEL.ATSS, "MEAN", d.TEST
    m = VLDyHeadModule(cfg).train()
    with pytest.raises(NotImplementedError, match="targets"):
        m([(160, 224)], [torch.zeros(1, 256, 20, 28)], {"embedded": torch.zeros(1, 256, 768)}, {1: [3]})
    assert all(k.startswith("head.") for k in m.state_dict())


def _normaliser_worker(rank, port, out_dir):
    import torch.distributed as dist
    from fiber_amd.modules.grounding_train import normalisers
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        num_pos = torch.tensor([[3, 4], [0, 0]][rank], dtype=torch.int32)
        sum_ctr = torch.tensor([2.5, 0.0][rank])
        n, s = normalisers(num_pos, sum_ctr)
        n0, s0 = normalisers(torch.zeros(2, dtype=torch.int32), torch.tensor(0.0))
        torch.save((float(n), float(s), float(n0), float(s0)), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_normalisers_under_gloo(tmp_path):
    from fiber_amd.modules.grounding_train import normalisers
    n, s = normalisers(torch.tensor([3, 4], dtype=torch.int32), torch.tensor(2.5))
    assert float(n) == 7.0 and float(s) == 2.5               # no process group: plain
    assert float(normalisers(torch.zeros(2, dtype=torch.int32), torch.tensor(0.0))[0]) == 1.0
    mp_util.spawn_with_retry(_normaliser_worker, lambda port: (port, str(tmp_path)), nprocs=2, deadline_s=120)
    for r in range(2):
        n, s, n0, s0 = torch.load(os.path.join(str(tmp_path), f"r{r}.pt"))
        assert (n, s) == (3.5, 1.25), "sum over the ranks / world size"
        assert (n0, s0) == (1.0, 0.0), "max(0 / 2, 1)"
