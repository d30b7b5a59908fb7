"""Host-side pieces of COCO caption fine-tuning (caption_mle) that need no GPU: the model's caption modules and state-dict keys, the
DDP unused-parameter list, the named config, optimizer grouping, the decoder mask, the refusal of the tasks still out of scope and the
result-file wrap-up."""
import json

import pytest
import torch

from oracle import cases


def _model(base, **over):
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS
    torch.manual_seed(0)
    return FIBERTransformerSS(make_config(**dict(base, **over)))


@pytest.fixture(scope="module")
def tiny():
    return _model(cases.TINY, loss_names={"caption_mle": 1})


def test_caption_model_builds_with_reference_modules(tiny):
    c = tiny.config
    dim = c["input_image_embed_size"]
    assert len(tiny.cross_modal_att_layers) == c["num_layers"] - 2                     # fiber_module.py:116-128: all ten in the state dict
    for lt in tiny.cross_modal_att_layers:
        assert tuple(lt.weight.shape) == (dim // 2, dim) and tuple(lt.bias.shape) == (dim // 2,)
        assert float(lt.bias.detach().abs().max()) == 0.0                                        # objectives.init_weights
    plain = _model(cases.TINY)                                                          # mlm + itm
    keys, pkeys = set(tiny.state_dict()), set(plain.state_dict())
    added = keys - pkeys
    assert added == {f"cross_modal_att_layers.{i}.{w}" for i in range(c["num_layers"] - 2) for w in ("weight", "bias")}
    assert pkeys - keys == {k for k in pkeys if k.startswith(("itm_score.", "rank_output."))}
    assert any(k.startswith("mlm_score.") for k in keys)


def test_unused_parameters_of_a_caption_model(tiny):
    names = set(tiny.unused_parameter_names())
    params = dict(tiny.named_parameters())
    assert names <= set(params)
    first_fuse = tiny.num_text_layer - tiny.num_fuse_block
    for i in range(tiny.num_text_layer - 2):
        assert (f"cross_modal_att_layers.{i}.weight" in names) == (i < first_fuse)
    for n in params:
        if n.startswith("vit_model.") and "i2t" in n or n.startswith(("vit_model.norm.", "cross_modal_image_")) or "pooler" in n:
            assert n in names, n
    for i in range(tiny.num_text_layer):                                                # every text layer runs, LayerNorms included
        assert f"text_transformer.encoder.layer.{i}.output.LayerNorm.weight" not in names
        assert f"text_transformer.encoder.layer.{i}.attention.self.query.weight" not in names
    assert "text_transformer.encoder.layer.7.crossattention_t2i.self.key.weight" not in names
    assert "vit_model.layers.3.blocks.1.attn.qkv.weight" not in names and "vit_model.layers.2.downsample.reduction.weight" not in names


def test_unused_parameters_swin_t_keeps_layers_6_to_9():
    """On Swin-T infer() never runs text layers 6..9; infer_caption does, so a caption model must not list them."""
    m = _model(cases.SWIN_T, loss_names={"caption_mle": 1})
    names = set(m.unused_parameter_names())
    for i in range(6, 10):
        assert not any(n.startswith(f"text_transformer.encoder.layer.{i}.") and "alpha_t2i" not in n
                       and "crossattention_t2i.output.LayerNorm" not in n for n in names), i
    i2t = [n for n, _ in m.named_parameters() if n.startswith("vit_model.") and "i2t" in n]
    assert i2t and set(i2t) <= names


def test_named_caption_config():
    from fiber_amd.config import named_config
    c = named_config("task_finetune_caption_mle_coco")
    assert c["loss_names"]["caption_mle"] == 1 and sum(c["loss_names"].values()) == 1
    assert (c["exp_name"], c["datasets"], c["batch_size"], c["max_epoch"], c["max_steps"]) == ("finetune_caption_mle_coco", ["coco"], 512, 10, None)
    assert (c["warmup_steps"], c["learning_rate"], c["lr_mult_cross_modal"], c["lr_mult_head"]) == (0.1, 5e-5, 5, 5)
    assert (c["max_text_len"], c["image_size"], c["pretrained_vit"]) == (50, 576, False)
    assert c["train_transform_keys"] == ["albef_randaug"] and c["val_transform_keys"] == ["albef"]


def test_schedule_groups_caption_modules(tiny):
    from fiber_amd.modules import fiber_utils
    (opt,), _ = fiber_utils.set_schedule(tiny)
    group_of = {id(p): gi for gi, g in enumerate(opt.param_groups) for p in g["params"]}
    for n, p in tiny.named_parameters():
        if n.startswith("cross_modal_att_layers."):
            assert group_of[id(p)] in (4, 5), n
        if n.startswith("mlm_score."):
            assert group_of[id(p)] in (2, 3), n


@pytest.mark.parametrize("task", ["caption_gold", "caption_cider", "nlvr2"])
def test_other_tasks_still_refused(task):
    with pytest.raises(NotImplementedError):
        _model(cases.TINY, loss_names={task: 1})


def test_decoder_mask_and_dense_mask_refusal(tiny):
    from fiber_amd.modules import roberta
    m = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1]])
    d = roberta._prepare_decoder_attention_mask(m, m.shape, torch.zeros(2, 4, 8), "cpu")
    assert d.causal and d.kmask.dtype == torch.float32 and tuple(d.kmask.shape) == (2, 4)
    assert d.kmask[0, 3] == torch.finfo(torch.float32).min and float(d.kmask[0, :3].abs().max()) == 0.0 and float(d.kmask[1].abs().max()) == 0.0
    assert roberta._prepare_decoder_attention_mask(None, m.shape, torch.zeros(2, 4, 8), "cpu").kmask is None
    from fiber_amd import ops
    for causal in (True, False):                                                        # [B, 1, L, L] would be misread as a key mask
        with pytest.raises(ValueError):
            ops.mha_qkv_packed(torch.zeros(8, 3 * 64), torch.zeros(2, 1, 4, 4), 2, 2, 0.125, causal=causal)


def test_caption_test_wrapup_writes_result(tmp_path, monkeypatch):
    from fiber_amd.modules import objectives
    monkeypatch.chdir(tmp_path)
    outs = [{"image_ids": [5, 7], "captions": ["a dog", "a cat"]}, {"image_ids": [5, 9], "captions": ["dup", "a bird"]}]
    objectives.caption_test_wrapup(outs, "model")
    got = json.loads((tmp_path / "result" / "caption.json").read_text())
    assert got == [{"image_id": 5, "caption": "a dog"}, {"image_id": 7, "caption": "a cat"}, {"image_id": 9, "caption": "a bird"}]
    assert not (tmp_path / "caption_0.json").exists()


@pytest.mark.parametrize("name", ["caption_tiny", "caption_swin_t", "caption_swin_b_576"])
def test_caption_state_dict_and_unused_list_match_reference(name, golden):
    """Against the reference's caption model (tests/golden/caption_*.npz, tools/gen_caption_golden.py): the sorted state-dict keys, and the
    parameters that get no gradient from the reference's compute_caption_mle -- the list DDP relies on."""
    from tests import caption_cases as cc
    gold = golden(name)
    m = _model(cc.CAPTION_CASES[name]["config"])
    assert sorted(m.state_dict().keys()) == gold["keys"].tolist()
    assert m.unused_parameter_names() == sorted(gold["unused_params"].tolist())
