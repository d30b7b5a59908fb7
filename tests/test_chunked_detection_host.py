"""Host tests of chunked open-vocabulary detection: the prompts of modules/detection_prompts.py against strings and token lists written
out here, ops.det_merge's host path against the independent reference of tests/chunk_cases.py, and the wrapper's refusals."""
import pytest
import torch

import chunk_cases as cc
from fiber_amd import ops
from fiber_amd.modules import DetectionPrompts, Detections, build_detection_prompts, clean_name

TOK = cc.StubTokenizer()
CATS = cc.PAIR["categories"]


def _ids(tokens, length=256):
    ids = [0 if t == "<s>" else 2 if t == "</s>" else cc.StubTokenizer.word_id(t) for t in tokens]
    return ids + [1] * (length - len(ids))


def test_clean_name():
    assert clean_name("traffic_light") == "traffic light"
    assert clean_name("dog (animal)") == "dog "
    assert clean_name("hot  dog") == "hot dog"
    assert clean_name("a___(b)") == "a  "                    # ONE pass over double blanks, as the reference's single re.sub


def test_one_prompt_for_all():
    p = build_detection_prompts(CATS, TOK)
    assert isinstance(p, DetectionPrompts) and len(p) == 1 and p.chunk_width == 5
    assert p.queries == ["traffic light. dog . hot dog. cup. bird"]
    tokens = ["<s>", "traffic", "light", ".", "dog", ".", "hot", "dog", ".", "cup", ".", "bird", "</s>"]
    assert TOK(p.queries[0]).tokens == tokens
    assert p.input_ids.dtype == torch.int64 and p.input_ids.tolist() == [_ids(tokens)]
    assert p.attention_mask.tolist() == [[1] * 13 + [0] * 243]
    assert p.positive_maps == [{1: [1, 2], 2: [4], 3: [6, 7], 4: [9], 5: [11]}]            # "dog ": the end falls back from the blank
    assert p.label_table.dtype == torch.int32 and p.label_table.tolist() == [[1, 2, 3, 4, 5]]
    assert p.packed.class_ptr.tolist() == [[0, 2, 3, 5, 6, 7]] and p.packed.tok_idx.tolist() == [1, 2, 4, 6, 7, 9, 11]
    assert p.category_ids == [4, 9, 10, 21, 22] and p.unmapped == []


def test_chunk_with_a_remainder():
    p = build_detection_prompts(CATS, TOK, chunk=2, pad_max=False)
    assert p.queries == ["traffic light. dog ", "hot dog. cup", "bird"]
    assert p.positive_maps == [{1: [1, 2], 2: [4]}, {1: [1, 2], 2: [4]}, {1: [1]}]
    assert p.label_table.tolist() == [[1, 2], [3, 4], [5, 0]]
    assert p.input_ids.tolist() == [_ids(["<s>", "traffic", "light", ".", "dog", "</s>"], 6), _ids(["<s>", "hot", "dog", ".", "cup", "</s>"], 6),
                                    _ids(["<s>", "bird", "</s>"], 6)]
    assert p.attention_mask.sum(1).tolist() == [6, 6, 3]
    assert p.packed.class_ptr.tolist() == [[0, 2, 3], [3, 5, 6], [6, 7, 7]] and p.packed.tok_idx.tolist() == [1, 2, 4, 1, 2, 4, 1]


def test_chunk_dividing_evenly():
    p = build_detection_prompts(CATS[:4], TOK, chunk=2)
    assert p.queries == ["traffic light. dog ", "hot dog. cup"] and p.label_table.tolist() == [[1, 2], [3, 4]]
    assert p.input_ids.shape == (2, 256) and p.chunk_width == 2
    same = build_detection_prompts(CATS[:4], TOK, chunk=4)
    assert len(same) == 1 and same.queries == build_detection_prompts(CATS[:4], TOK).queries


def test_caption_prompt_and_separator():
    prompt = [dict(prefix="a photo of ", name="mug", suffix=" here"), dict(prefix="the ", name="sparrow", suffix="")]
    p = build_detection_prompts(CATS[3:], TOK, caption_prompt=prompt, separation_tokens=" ; ")
    assert p.queries == ["a photo of mug here ; the sparrow"]
    assert TOK(p.queries[0]).tokens == ["<s>", "a", "photo", "of", "mug", "here", ";", "the", "sparrow", "</s>"]
    assert p.positive_maps == [{1: [4], 2: [8]}]
    chunked = build_detection_prompts(CATS[3:], TOK, chunk=1, caption_prompt=prompt)       # indexed inside the chunk, as the reference
    assert chunked.queries == ["a photo of mug here", "a photo of mug here"]


def test_additional_labels():
    p = build_detection_prompts(CATS[3:], TOK, additional_labels=["person", "car"])
    assert p.queries == ["cup. bird. person. car"] and p.positive_maps == [{1: [1], 2: [3]}]
    assert p.label_table.tolist() == [[1, 2]]
    p = build_detection_prompts(CATS[3:], TOK, chunk=1, additional_labels=["person"])
    assert p.queries == ["cup. person", "bird. person"]


def test_a_name_without_a_span():
    cats = [dict(id=1, name="cup"), dict(id=2, name="_"), dict(id=5, name="(thing)")]
    p = build_detection_prompts(cats, TOK)
    assert p.queries == ["cup.  . "]
    # " " at character 5: the start falls forward onto the second full stop (position 3), the end back onto the first (2): no position
    # "" at the end of the string: no character to look up
    assert p.unmapped == [2, 5] and p.positive_maps == [{1: [1]}]
    assert p.packed.class_ptr.tolist() == [[0, 1, 1, 1]] and p.label_table.tolist() == [[1, 2, 3]]


def test_refusals():
    many = [dict(id=i, name=f"thing{i}") for i in range(1, 301)]
    with pytest.raises(ValueError, match="chunk 0"):
        build_detection_prompts(many, TOK)                   # 300 names and 299 separators
    long_second = [dict(id=1, name="a"), dict(id=2, name="b"), dict(id=3, name="x y z w"), dict(id=4, name="p q r s")]
    assert len(build_detection_prompts(long_second, TOK, chunk=2, max_query_len=11)) == 2            # <s> + 4 + . + 4 + </s> = 11 fit
    with pytest.raises(ValueError, match="chunk 1"):
        build_detection_prompts(long_second, TOK, chunk=2, max_query_len=10)
    with pytest.raises(ValueError, match="ascending"):
        build_detection_prompts([dict(id=2, name="a"), dict(id=1, name="b")], TOK)
    with pytest.raises(ValueError, match="positive number"):
        build_detection_prompts(many[:3], TOK, chunk=0)


def test_lvis_width():
    """1203 categories in chunks of 40: 31 prompts, 40 classes wide, every category in exactly one (chunk, local class)"""
    cats = [dict(id=3 * i + 7, name=f"thing{i} kind") for i in range(1203)]
    p = build_detection_prompts(cats, TOK, chunk=40)
    assert len(p) == 31 and p.chunk_width == 40 and p.label_table.shape == (31, 40) and p.input_ids.shape == (31, 256)
    used = p.label_table[p.label_table > 0]
    assert sorted(used.tolist()) == list(range(1, 1204)) and int((p.label_table[30] > 0).sum()) == 3
    assert p.label_table[7, 5] == 7 * 40 + 5 + 1 and p.category_ids[7 * 40 + 5] == 3 * (7 * 40 + 5) + 7
    assert p.positive_maps[7][6] == [16, 17] and p.unmapped == []          # <s>, then three tokens per name: "thing285", "kind", "."
    assert p.packed.class_ptr.shape == (31, 41) and int(p.packed.class_ptr[30, -1]) == 2 * 1203
    assert int(p.attention_mask[0].sum()) == 40 * 3 - 1 + 2 and int(p.attention_mask[30].sum()) == 3 * 3 - 1 + 2


# ---- ops.det_merge on CPU tensors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.MERGE_CASES))
def test_merge_host_path_against_the_list_reference(name):
    x = cc.merge_inputs(name)
    got, want = ops.det_merge(*cc.merge_args(x)), cc.merge_ref(*cc.merge_args(x))
    for field, g, w in zip(cc.MERGE_FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{name}: {field}"
    assert float(got[1].max()) < cc.JUNK                     # no slot past count got in
    K, D = x["scores"].shape[1:]
    assert got[1].shape[1] == (K * D if x["max_dets"] is None else min(x["max_dets"], K * D))


def test_merge_cases_cover_what_they_claim():
    x = cc.merge_inputs("ties")
    live = x["scores"][0][x["scores"][0] < cc.JUNK]
    assert live.numel() > live.unique().numel()
    assert any(len(set(x["scores"][0, k, :int(x["count"][0, k])].tolist())) < int(x["count"][0, k]) for k in range(3))     # within a chunk
    x = cc.merge_inputs("n_eq_total")
    assert x["max_dets"] == int(x["count"][0].sum()) < int(x["count"][1].sum())
    x = cc.merge_inputs("b3")
    out = ops.det_merge(*cc.merge_args(x))
    Cc = x["label_table"].shape[1]
    assert int(x["labels"][0, 0, 0]) == Cc and int(x["labels"][2, 3, 0]) == Cc + 1
    at = (out[3][2] == x["source"][2, 3, 0]).nonzero()[0, 0]
    assert int(out[2][2, at]) == 0 and int(out[4][2, at]) == 3         # the label that cannot be emitted: label 0, its chunk kept


def test_merge_ties_go_to_the_earlier_chunk_then_slot():
    scores = torch.tensor([[[0.5, 0.5, 0.25], [0.5, 0.25, 0.25]]])
    labels = torch.ones((1, 2, 3), dtype=torch.int32)
    source = torch.arange(6, dtype=torch.int32).view(1, 2, 3)
    out = ops.det_merge(torch.zeros(1, 2, 3, 4), scores, labels, source, torch.tensor([[3, 3]], dtype=torch.int32),
                        torch.tensor([[7], [8]], dtype=torch.int32))
    assert out[3].tolist() == [[0, 1, 3, 2, 4, 5]] and out[4].tolist() == [[0, 0, 1, 0, 1, 1]] and out[2].tolist() == [[7, 7, 8, 7, 8, 8]]


def test_merge_into_given_tensors_and_empty_shapes():
    x = cc.merge_inputs("none")
    want = ops.det_merge(*cc.merge_args(x))
    out = tuple(torch.full_like(t, 77) for t in want)
    back = ops.det_merge(*cc.merge_args(x), out=out)
    assert all(a is b for a, b in zip(back, out)) and all(torch.equal(a, b) for a, b in zip(out, want))
    z = ops.det_merge(x["boxes"][:0], x["scores"][:0], x["labels"][:0], x["source"][:0], x["count"][:0], x["label_table"])
    assert z[0].shape == (0, 12, 4) and z[5].shape == (0,)
    z = ops.det_merge(x["boxes"], x["scores"], x["labels"], x["source"], x["count"], x["label_table"], max_dets=0)
    assert z[1].shape == (2, 0) and z[5].tolist() == [0, 0]


def test_merge_wrapper_refusals():
    x = cc.merge_inputs("none")
    a = dict(zip(("boxes", "scores", "labels", "source", "count", "label_table"), cc.merge_args(x)))
    bad = [dict(scores=a["scores"].double()), dict(boxes=a["boxes"].half()), dict(labels=a["labels"].long()), dict(source=a["source"].long()),
           dict(count=a["count"].long()), dict(label_table=a["label_table"].long()),
           dict(boxes=a["boxes"][:, :, :, :3]), dict(labels=a["labels"][:, :2]), dict(source=a["source"][:1]), dict(count=a["count"][:, :2]),
           dict(label_table=a["label_table"][:2]), dict(label_table=a["label_table"][0]), dict(scores=a["scores"][0]),
           dict(boxes=a["boxes"].reshape(2, 12, 4))]
    for change in bad:
        with pytest.raises(ValueError):
            ops.det_merge(**dict(a, **change))
    with pytest.raises(ValueError, match="max_dets"):
        ops.det_merge(**a, max_dets=-1)
    with pytest.raises(ValueError, match="out must be"):
        ops.det_merge(**a, out=tuple(torch.zeros(1) for _ in range(6)))
    cap = ops.DET_MERGE_MAX_CANDIDATES
    assert cap >= 31 * 300 and cap == ops.det_merge_max_candidates()      # the host path's bound is the kernel's

    def wide(K, D):
        return (torch.zeros(1, K, D, 4), torch.zeros(1, K, D), torch.ones((1, K, D), dtype=torch.int32), torch.zeros((1, K, D), dtype=torch.int32),
                torch.zeros((1, K), dtype=torch.int32), torch.ones((K, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="capacity"):
        ops.det_merge(*wide(65, 2))
    with pytest.raises(ValueError, match="capacity"):
        ops.det_merge(*wide(2, cap // 2 + 1))
    assert ops.det_merge(*wide(64, cap // 64))[5].tolist() == [0]


def test_detections_chunk_defaults_to_none_and_the_loop_checks_the_categories():
    from fiber_amd.modules import BoxAPEvaluator, evaluate_detection_chunked
    d = Detections(torch.zeros(1, 2, 4), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                   torch.zeros(1, dtype=torch.int32))
    assert d.chunk is None
    ev = BoxAPEvaluator(CATS[:4])
    with pytest.raises(ValueError, match="other categories"):
        evaluate_detection_chunked(None, [], ev, build_detection_prompts(CATS, TOK, chunk=2))
