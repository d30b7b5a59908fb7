"""Detection prompts of the fine-grained model: a category list -> the captions the model reads and the maps from their tokens to classes.

Mirrors fine_grained/maskrcnn_benchmark/engine/inference.py: clean_name (:80-84), create_positive_dict (:106-139), chunks (:142-153),
create_queries_and_maps_from_dataset (:156-191) and create_queries_and_maps (:194-270).  With TEST.CHUNKED_EVALUATION = n the reference cuts
the sorted categories into chunks of n, writes one caption per chunk ("name. name. ...") and runs the model once per (image, chunk); LVIS
(1203 categories, n = 40) takes 31 captions.

Differences in the call surface, none in the strings or the spans:
  * no tokenizer files are assumed: `tokenizer` is the caller's, called as tokenizer(query); its result has `input_ids` and
    `char_to_token(i)` as a Hugging Face fast tokenizer's has;
  * the positive maps carry CHUNK-LOCAL labels 1..n_k (the reference keys them by global category id and scores
    TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = 3000 classes per launch, nearly all of them empty): the score, top-k and decode launches of a
    chunk are C = n wide, and `label_table` takes (chunk, local class) to the label BoxAPEvaluator reads;
  * a caption of more than max_query_len tokens raises (the reference's tokenizer call does not truncate, and the model's 256 positions
    would be indexed out of range).
As in the reference, `caption_prompt` is indexed by a category's position inside its chunk.
"""
import re

import torch

from ..data import pad_input_ids
from .grounding_inference import pack_positive_maps


def clean_name(name):
    """:80-84"""
    name = re.sub(r"\(.*\)", "", name)
    name = re.sub(r"_", " ", name)
    name = re.sub(r"  ", " ", name)
    return name


def _char_to_token(tokenized, first, *fallbacks):
    """create_positive_dict's lookup (:115-130): the first position, then the fallbacks while the answer is None; an exception in a
    fallback ends the search with None"""
    pos = tokenized.char_to_token(first)
    if pos is None:
        try:
            for i in fallbacks:
                pos = tokenized.char_to_token(i)
                if pos is not None:
                    break
        except Exception:
            pos = None
    return pos


def query_and_spans(names, separation_tokens=". ", caption_prompt=None, additional_labels=None):
    """create_queries_and_maps (:196-234) up to the tokenizer -> (query, [(start, end)] per name)"""
    names = [clean_name(n) for n in names]
    spans, query = [], ""
    for i, name in enumerate(names):
        if caption_prompt is not None:
            query += caption_prompt[i]["prefix"]
        start = len(query)
        query += caption_prompt[i]["name"] if caption_prompt is not None else name
        spans.append((start, len(query)))
        if caption_prompt is not None:
            query += caption_prompt[i]["suffix"]
        if i != len(names) - 1:
            query += separation_tokens
    if additional_labels is not None:
        query += separation_tokens
        for i, label in enumerate(additional_labels):
            query += label
            if i != len(additional_labels) - 1:
                query += separation_tokens
    return query, spans


class DetectionPrompts:
    """K prompts over one category list: queries (K strings), input_ids / attention_mask int64 [K, L], positive_maps (K dicts: chunk-local
    label 1..n_k -> token positions), packed (PackedPositiveMaps [K, Cc + 1], Cc = max n_k), label_table int32 [K, Cc] (local class c of
    chunk k -> (index of its category in the sorted ids) + 1, the label BoxAPEvaluator reads; 0 where chunk k has no class c),
    category_ids (the sorted ids) and unmapped (ids of the categories whose name has no token span: their rows are empty and score -1)."""

    def __init__(self, queries, input_ids, attention_mask, positive_maps, packed, label_table, category_ids, unmapped):
        self.queries, self.input_ids, self.attention_mask, self.positive_maps = queries, input_ids, attention_mask, positive_maps
        self.packed, self.label_table, self.category_ids, self.unmapped = packed, label_table, list(category_ids), list(unmapped)

    def __len__(self):
        return len(self.queries)

    @property
    def chunk_width(self):
        return self.packed.num_classes

    def to(self, device):
        """Stream-ordered copies (non_blocking): nothing here waits for the device"""
        have, device = self.input_ids.device, torch.device(device)
        if have.type == device.type and device.index in (None, have.index):
            return self
        return DetectionPrompts(self.queries, self.input_ids.to(device, non_blocking=True), self.attention_mask.to(device, non_blocking=True),
                                self.positive_maps, self.packed.to(device), self.label_table.to(device, non_blocking=True),
                                self.category_ids, self.unmapped)


def build_detection_prompts(categories, tokenizer, chunk=-1, separation_tokens=". ", caption_prompt=None, additional_labels=None,
                            max_query_len=256, pad_max=True, pad_id=1):
    """categories: [{"id", "name", ...}] in ascending id order (the list BoxAPEvaluator takes); chunk: categories per prompt
    (TEST.CHUNKED_EVALUATION), -1 = one prompt for all; separation_tokens / caption_prompt / additional_labels: DATASETS.SEPARATION_TOKENS,
    DATASETS.CAPTION_PROMPT (when USE_CAPTION_PROMPT) and DATASETS.SUPRESS_QUERY (when USE_SUPRESS_QUERY); max_query_len / pad_max:
    LANGUAGE_BACKBONE.MAX_QUERY_LEN / PAD_MAX.  -> DetectionPrompts on the host."""
    ids = [c["id"] for c in categories]
    if not ids or ids != sorted(set(ids)):
        raise ValueError("build_detection_prompts: categories is a non-empty list of {'id', 'name'} in ascending id order without repeats")
    if chunk != -1 and int(chunk) <= 0:
        raise ValueError(f"build_detection_prompts: chunk {chunk} (a positive number of categories per prompt, or -1 for one prompt)")
    n = len(ids) if chunk == -1 else int(chunk)
    groups = [list(range(i, min(i + n, len(ids)))) for i in range(0, len(ids), n)]
    Cc = max(len(g) for g in groups)
    queries, token_ids, maps, unmapped = [], [], [], []
    table = torch.zeros((len(groups), Cc), dtype=torch.int32)
    for k, group in enumerate(groups):
        query, spans = query_and_spans([categories[i]["name"] for i in group], separation_tokens, caption_prompt, additional_labels)
        tokenized = tokenizer(query)
        toks = torch.as_tensor(tokenized["input_ids"] if isinstance(tokenized, dict) else tokenized.input_ids, dtype=torch.int64).reshape(-1)
        if toks.numel() > max_query_len:
            raise ValueError(f"build_detection_prompts: the prompt of chunk {k} ({len(group)} categories from id {ids[group[0]]}) has "
                             f"{toks.numel()} tokens, more than max_query_len = {max_query_len}: use a smaller chunk")
        positive = {}
        for local, (i, (beg, end)) in enumerate(zip(group, spans), start=1):
            table[k, local - 1] = i + 1
            beg_pos = _char_to_token(tokenized, beg, beg + 1, beg + 2)
            end_pos = _char_to_token(tokenized, end - 1, end - 2, end - 3)
            if beg_pos is None or end_pos is None or end_pos < beg_pos:      # (:131-137: `continue`, or a loop over no position)
                unmapped.append(ids[i])
                continue
            positive[local] = list(range(beg_pos, end_pos + 1))
        queries.append(query)
        token_ids.append(toks)
        maps.append(positive)
    padded = pad_input_ids(token_ids, max_query_len, pad_max, pad_id)
    return DetectionPrompts(queries, padded["input_ids"], padded["attention_mask"], maps, pack_positive_maps(maps, Cc), table, ids, unmapped)
