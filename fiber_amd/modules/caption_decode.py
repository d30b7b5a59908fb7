"""KV-cached decoding of the caption model: one new token per step through the causal text stack.

infer_caption, run per generated token as the reference does, recomputes every text layer on the whole sequence to use one position of
the result and re-projects the image tokens to keys and values in every fusion layer, per beam.  The image tokens never change while
decoding and are the same for the beams of an image; a causal layer's keys and values of the positions before t do not change either
(tests/test_hip_caption.py::test_causal_no_look_ahead_exact).  CaptionDecoder therefore keeps

  * per fusion layer the image keys | values, [bs, Li, 2C], ONCE PER IMAGE (ops.mha_decode_cross serves an image's rows from one fetch),
  * per text layer a self-attention cache [N, max_text_len, 2C] for N = bs * rows_per_image row slots,
  * one int32 ancestry table [N, max_text_len]: anc[n, j] is the slot that holds position j of row n's sequence (-1: padding under a key mask).

A beam reorder gathers the ancestry table -- never a cache: slot n only ever receives the token row n processes, and
ops.mha_decode_self follows anc to the slots of the row's ancestors.  Evaluation arithmetic only (no dropout, no gradient), the layers in
RobertaLayer.forward's order on [N, 1, C] rows through the same ops.  The small-M GEMMs of a step stay the tile kernels' business.
"""
import math

import torch

from .. import ops


class CaptionDecoder:
    """decoder = model.caption_decoder(image_embeds, rows_per_image); feats = decoder.step(tokens, parent) once per position."""

    @torch.no_grad()
    def __init__(self, model, image_embeds, rows_per_image):
        if ops.residual_fp32():
            raise NotImplementedError("CaptionDecoder with residual_dtype='fp32' is not built: the single-token layers run on the bf16 stream")
        txt = model.text_transformer
        self.model, self.layers = model, list(txt.encoder.layer)
        self.rows_per_image = int(rows_per_image)
        self.max_len = int(model.hparams.config["max_text_len"])
        if self.max_len > ops.DECODE_MAX_LEN:
            raise NotImplementedError(f"CaptionDecoder: max_text_len {self.max_len} exceeds the decode kernel's {ops.DECODE_MAX_LEN}")
        if not 1 <= self.rows_per_image <= ops.DECODE_MAX_ROWS:
            raise NotImplementedError(f"CaptionDecoder: {rows_per_image} rows per image (1 .. {ops.DECODE_MAX_ROWS})")
        bs, dev = image_embeds.shape[0], image_embeds.device
        self.N = N = bs * self.rows_per_image
        att = self.layers[0].attention.self
        self.heads, self.scale = att.num_attention_heads, 1.0 / math.sqrt(att.attention_head_size)
        C = att.all_head_size
        n_layers, first_fuse = len(self.layers), len(self.layers) - model.num_fuse_block
        self.image_kv = {}
        for i in range(first_fuse, n_layers):                # infer_caption: the top two fusion layers attend to the image tokens themselves
            enc = image_embeds
            if i < n_layers - 2:
                lt = model.cross_modal_att_layers[i]
                enc = ops.linear(image_embeds, lt.weight, lt.bias)
            ca = self.layers[i].crossattention_t2i.self
            self.image_kv[i] = ops.linear_packed(enc, [(ca.key.weight, ca.key.bias), (ca.value.weight, ca.value.bias)]).detach()
        self.caches = [torch.zeros((N, self.max_len, 2 * C), dtype=torch.bfloat16, device=dev) for _ in self.layers]
        self.anc = torch.zeros((N, self.max_len), dtype=torch.int32, device=dev)
        self.own = torch.arange(N, dtype=torch.int32, device=dev)
        self.ids = torch.full((N, self.max_len), txt.embeddings.padding_idx, dtype=torch.long, device=dev)
        self.t = 0

    def _embed(self, t):
        """Row t of text_transformer.embeddings(ids[:, :t + 1]) in evaluation mode, bit for bit: the embedding kernel over the prefix (RoBERTa
        positions count the non-pad tokens so far, and an ended beam feeds pads), last row taken"""
        e = self.model.text_transformer.embeddings
        y = ops.roberta_embed(self.ids[:, :t + 1].contiguous(), e.word_embeddings.weight, e.position_embeddings.weight,
                              e.token_type_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias, pad=e.padding_idx, eps=e.LayerNorm.eps,
                              p_drop=0.0, training=False)
        return y[:, t:t + 1].contiguous()

    @torch.no_grad()
    def step(self, tokens, parent=None, live=None):
        """tokens int64 [N]: the token each row puts at position t (t counts the calls); parent int64 [N] or None: the row of the previous
        step that row n continues (None: itself); live bool [N] or None: column t of infer_caption's text_masks -- False marks padding, which
        is then no key for this or any later position (None, as the decoding loops run with text_masks None: every position is a key).
        -> the cross_modal_text_transform'ed features of the new position, [N, hidden_size]."""
        t, N = self.t, self.N
        if t >= self.max_len:
            raise ValueError(f"CaptionDecoder.step: position {t} is past max_text_len {self.max_len}")
        tokens = tokens.reshape(-1)
        if tokens.numel() != N:
            raise ValueError(f"CaptionDecoder.step: {tokens.numel()} tokens for {N} rows")
        if parent is not None and t > 0:
            parent = parent.reshape(-1)
            self.anc = self.anc.index_select(0, parent)      # the reorder: [N, L] int32, whatever the caches hold
            self.ids = self.ids.index_select(0, parent)
        self.anc[:, t] = self.own if live is None else torch.where(live.reshape(-1).bool(), self.own, torch.full_like(self.own, -1))
        self.ids[:, t] = tokens
        x = self._embed(t)
        C, heads, scale = x.shape[-1], self.heads, self.scale
        for i, layer in enumerate(self.layers):
            sa, so = layer.attention.self, layer.attention.output
            qkv = ops.linear_packed(x, [(sa.query.weight, sa.query.bias), (sa.key.weight, sa.key.bias), (sa.value.weight, sa.value.bias)])
            o = ops.mha_decode_self(qkv.view(N, 3 * C), self.caches[i], self.anc, t, heads, scale).view(N, 1, C)
            if i not in self.image_kv:
                a = ops.linear(o, so.dense.weight, so.dense.bias, residual=x)
            else:
                a = ops.linear(o, so.dense.weight, so.dense.bias)
                ca = layer.crossattention_t2i
                q = ops.linear(a, ca.self.query.weight, ca.self.query.bias).view(N, C)
                c = ops.mha_decode_cross(q, self.image_kv[i], self.rows_per_image, heads, scale).view(N, 1, C)
                c = ops.linear(c, ca.output.dense.weight, ca.output.dense.bias)
                a = ops.stream_add(x, a, b=c, alpha=layer.alpha_t2i, training=False)
            ln = so.LayerNorm
            a = ops.layernorm(a, ln.weight, ln.bias, ln.eps)
            fi, fo = layer.intermediate.dense, layer.output
            h = ops.mlp(a, fi.weight, fi.bias, fo.dense.weight, fo.dense.bias, residual=a)
            x = ops.layernorm(h, fo.LayerNorm.weight, fo.LayerNorm.bias, fo.LayerNorm.eps)
        tt = self.model.cross_modal_text_transform
        self.t = t + 1
        return ops.linear(x, tt.weight, tt.bias).view(N, -1)
