"""MLMDecoder — drop-in for espnet2/asr/decoder/mlm_decoder.py:22-130 (the Mask-CTC masked-LM decoder).

A TransformerDecoder whose embedding and output layer have vocab_size + 1 rows (the last one is <mask>) and whose
self-attention is not causal: the reference's target mask is valid(i) & valid(j) (mlm_decoder.py:111-115).  Same
state_dict keys and shapes as the reference class (embed.0.weight, decoders.N.*, after_norm.*, output_layer.*), the
same kernels and explicit backward as TransformerDecoder; only the self-attention's causal flag differs.

Padded query rows (i >= ys_in_len_b) need no special handling.  The kernels let such a row attend the valid keys,
where the reference zeroes its attention; every such row has ys_out == ignore_id, and a row of source attention, of
an FFN or of a LayerNorm does not mix with other rows (and a padded row is never a valid key), so neither the loss
nor any gradient sees the difference.  forward()'s logits at padded rows therefore differ from the reference's.

Unsupported options raise like TransformerDecoder's: the `embed` input layer (not `linear`), pre-LN, output layer.

Inference (MaskCTCInference): prepare_memory (inherited) projects every layer's source-attention keys and values of
the encoder output once; forward_masked runs the L rows of one utterance over it, once per refinement pass, and
forward_masked_batch the rows of several ragged utterances of one prepared batch in the same launches.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ... import kernels as K
from ...blocks import Seeds, empty
from ..encoder.abs_encoder import pos_table
from .transformer_decoder import PreparedMemory, TransformerDecoder


class MLMDecoder(TransformerDecoder):
    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4,
                 linear_units: int = 2048, num_blocks: int = 6, dropout_rate: float = 0.1,
                 positional_dropout_rate: float = 0.1, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, input_layer: str = "embed",
                 use_output_layer: bool = True, pos_enc_class=None, normalize_before: bool = True,
                 concat_after: bool = False):
        super().__init__(vocab_size + 1, encoder_output_size, attention_heads, linear_units, num_blocks, dropout_rate,
                         positional_dropout_rate, self_attention_dropout_rate, src_attention_dropout_rate, input_layer,
                         use_output_layer, pos_enc_class, normalize_before, concat_after)
        for layer in self.decoders:
            layer.causal = False

    def forward_one_step(self, tgt, tgt_mask, memory, cache=None):
        raise NotImplementedError("MLMDecoder is not autoregressive: no one-step interface (use forward_masked)")

    def forward_masked(self, y_in: torch.Tensor, mem: PreparedMemory) -> torch.Tensor:
        """One whole-sequence pass of one utterance in eval mode: y_in (L,) int64 on the device (tokens and
        <mask>), mem a PreparedMemory of that utterance -> raw logits (L, vocab_size + 1).  Self-attention over the L
        rows is non-causal, on the generic attention kernels with B = 1; source attention reads the prepared
        keys and values with esp_decode_attn, the L rows as decode rows of utterance 0.  No host synchronisation."""
        self._eval_only("forward_masked")
        if mem.U != 1:
            raise ValueError(f"forward_masked: a memory of {mem.U} utterances (one utterance at a time)")
        L, D = int(y_in.shape[0]), self.D
        H = self.decoders[0].self_attn.h
        dk = D // H
        dev = mem.kv.device
        with torch.no_grad():
            pe = pos_table("abs", max(512, 1 << (L - 1).bit_length()), D, dev)
            x = torch.empty(L, D, dtype=torch.float32, device=dev)
            K.embed_fwd(y_in, self.embed[0].weight, pe, x, L, math.sqrt(D), 0.0, 0)
            klen = self._klen(L, dev)
            src_idx = mem.index(np.zeros(L, dtype=np.int32))
            seeds = Seeds(0)
            ctx = empty(L, D, like=x)
            for l, layer in enumerate(self.decoders):
                ca = layer.src_attn
                h, _ = layer.norm1.fwd(x)
                x, _ = layer.self_attn.fwd(h, x, 1, L, klen, False, 0.0, seeds, False)
                h, _ = layer.norm2.fwd(x)
                q = ca.linear_q.fwd(h)
                kv = mem.kv[l]
                K.decode_attn(q, D, 0, kv, 2 * D, mem.T * 2 * D, 0, kv, 2 * D, mem.T * 2 * D, D, ctx, D, 0, src_idx, H,
                              dk, mem.U, mem.T)
                x = ca.linear_out.fwd(ctx, R=x, beta=1.0)
                h, _ = layer.norm3.fwd(x)
                x, _ = layer.feed_forward.fwd(h, x, 1.0, 0.0, seeds, False)
            y, _ = self.after_norm.fwd(x)
            return self.output_layer.fwd(y)

    def forward_masked_batch(self, y_in: torch.Tensor, ylens, mem: PreparedMemory, rows) -> torch.Tensor:
        """forward_masked for Ua sequences in one pass: y_in (Ua, Lmax) int64 on the device (a valid id at the padded
        positions), ylens their lengths (host, all >= 1), mem a PreparedMemory of U utterances, rows (Ua,) the
        utterance of mem each sequence reads -> raw logits (Ua * Lmax, vocab_size + 1).  Position i of every sequence
        gets pe[i]; self-attention is non-causal on the generic kernels with B = Ua and ylens as key counts; source
        attention sends the Lmax rows of sequence a to utterance rows[a] with that utterance's memory length.  The
        logits of padded rows (i >= ylens[a]) are not meant to be read; as keys those rows are masked by the key
        count.  The key counts and the launch index are kept while (ylens, rows) repeat: every pass of a batch.  No
        host synchronisation."""
        self._eval_only("forward_masked_batch")
        Ua, Lmax = (int(n) for n in y_in.shape)
        D = self.D
        H = self.decoders[0].self_attn.h
        dk = D // H
        dev = mem.kv.device
        ylens = np.asarray(ylens, dtype=np.int32).reshape(-1)
        rows = np.asarray(rows, dtype=np.int32).reshape(-1)
        if ylens.shape[0] != Ua or rows.shape[0] != Ua or ylens.min() < 1 or ylens.max() > Lmax:
            raise ValueError(f"forward_masked_batch: lengths {ylens.tolist()} / utterances {rows.tolist()} for "
                             f"{Ua} sequences of {Lmax} positions (every length in [1, {Lmax}])")
        with torch.no_grad():
            pe = pos_table("abs", max(512, 1 << (Lmax - 1).bit_length()), D, dev)
            x = torch.empty(Ua * Lmax, D, dtype=torch.float32, device=dev)
            K.embed_fwd(y_in, self.embed[0].weight, pe, x, Lmax, math.sqrt(D), 0.0, 0)
            klen = self._klens(ylens, dev)
            src_idx = mem.index(np.repeat(rows, Lmax))
            seeds = Seeds(0)
            ctx = empty(Ua * Lmax, D, like=x)
            for l, layer in enumerate(self.decoders):
                ca = layer.src_attn
                h, _ = layer.norm1.fwd(x)
                x, _ = layer.self_attn.fwd(h, x, Ua, Lmax, klen, False, 0.0, seeds, False)
                h, _ = layer.norm2.fwd(x)
                q = ca.linear_q.fwd(h)
                kv = mem.kv[l]
                K.decode_attn(q, D, 0, kv, 2 * D, mem.T * 2 * D, 0, kv, 2 * D, mem.T * 2 * D, D, ctx, D, 0, src_idx, H,
                              dk, mem.U, mem.T)
                x = ca.linear_out.fwd(ctx, R=x, beta=1.0)
                h, _ = layer.norm3.fwd(x)
                x, _ = layer.feed_forward.fwd(h, x, 1.0, 0.0, seeds, False)
            y, _ = self.after_norm.fwd(x)
            return self.output_layer.fwd(y)

    def _klens(self, ylens: np.ndarray, dev) -> torch.Tensor:
        """The self-attention key counts of a batch on the device (kept while they repeat: every pass of a batch)."""
        key = (ylens.tobytes(), str(dev))
        c = getattr(self, "_klens_cache", None)
        if c is None or c[0] != key:
            c = (key, K.h2d(torch.from_numpy(np.ascontiguousarray(ylens)), dev))
            self._klens_cache = c
        return c[1]

    def _klen(self, L: int, dev) -> torch.Tensor:
        """The self-attention key count [L] on the device (kept while L repeats: every pass of an utterance)."""
        c = getattr(self, "_klen_cache", None)
        if c is None or c[0] != (L, str(dev)):
            c = ((L, str(dev)), K.h2d(torch.tensor([L], dtype=torch.int32), dev))
            self._klen_cache = c
        return c[1]
