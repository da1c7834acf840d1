"""ContextualBlockTransformerEncoder -- drop-in for espnet2/asr/encoder/contextual_block_transformer_encoder.py
(forward_train, lines 209-361: training, validation and non-streaming decoding) over
espnet/nets/pytorch_backend/transformer/contextual_block_encoder_layer.py and subsampling_without_posenc.py.

After subsampling, the T' frames of an utterance are cut into nblk overlapping blocks of S = block_size + 2 slots:
slot 0 the previous block's context vector, slots 1..bs the frames blk*hop .. blk*hop + bs - 1 (zero past T'),
slot bs + 1 the block's own context vector (the mean of its frame window, through the positional step with the block
index as position when ctx_pos_enc).  Every layer runs on all B*nblk blocks at once as (B*nblk*S, D) rows; before
layer l >= 1 slot 0 of block b is overwritten with the previous layer's output at block max(b - 1, 0), slot bs + 1.
The attention mask is the same for every block (queries 1..bs+1 see keys 0..bs): lengths are ignored in block mode,
as in the reference -- padded frames and the zero tail of the last block are attended and enter the means.  Query
row 0 is dead: its output is overwritten or dropped, so nothing computed at slot 0 after the attention is read.

T' <= block_size or block_size == 0: the plain Transformer stack with the pad mask (pos_enc, layers, after_norm).

Kernels: esp_cbt_chunk / ctx_shift / unchunk for the layout, esp_block_attn_fwd / _bwd for the attention core
(kernels.CBT_ATTN_FUSED; False: MultiHeadedAttention's generic kernels with a key length of bs + 1 per block)."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import nn

from ... import kernels as K
from ...blocks import (Ctx, LayerNorm, MultiHeadedAttention, PositionwiseFeedForward, Seeds, empty, grad_buf,
                       make_subsampling)
from .abs_encoder import StackedEncoder, pos_table
from .transformer_encoder import TransformerEncoderLayer


class BlockLayout:
    """The block layout of T frames (host arithmetic; the kernels of csrc/cbt.hip restate it)."""

    def __init__(self, T: int, block_size: int, hop_size: int, look_ahead: int):
        assert T > block_size > 0
        self.T, self.bs, self.hop, self.la = T, block_size, hop_size, look_ahead
        self.S = block_size + 2
        # math.ceil(float(T - past_size - look_ahead) / float(hop_size)), past_size = bs - hop - la
        self.nblk = -(-(T - block_size + hop_size) // hop_size)

    def window(self, blk: int) -> Tuple[int, int]:
        """Frames [lo, hi) of block blk: its frame slots and the window of its context mean."""
        lo = blk * self.hop
        return lo, min(lo + self.bs, self.T)

    def chunk_source(self):
        """(nblk, S) int: the frame held by each slot; -1 a zero slot, -2 - k the context vector of block k."""
        src = [[-1] * self.S for _ in range(self.nblk)]
        for blk in range(self.nblk):
            lo, hi = self.window(blk)
            for t in range(lo, hi):
                src[blk][t - lo + 1] = t
            src[blk][0] = -2 - max(blk - 1, 0)
            src[blk][self.S - 1] = -2 - blk
        return src

    def output_source(self):
        """(T, 2) int: the (block, slot) every output frame is copied from."""
        first = self.bs - self.la
        out = []
        for t in range(self.T):
            blk = 0 if t < first else min((t - first) // self.hop + 1, self.nblk - 1)
            out.append((blk, t - blk * self.hop + 1))
        return out


class ContextualBlockEncoderLayer(TransformerEncoderLayer):
    """contextual_block_encoder_layer.py:16-138 (pre-LN, no concat): the Transformer layer with the block mask.
    fwd(x, klen, Z, S, seeds, training) -- klen None: block mode on (Z*S, D) rows, Z = B*nblk sequences of S slots
    (the fixed block mask); else the plain layer over Z utterances of S frames."""

    def _attn_fwd(self, h, resid, klen, Z, S, seeds, training):
        a = self.self_attn
        if klen is not None or not (K.CBT_ATTN_FUSED and K.block_attn_ok(S, a.d_k)):
            if klen is None:  # block mode on the generic kernels: keys 0..bs of every block
                klen = _block_klen(Z, S - 1, h.device)
            return super()._attn_fwd(h, resid, klen, Z, S, seeds, training)
        H, dk = a.h, a.d_k
        D = H * dk
        M = Z * S
        w, b = a._w(("linear_q", "linear_k", "linear_v"))
        qkv = empty(M, 3 * D, like=h)
        K.linear_fwd(h, w, b, qkv)
        ctx_ = empty(M, D, like=h)
        lse = empty(Z * H * S, like=h)
        pa = a.p if training else 0.0
        sa = seeds.next()
        K.block_attn_fwd(qkv, ctx_, lse, Z, S, H, dk, pa, sa)
        out = empty(M, D, like=h)
        pr = self.p if training else 0.0
        so = seeds.next()
        a.linear_out.fwd(ctx_, out, drop_p=pr, seed=so, R=resid, beta=1.0)
        return out, Ctx(fused=True, x=h, qkv=qkv, ctx=ctx_, lse=lse, pa=pa, sa=sa, pr=pr, so=so, Z=Z, S=S)

    def _attn_bwd(self, c, dout):
        a = self.self_attn
        if not c.get("fused"):
            return super()._attn_bwd(c, dout)
        H, dk = a.h, a.d_k
        D = H * dk
        dz = grad_buf(dout)
        K.scale_dropout(dout, dz, drop_p=c.pr, seed=c.so)
        dctx = a.linear_out.bwd(dz, c.ctx)
        dqkv = empty(c.Z * c.S, 3 * D, like=dout)
        K.block_attn_bwd(c.qkv, dctx, c.lse, dqkv, c.Z, c.S, H, dk, c.pa, c.sa)
        w, _ = a._w(("linear_q", "linear_k", "linear_v"))
        gw, gb = a._w(("linear_q", "linear_k", "linear_v"), grad=True)
        K.linear_bwd_weight(dqkv, c.x, gw, gb)
        dx = empty(c.Z * c.S, D, like=dout)
        K.linear_bwd_data(dqkv, w, dx)
        return dx


_KLEN = {}


def _block_klen(Z: int, n: int, device) -> torch.Tensor:
    key = (Z, n, str(device))
    t = _KLEN.get(key)
    if t is None:  # never evicted (as abs_encoder's positional tables): a captured step holds only the raw pointer
        t = _KLEN[key] = torch.full((Z,), n, dtype=torch.int32, device=device)
    return t


class ContextualBlockTransformerEncoder(StackedEncoder):
    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 attention_dropout_rate: float = 0.0, input_layer: Optional[str] = "conv2d", pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False, positionwise_layer_type: str = "linear",
                 positionwise_conv_kernel_size: int = 1, padding_idx: int = -1, block_size: int = 40,
                 hop_size: int = 16, look_ahead: int = 16, init_average: bool = True, ctx_pos_enc: bool = True):
        super().__init__(output_size, positional_dropout_rate)
        bad = []
        if input_layer not in ("conv2d", "conv2d6"):
            bad.append(f"input_layer={input_layer}")
        if not normalize_before:
            bad.append("normalize_before=False")
        if concat_after:
            bad.append("concat_after=True")
        if positionwise_layer_type != "linear":
            bad.append(f"positionwise_layer_type={positionwise_layer_type}")
        if pos_enc_class is not None:
            bad.append("pos_enc_class")
        if not init_average:
            bad.append("init_average=False")
        if bad:
            raise NotImplementedError(_UNSUPPORTED + "; got " + ", ".join(bad))
        if block_size < 0 or (block_size != 0 and (hop_size <= 0 or block_size - hop_size - look_ahead < 0
                                                   or look_ahead < 0)):
            raise ValueError(f"block_size={block_size}, hop_size={hop_size}, look_ahead={look_ahead}: need "
                             "hop_size > 0 and block_size - hop_size - look_ahead >= 0")
        self.embed = make_subsampling(input_layer, input_size, output_size, pos_enc=False)
        self.encoders = nn.ModuleList([
            ContextualBlockEncoderLayer(output_size,
                                        MultiHeadedAttention(attention_heads, output_size, attention_dropout_rate),
                                        PositionwiseFeedForward(output_size, linear_units, dropout_rate, K.ACT_RELU),
                                        dropout_rate) for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self.block_size = block_size
        self.hop_size = hop_size
        self.look_ahead = look_ahead
        self.init_average = init_average
        self.ctx_pos_enc = ctx_pos_enc

    def layout(self, T2: int) -> Optional[BlockLayout]:
        """The block layout of T2 subsampled frames; None: the short path (the plain Transformer stack)."""
        if self.block_size == 0 or T2 <= self.block_size:
            return None
        return BlockLayout(T2, self.block_size, self.hop_size, self.look_ahead)

    def run_forward(self, feats, ilens_cpu, seeds: Seeds, training: bool, klen=None, tvalid=None, inter=None):
        """klen (int32 output lengths on device) is read by the short path alone; olens come from the pad mask,
        also in block mode."""
        if tvalid is not None:
            raise NotImplementedError(_UNSUPPORTED + "; got tvalid (length buckets)")
        assert inter is None
        B, olens = self._begin(feats, ilens_cpu)
        L = self.layout(self.embed.out_frames(feats.shape[1]))
        if L is None:  # the plain Transformer stack with the pad mask
            klen = self._klen(klen, olens, feats.device)
            x, c_emb = self._embed_abs(feats, seeds, training)
            x, ctxs = self._layers_fwd(x, klen, B, c_emb.T2, seeds, training)
            return self._finish(x, B, olens, emb=c_emb, layers=ctxs, L=None)
        D = self._output_size
        pp = self.positional_dropout_rate if training else 0.0
        x, c_emb = self.embed.fwd(feats, 1.0, 0.0, seeds, training)
        T2 = c_emb.T2
        assert T2 == L.T
        pe = pos_table("abs", max(T2, L.nblk), D, feats.device)
        sp, sc = seeds.next(), seeds.next()
        Z, S = B * L.nblk, L.S
        y = empty(Z * S, D, like=x)
        K.cbt_chunk_fwd(x, pe, y, B, T2, D, L.bs, L.hop, L.la, L.nblk, math.sqrt(D), self.ctx_pos_enc, pp, sp, sc)
        ctxs = []
        for i, layer in enumerate(self.encoders):
            if i > 0:  # in place, before anything keeps the buffer: slot 0 <- the previous block's context slot
                K.cbt_ctx_shift(y, B, L.nblk, S, D)
            y, c = layer.fwd(y, None, Z, S, seeds, training)
            ctxs.append(c)
        ys = empty(B * T2, D, like=x)
        K.cbt_unchunk_fwd(y, ys, B, T2, D, L.bs, L.hop, L.la, L.nblk)
        return self._finish(ys, B, olens, emb=c_emb, layers=ctxs, pp=pp, sp=sp, sc=sc, L=L)

    def run_backward(self, saved, dhs, grad_hook=None, dfeats=None):
        """dfeats: a (B, T, F) buffer that receives the feature gradient (training passes none: fbank needs none)."""
        L = saved.L
        if L is None:
            return self._embed_bwd(saved.emb, self._layers_bwd(saved, dhs, grad_hook), grad_hook, dfeats)
        B, T2, D = dhs.shape
        dy = self.after_norm.bwd_new(saved.after, dhs.view(B * T2, D))
        if grad_hook is not None:
            grad_hook(self.after_norm)
        d = empty(B * L.nblk * L.S, D, like=dy)
        K.cbt_unchunk_bwd(dy, d, B, T2, D, L.bs, L.hop, L.la, L.nblk)
        for i in range(len(self.encoders) - 1, -1, -1):
            d = self.encoders[i].bwd(saved.layers[i], d)
            saved.layers[i] = None
            if i > 0:
                K.cbt_ctx_shift(d, B, L.nblk, L.S, D, backward=True)
            if grad_hook is not None:
                grad_hook(self.encoders[i])
        dx = empty(B * T2, D, like=d)
        K.cbt_chunk_bwd(d, dx, B, T2, D, L.bs, L.hop, L.la, L.nblk, math.sqrt(D), self.ctx_pos_enc, saved.pp,
                        saved.sp, saved.sc)
        self._embed_bwd(saved.emb, dx, grad_hook, dfeats)

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states: torch.Tensor = None,
                is_final: bool = True, infer_mode: bool = False
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        if infer_mode and not self.training:
            raise NotImplementedError(_UNSUPPORTED + "; got infer_mode=True")
        return super().forward(xs_pad, ilens, prev_states)

    def forward_infer(self, *args, **kwargs):
        raise NotImplementedError(_UNSUPPORTED + "; got forward_infer")


_UNSUPPORTED = ("espnet_slurp_amd ContextualBlockTransformerEncoder supports input_layer conv2d / conv2d6, pre-LN, "
                "no concat_after, linear position-wise layers, the default positional encoding and init_average=True "
                "through forward_train; unsupported: input_layer other than conv2d / conv2d6, normalize_before=False, "
                "concat_after, positionwise_layer_type other than linear, pos_enc_class, init_average=False, "
                "infer_mode=True / forward_infer (streaming decoding), tvalid (length buckets: the block layout "
                "depends on the batch's own padded length)")
