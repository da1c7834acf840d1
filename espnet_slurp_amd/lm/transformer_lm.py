"""TransformerLM -- drop-in for espnet2/lm/transformer_lm.py:12-131 (over espnet1 transformer/encoder.py with
input_layer="linear"): perplexity / validation loss (forward, inference only), the shallow-fusion scorer
(score / batch_score) and the training step (run_forward / run_backward, driven by ESPnetLanguageModel).

Embedding(V, embed_unit) -> Linear(embed_unit, att_unit) -> torch.nn.LayerNorm (eps 1e-5) -> ReLU -> positional step
(identity for pos_enc None; x*sqrt(att_unit) + pe for "sinusoidal") -> `layer` pre-LN blocks [x += MHA(LN x) causal;
x += FFN_relu(LN x)] (eps 1e-12) -> after_norm -> Linear(att_unit, V).  Same state_dict keys and shapes as the
reference (encoder.embed.{0,1}, encoder.encoders.N.*, encoder.after_norm, decoder).

Key mask: the reference's _target_mask hides, in every layer and on top of causality, each key position whose token
id is 0.  forward() takes zeros as trailing padding only (the data path: a key length per row) and raises on an
interior zero; the one-step scorer honours the mask itself (beam-search prefixes may contain token 0), through
esp_decode_attn_masked.

The scorer computes only the newest position of every prefix over a DecoderCache of per-layer K | V (the decoder's
cache class and its two state forms: a DecoderCache whose rows are ys' rows, or the reference's list form of
RowState / None).  With kernels.LM_STEP_FUSED and at most kernels.LM_STEP_MAX_ROWS rows a layer step is 5 launches
on esp_step_linear (LN + qkv + cache write; masked attention; out-proj + residual; LN + w_1 + ReLU; w_2 + residual);
otherwise the same step runs on the generic kernels (kernels.lm_step_linear: LayerNorm, linear_fwd, a cache write).

Training (run_forward / run_backward, explicit like the encoders): embedding gather -> embed.0 -> the input layer's
tail in training form (esp_lm_front_fwd: LayerNorm -> Dropout -> ReLU -> positional step) -> the layers -> after_norm
-> decoder; every parameter gradient lands in flat.grad.  The layers' _attn_fwd / _attn_bwd are overridden here
(_lm_attn_fwd / _lm_attn_bwd): their self-attention core runs on esp_causal_attn_fwd / _bwd (one launch each way, no
score tensor) when kernels.LM_ATTN_FUSED and kernels.causal_attn_ok(L, d_k) hold, else on MultiHeadedAttention's
generic kernels.  Dropout sites and rates are the
reference's: the input layer's Dropout, each layer's two residual dropouts and the FFN's inner dropout at
dropout_rate; PositionalEncoding's own dropout ("sinusoidal" only) at the espnet1 Encoder's default
positional_dropout_rate 0.1, which the reference's TransformerLM does not override; no attention dropout (0.0).
"""
from __future__ import annotations

import math
import types
from typing import Any, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .. import kernels as K
from ..asr.decoder.transformer_decoder import DecoderCache, RowState, merge_row_states
from ..asr.encoder.abs_encoder import pos_table
from ..asr.encoder.transformer_encoder import TransformerEncoderLayer
from ..blocks import Ctx, LayerNorm, Linear, MultiHeadedAttention, PositionwiseFeedForward, Seeds, empty, grad_buf
from ..flat import FlatParams


class AbsLM(nn.Module):
    """espnet2/lm/abs_model.py:9-30."""

    def forward(self, input: torch.Tensor, hidden):
        raise NotImplementedError


def _ln(norm: LayerNorm):
    return norm.weight, norm.bias, norm.eps


# espnet1 Encoder.__init__'s default, handed to pos_enc_class: the reference's TransformerLM passes dropout_rate only
POSITIONAL_DROPOUT_RATE = 0.1


def _lm_attn_fwd(self, h, resid, klen, B, T, seeds, training):
    """TransformerEncoderLayer._attn_fwd of the LM's layers (bound to each layer by _Encoder): the self-attention
    core (scores, mask, softmax, P.V) on the fused esp_causal_attn_fwd for the shapes it serves; the projections and
    the residual dropout stay the GEMMs MultiHeadedAttention uses.  The dropout seeds are drawn as the generic path
    draws them, so both paths see the same masks."""
    sa = self.self_attn
    H, dk = sa.h, sa.d_k
    if not (K.LM_ATTN_FUSED and K.causal_attn_ok(T, dk)):
        return TransformerEncoderLayer._attn_fwd(self, h, resid, klen, B, T, seeds, training)
    D = H * dk
    w, b = sa._w(("linear_q", "linear_k", "linear_v"))
    qkv = empty(B * T, 3 * D, like=h)
    K.linear_fwd(h, w, b, qkv)
    ctx = empty(B * T, D, like=h)
    lse = empty(B * H * T, like=h)
    K.causal_attn_fwd(qkv, klen, ctx, lse, B, T, H, dk)
    seeds.next()  # the generic path's attention-dropout seed (the LM's rate is 0.0)
    out = empty(B * T, D, like=h)
    pr = self.p if training else 0.0
    so = seeds.next()
    sa.linear_out.fwd(ctx, out, drop_p=pr, seed=so, R=resid, beta=1.0)
    return out, Ctx(fused=True, xq=h, qkv=qkv, ctx=ctx, lse=lse, klen=klen, pr=pr, so=so, B=B, T=T)


def _lm_attn_bwd(self, c, d):
    """The adjoint of _lm_attn_fwd (the generic path's own when the forward took it)."""
    if not c.get("fused"):
        return TransformerEncoderLayer._attn_bwd(self, c, d)
    sa = self.self_attn
    H, dk = sa.h, sa.d_k
    D = H * dk
    dz = grad_buf(d)
    K.scale_dropout(d, dz, drop_p=c.pr, seed=c.so)
    dctx = sa.linear_out.bwd(dz, c.ctx)
    dqkv = empty(c.B * c.T, 3 * D, like=d)
    K.causal_attn_bwd(c.qkv, c.klen, dctx, c.lse, dqkv, c.B, c.T, H, dk)
    names = ("linear_q", "linear_k", "linear_v")
    w, _ = sa._w(names)
    gw, gb = sa._w(names, grad=True)
    K.linear_bwd_weight(dqkv, c.xq, gw, gb)
    dx = empty(c.B * c.T, D, like=d)
    K.linear_bwd_data(dqkv, w, dx)
    return dx


class _Encoder(nn.Module):
    """Parameter layout of the espnet1 Encoder with input_layer="linear" (embed.0 Linear, embed.1 torch LayerNorm;
    embed.2-4 -- Dropout, ReLU, the positional class -- hold no parameters)."""

    def __init__(self, idim, att_unit, head, unit, layer, dropout_rate):
        super().__init__()
        self.embed = nn.Sequential(Linear(idim, att_unit), LayerNorm(att_unit, eps=1e-5))
        self.encoders = nn.ModuleList([
            TransformerEncoderLayer(att_unit, MultiHeadedAttention(head, att_unit, 0.0),
                                    PositionwiseFeedForward(att_unit, unit, dropout_rate, K.ACT_RELU), dropout_rate,
                                    causal=True)
            for _ in range(layer)])
        for l in self.encoders:  # the LM's attention core, local to the LM: the layer class stays the encoders' own
            l._attn_fwd = types.MethodType(_lm_attn_fwd, l)
            l._attn_bwd = types.MethodType(_lm_attn_bwd, l)
        self.after_norm = LayerNorm(att_unit)


class TransformerLM(AbsLM):
    def __init__(self, vocab_size: int, pos_enc: Optional[str] = None, embed_unit: int = 128, att_unit: int = 256,
                 head: int = 2, unit: int = 1024, layer: int = 4, dropout_rate: float = 0.5):
        super().__init__()
        if pos_enc not in (None, "sinusoidal"):
            raise ValueError(f"unknown pos-enc option: {pos_enc}")
        self.pos_enc = pos_enc
        self.embed = nn.Embedding(vocab_size, embed_unit)
        self.encoder = _Encoder(embed_unit, att_unit, head, unit, layer, dropout_rate)
        self.decoder = Linear(att_unit, vocab_size)
        self.vocab_size, self.embed_unit, self.D, self.h = vocab_size, embed_unit, att_unit, head
        self.dropout_rate = dropout_rate
        self.positional_dropout_rate = POSITIONAL_DROPOUT_RATE  # PositionalEncoding's own dropout ("sinusoidal")
        self.flat: Optional[FlatParams] = None
        self._zero_pe = None

    # ------------------------------------------------------------------ setup
    def flatten(self, device=None) -> FlatParams:
        """Move the parameters into one flat device buffer (the fused q|k|v weight views need it).  Call once,
        after .to(device); the scorer and forward() do it on first use otherwise."""
        device = device or next(self.parameters()).device
        self.flat = FlatParams(self, device)
        for l in self.encoder.encoders:
            l.self_attn.flat = self.flat
        return self.flat

    def _ready(self):
        if self.flat is None:
            self.flatten()
        return self.embed.weight.device

    def _gather(self, tok: torch.Tensor) -> torch.Tensor:
        """Embedding rows of tok (n,) int64 on the device -> (n, embed_unit)."""
        E = self.embed.weight
        if self._zero_pe is None or self._zero_pe.device != E.device:
            self._zero_pe = torch.zeros(1, self.embed_unit, dtype=torch.float32, device=E.device)
        e = torch.empty(tok.numel(), self.embed_unit, dtype=torch.float32, device=E.device)
        K.embed_fwd(tok, E, self._zero_pe, e, 1, 1.0, 0.0, 0)
        return e

    def _pe(self, n: int, dev):
        return pos_table("abs", n, self.D, dev) if self.pos_enc == "sinusoidal" else None

    # ------------------------------------------------------------------ full sequences
    def forward(self, input: torch.Tensor, hidden=None) -> Tuple[torch.Tensor, None]:
        """input (B, L) token ids -> (logits (B, L, V), None), without gradients.  A row's zeros must be trailing
        padding (they shorten its key length, as the reference's mask does); a zero followed by a non-zero token
        raises ValueError."""
        dev = self._ready()
        ids = input.detach().to("cpu", torch.int64)
        B, L = ids.shape
        nz = ids != 0
        lens = nz.sum(1)
        if not bool((nz == (torch.arange(L)[None, :] < lens[:, None])).all()) or int(lens.min()) < 1:
            raise ValueError("TransformerLM.forward: token 0 is padding and may only trail a row (the reference masks "
                             "every key whose id is 0; use score / batch_score for prefixes that contain it)")
        with torch.no_grad():
            tok = K.h2d(ids.reshape(-1).contiguous(), dev)
            klen = K.h2d(lens.to(torch.int32), dev)
            emb = self.encoder.embed
            lin = emb[0].fwd(self._gather(tok))
            x = K.step_ln_act(lin, emb[1].weight, emb[1].bias, emb[1].eps, torch.empty_like(lin), pe=self._pe(L, dev),
                              xscale=math.sqrt(self.D), L=L)
            seeds = Seeds(0)
            for layer in self.encoder.encoders:
                x, _ = layer.fwd(x, klen, B, L, seeds, False)
            y, _ = self.encoder.after_norm.fwd(x)
            logits = self.decoder.fwd(y)
        return logits.view(B, L, -1), None

    # ------------------------------------------------------------------ training step
    def run_forward(self, tok: torch.Tensor, klen: torch.Tensor, B: int, L: int, seeds: Seeds, training: bool):
        """tok (B*L,) int64 and klen (B,) int32 on the device -> (logits (B*L, V), saved).  Device work only: no
        host synchronisation, no host copy (a captured graph replays it).  Rows at or beyond klen[b] are padding:
        no key reads them and the caller's loss gradient is zero there."""
        dev = self._ready()
        emb = self.encoder.embed
        e = self._gather(tok)
        lin = emb[0].fwd(e)
        p1 = self.dropout_rate if training else 0.0
        p2 = self.positional_dropout_rate if training else 0.0
        s1, s2 = seeds.next(), seeds.next()
        pe = self._pe(L, dev)
        x, mean, rstd = torch.empty_like(lin), empty(B * L, like=lin), empty(B * L, like=lin)
        K.lm_front_fwd(lin, emb[1].weight, emb[1].bias, emb[1].eps, x, mean, rstd, pe=pe, xscale=math.sqrt(self.D),
                       L=L, p1=p1, seed1=s1, p2=p2, seed2=s2)
        ctxs = []
        for layer in self.encoder.encoders:
            x, c = layer.fwd(x, klen, B, L, seeds, training)
            ctxs.append(c)
        y, c_an = self.encoder.after_norm.fwd(x)
        logits = self.decoder.fwd(y)
        return logits, Ctx(tok=tok, e=e, lin=lin, mean=mean, rstd=rstd, p1=p1, p2=p2, s1=s1, s2=s2,
                           has_pe=pe is not None, layers=ctxs, an=c_an, y=y)

    def run_backward(self, saved: Ctx, dlogits: torch.Tensor) -> None:
        """The adjoint of run_forward for dlogits (B*L, V): every parameter gradient is accumulated into
        flat.grad."""
        enc = self.encoder
        dy = self.decoder.bwd(dlogits, saved.y)
        d = enc.after_norm.bwd_new(saved.an, dy)
        for layer, c in zip(reversed(enc.encoders), reversed(saved.layers)):
            d = layer.bwd(c, d)
        ln = enc.embed[1]
        dlin = torch.empty_like(d)
        K.lm_front_bwd(d, saved.lin, ln.weight, ln.bias, saved.mean, saved.rstd, dlin, ln.weight.grad, ln.bias.grad,
                       has_pe=saved.has_pe, xscale=math.sqrt(self.D), p1=saved.p1, seed1=saved.s1, p2=saved.p2,
                       seed2=saved.s2)
        de = enc.embed[0].bwd(dlin, saved.e)
        K.embed_bwd(saved.tok, de, self.embed.weight.grad, 1.0, 0.0, 0)

    # ------------------------------------------------------------------ one-step scorer
    def _eval_only(self, what: str):
        if self.training:
            raise RuntimeError(f"TransformerLM.{what}: the scorer is inference only (call .eval())")

    def init_cache(self, rows: int = 1, capacity: int = 32) -> DecoderCache:
        """An empty K | V cache for `rows` prefixes with room for `capacity` positions."""
        return DecoderCache(len(self.encoder.encoders), self.D, self.embed.weight.device, rows=rows, capacity=capacity)

    def _step(self, tok: torch.Tensor, mask: torch.Tensor, cache: DecoderCache, want_logp: bool = True
              ) -> Optional[torch.Tensor]:
        """Position cache.len of every row: tok (N,) int64 device, the row's token there; mask (N, cache.len + 1)
        uint8 device, 1 where the row's token is not 0."""
        N, D, pos = tok.shape[0], self.D, cache.len
        H, dk = self.h, self.D // self.h
        dev = tok.device
        cache.ensure(N, pos + 1)
        R, C = cache.row_capacity, cache.capacity
        enc = self.encoder
        lin_w, ln_in = enc.embed[0], enc.embed[1]
        lin = K.lm_step_linear(self._gather(tok), lin_w.weight, lin_w.bias)
        pe = self._pe(max(512, 1 << pos.bit_length()), dev)
        x = K.step_ln_act(lin, ln_in.weight, ln_in.bias, ln_in.eps, torch.empty_like(lin), pe=pe, xscale=math.sqrt(D),
                          L=1, pos0=pos)
        idx = K.DecodeIndex(np.arange(N), pos + 1, dev)
        ctx = empty(N, D, like=x)
        for l, layer in enumerate(enc.encoders):
            sa, ff = layer.self_attn, layer.feed_forward
            w, b = sa._w(("linear_q", "linear_k", "linear_v"))
            cb = cache.buf[l]
            q = K.lm_step_linear(x, w, b, ln=_ln(layer.norm1), c0=D, cache=cb, pos=pos)  # K | V -> cb[:, pos]
            K.decode_attn_masked(q, q.stride(0), 0, cb, 2 * D, C * 2 * D, 0, cb, 2 * D, C * 2 * D, D, ctx, D, 0, idx,
                                 mask, H, dk, R, C)
            x = K.lm_step_linear(ctx, sa.linear_out.weight, sa.linear_out.bias, R=x)
            hdn = K.lm_step_linear(x, ff.w_1.weight, ff.w_1.bias, ln=_ln(layer.norm2), relu=True)
            x = K.lm_step_linear(hdn, ff.w_2.weight, ff.w_2.bias, R=x)
        cache.len = pos + 1
        if not want_logp:
            return None
        logits = K.lm_step_linear(x, self.decoder.weight, self.decoder.bias, ln=_ln(enc.after_norm))
        logp = torch.empty_like(logits)
        K.log_softmax(logits, logp, N, logits.shape[1])
        return logp

    def forward_one_step(self, ys: torch.Tensor, cache: Optional[DecoderCache] = None
                         ) -> Tuple[torch.Tensor, DecoderCache]:
        """ys (N, L) prefixes -> (log p(. | prefix) (N, V), cache); only position L-1 is computed.  cache: what an
        earlier step returned, its rows already in ys' order; None (or an empty cache) computes the earlier
        positions one by one first."""
        self._eval_only("forward_one_step")
        dev = self._ready()
        N, L = ys.shape
        with torch.no_grad():
            if cache is None:
                cache = self.init_cache(N)
            if cache.len == 0:
                cache.n = N
            if cache.n != N or cache.len > L - 1:
                raise ValueError(f"forward_one_step: cache of {cache.n} rows x {cache.len} positions for ys {N} x {L}")
            ys = K.h2d(ys.to(torch.int64), dev).contiguous()
            mask = (ys != 0).to(torch.uint8)
            while cache.len < L - 1:
                p = cache.len
                self._step(ys[:, p].contiguous(), mask[:, :p + 1], cache, want_logp=False)
            return self._step(ys[:, L - 1].contiguous(), mask, cache), cache

    def score(self, y: torch.Tensor, state: Optional[DecoderCache], x=None) -> Tuple[torch.Tensor, DecoderCache]:
        """y (L,) prefix, state (None at first), x ignored -> (logp (V,), state)."""
        logp, state = self.forward_one_step(y.unsqueeze(0), state)
        return logp[0], state

    def batch_score(self, ys: torch.Tensor, states, xs=None) -> Tuple[torch.Tensor, Any]:
        """ys (N, L), states, xs ignored -> (logp (N, V), states).  states as TransformerDecoder.batch_score takes
        them: a DecoderCache whose rows are ys' rows (or None at the first step), returned as a DecoderCache; or
        the reference's list form (None entries at first, then RowState), returned as a list."""
        self._eval_only("batch_score")
        if states is None or isinstance(states, DecoderCache):
            return self.forward_one_step(ys, states)
        cache = merge_row_states(states, ys.shape[0], self.init_cache)
        logp, cache = self.forward_one_step(ys, cache)
        return logp, [RowState(cache, i) for i in range(ys.shape[0])]
