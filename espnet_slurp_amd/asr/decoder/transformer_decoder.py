"""TransformerDecoder — drop-in for espnet2/asr/decoder/transformer_decoder.py:28-145,232-280.

Embedding(V,D) -> x*sqrt(D)+PE (dropout) -> num_blocks x [LN -> causal self-MHA -> +res;
LN -> source MHA over the encoder output -> +res; LN -> FFN(ReLU) -> +res]
(transformer/decoder_layer.py:63-134) -> after_norm -> Linear(D, V).
Masks: tgt (j < ys_in_len_b and j <= i), memory (j < hlen_b) — applied inside the softmax
kernel, nothing materialised.  Explicit backward; the memory gradient of every layer is
accumulated into one dhs buffer.

Inference also has the reference's incremental interface (transformer_decoder.py:147-229):
prepare_memory / forward_one_step / score / batch_score compute only the newest position of every
decode row, over a preallocated self-attention K/V cache (DecoderCache) and the memory K/V projected
once per utterance (PreparedMemory), with the single-query attention kernel esp_decode_attn.
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import nn

from ... import kernels as K
from ...blocks import Ctx, LayerNorm, Linear, MultiHeadedAttention, PositionwiseFeedForward, Seeds, empty
from ..encoder.abs_encoder import pos_table


class AbsDecoder(nn.Module):
    """espnet2/asr/decoder/abs_decoder.py:9-18."""

    def forward(self, hs_pad, hlens, ys_in_pad, ys_in_lens):
        raise NotImplementedError


class DecoderLayer(nn.Module):
    def __init__(self, size, self_attn, src_attn, feed_forward, dropout_rate):
        super().__init__()
        self.size = size
        self.self_attn = self_attn
        self.src_attn = src_attn
        self.feed_forward = feed_forward
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)
        self.norm3 = LayerNorm(size)
        self.p = dropout_rate
        self.causal = True  # self-attention mask j <= i; False (MLMDecoder): every valid key

    def fwd(self, x, mem, B, L, Tm, tgt_klen, mem_klen, seeds, training):
        c = Ctx()
        h, c.ln1 = self.norm1.fwd(x, gemm_only=True)
        x, c.sa = self.self_attn.fwd(h, x, B, L, tgt_klen, self.causal, self.p, seeds, training)
        h, c.ln2 = self.norm2.fwd(x, gemm_only=True)
        x, c.src = self.src_attn.fwd(h, x, B, L, mem_klen, False, self.p, seeds, training, mem=mem, Tk=Tm)
        h, c.ln3 = self.norm3.fwd(x, gemm_only=True)
        x, c.ff = self.feed_forward.fwd(h, x, 1.0, self.p, seeds, training)
        return x, c

    def bwd(self, c, d, dmem):
        self.norm3.bwd(c.ln3, self.feed_forward.bwd(c.ff, d), d)
        self.norm2.bwd(c.ln2, self.src_attn.bwd(c.src, d, dmem), d)
        self.norm1.bwd(c.ln1, self.self_attn.bwd(c.sa, d), d)
        return d


class PreparedMemory:
    """The encoder memory of U utterances as every decoder layer's source attention reads it: kv
    (num_blocks, U*T, 2D) fp32, layer l's linear_k | linear_v projection of the (U, T, D) memory, computed once
    (TransformerDecoder.prepare_memory).  hlens: the utterances' encoder lengths (host int32)."""

    def __init__(self, kv: torch.Tensor, hlens: np.ndarray, U: int, T: int):
        self.kv, self.hlens, self.U, self.T = kv, hlens, U, T
        self._index = (None, None)

    def index(self, rows: np.ndarray) -> "K.DecodeIndex":
        """The (src, klen) launch index of decode rows reading utterances `rows` (kept while rows repeat)."""
        key = rows.tobytes()
        if self._index[0] != key:
            if rows.size and (rows.min() < 0 or rows.max() >= self.U):
                raise ValueError(f"PreparedMemory: row -> utterance index outside [0, {self.U})")
            self._index = (key, K.DecodeIndex(rows, self.hlens[rows], self.kv.device))
        return self._index[1]

    def set_window(self, T: int):
        """Source attention reads only the first T frames of every utterance from now on (the block-synchronous
        search's window; kv itself covers all frames, a frame's projection does not depend on the window).  Drops
        the cached launch index, which holds the lengths."""
        if not 1 <= T <= self.T:
            raise ValueError(f"PreparedMemory.set_window: {T} frames outside [1, {self.T}]")
        self.hlens = np.full(self.U, T, dtype=np.int32)
        self._index = (None, None)


class DecoderCache:
    """Self-attention cache of the one-step decoder: buf (num_blocks, rows, positions, 2D) fp32 holds, for every
    layer, each decode row's prefix keys (columns [0, D)) and values ([D, 2D)) -- not the layer outputs the
    reference caches; the state is opaque to a search, which only passes it back and reorders it.  Preallocated;
    rows and positions grow by doubling; reorder(index) keeps row index[i] as row i (the parent selection
    after pruning; an index may repeat and may be longer than the current row count).

    reorder_keep(index) is reorder for a search that may take one step back: the rows are gathered into a second
    buffer (esp_cache_gather, one launch for all layers) and the two buffers swap roles, so the rows of before the
    selection survive until the next reorder_keep; rollback() goes back to them, one position shorter."""

    def __init__(self, num_blocks: int, D: int, device, rows: int = 1, capacity: int = 32):
        self.buf = torch.empty(num_blocks, max(1, rows), max(1, capacity), 2 * D, dtype=torch.float32, device=device)
        self.n = rows   # decode rows in use
        self.len = 0    # positions stored per row
        self.alt = None   # reorder_keep's second buffer: the rows of before the last reorder_keep
        self.hist = None  # (n, len) of those rows; None: nothing to go back to

    @property
    def row_capacity(self) -> int:
        return self.buf.shape[1]

    @property
    def capacity(self) -> int:
        return self.buf.shape[2]

    def ensure(self, rows: int, length: int):
        nl, R, C, W = self.buf.shape
        if rows <= R and length <= C:
            return
        while R < rows:
            R *= 2
        while C < length:
            C *= 2
        new = torch.empty(nl, R, C, W, dtype=torch.float32, device=self.buf.device)
        if self.n and self.len:
            new[:, :self.n, :self.len] = self.buf[:, :self.n, :self.len]
        self.buf = new

    def _index(self, index) -> torch.Tensor:
        if not torch.is_tensor(index):
            index = K.h2d(torch.as_tensor(np.asarray(index, dtype=np.int64)), self.buf.device)
        return index.to(device=self.buf.device, dtype=torch.int64)

    def reorder(self, index) -> "DecoderCache":
        index = self._index(index)
        n = int(index.numel())
        g = self.buf[:, index, :self.len] if self.len else None  # gathered before the rows are overwritten
        self.ensure(n, self.len)
        if g is not None:
            self.buf[:, :n, :self.len] = g
        self.n = n
        return self

    def reorder_keep(self, index) -> "DecoderCache":
        """reorder(index), keeping the rows of before it for one rollback().  Growing this cache afterwards
        (ensure) allocates a new live buffer and leaves the kept one alone."""
        index = self._index(index).contiguous()
        n = int(index.numel())
        nl, R, C, W = self.buf.shape
        if self.alt is None or self.alt.shape[1] < n or self.alt.shape[2] < C:
            while R < n:
                R *= 2
            self.alt = torch.empty(nl, R, C, W, dtype=torch.float32, device=self.buf.device)
        if n and self.len:
            K.cache_gather(self.buf, self.alt, index, n, self.len, self.n)
        self.buf, self.alt = self.alt, self.buf
        self.hist, self.n = (self.n, self.len), n
        return self

    def rollback(self) -> "DecoderCache":
        """Back to the rows of before the last reorder_keep, without their newest position: the buffer and the row
        count of then, len one less (the step that wrote that position is taken again)."""
        if self.hist is None:
            raise RuntimeError("DecoderCache.rollback: no reorder_keep to go back from (one step of history is kept)")
        self.buf, self.alt = self.alt, self.buf
        self.n, self.len = self.hist[0], self.hist[1] - 1
        self.hist = None
        return self

    def select(self, index) -> "DecoderCache":
        """A new cache holding rows `index` of this one (this one is left as it is)."""
        index = self._index(index)
        nl, _, C, W = self.buf.shape
        out = DecoderCache(nl, W // 2, self.buf.device, rows=int(index.numel()), capacity=C)
        if self.len:
            out.buf[:, :, :self.len] = self.buf[:, index, :self.len]
        out.len = self.len
        return out


class RowState(NamedTuple):
    """One hypothesis' decoder state in the list form of batch_score: row `row` of `cache`."""
    cache: DecoderCache
    row: int


def merge_row_states(states, n: int, init_cache) -> Optional[DecoderCache]:
    """The list form of batch_score's states -> one cache whose rows are the list's entries: None when every entry
    is None (the first step), else the RowState rows gathered into a new cache (one gather per distinct source
    cache, no loop over hypotheses on the device).  init_cache(rows, capacity=) makes the new cache."""
    states = list(states)
    if len(states) != n:
        raise ValueError(f"batch_score: {len(states)} states for {n} prefixes")
    if all(s is None for s in states):
        return None
    if any(s is None for s in states):
        raise ValueError("batch_score: a mix of empty and non-empty states")
    first = states[0].cache
    if all(s.cache is first for s in states):
        return first.select([s.row for s in states])
    if len({s.cache.len for s in states}) != 1:
        raise ValueError("batch_score: states of different prefix lengths")
    cache = init_cache(len(states), capacity=max(s.cache.capacity for s in states))
    cache.len = first.len
    by_cache = {}
    for i, s in enumerate(states):
        by_cache.setdefault(id(s.cache), (s.cache, [], []))
        by_cache[id(s.cache)][1].append(i)
        by_cache[id(s.cache)][2].append(s.row)
    for c, dst, src in by_cache.values():
        cache.buf[:, cache._index(dst), :cache.len] = c.buf[:, c._index(src), :cache.len]
    return cache


class TransformerDecoder(AbsDecoder):
    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4,
                 linear_units: int = 2048, num_blocks: int = 6, dropout_rate: float = 0.1,
                 positional_dropout_rate: float = 0.1, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, input_layer: str = "embed",
                 use_output_layer: bool = True, pos_enc_class=None, normalize_before: bool = True,
                 concat_after: bool = False, layer_drop_rate: float = 0.0):
        super().__init__()
        if input_layer != "embed" or not use_output_layer or not normalize_before or concat_after or layer_drop_rate:
            raise NotImplementedError("espnet_slurp_amd TransformerDecoder: embed/pre-LN/output-layer form only")
        D = encoder_output_size
        self.embed = nn.Sequential(nn.Embedding(vocab_size, D))
        self.after_norm = LayerNorm(D)
        self.output_layer = Linear(D, vocab_size)
        self.decoders = nn.ModuleList([
            DecoderLayer(D, MultiHeadedAttention(attention_heads, D, self_attention_dropout_rate),
                         MultiHeadedAttention(attention_heads, D, src_attention_dropout_rate),
                         PositionwiseFeedForward(D, linear_units, dropout_rate, K.ACT_RELU), dropout_rate)
            for _ in range(num_blocks)])
        self.dropout_rate = dropout_rate
        self.positional_dropout_rate = positional_dropout_rate
        self.vocab_size = vocab_size
        self.D = D
        self.flat = None

    def attach_flat(self, flat):
        self.flat = flat
        for l in self.decoders:
            l.self_attn.flat = flat
            l.src_attn.flat = flat

    def run_forward(self, hs, hlens_i32, ys_in, ys_in_lens_i32, seeds: Seeds, training: bool):
        B, Tm, D = hs.shape
        L = ys_in.shape[1]
        mem = hs.reshape(B * Tm, D)
        pe = pos_table("abs", L, D, hs.device)
        x = empty(B * L, D, like=hs)
        pp = self.positional_dropout_rate if training else 0.0
        sp = seeds.next()
        E = self.embed[0].weight
        K.embed_fwd(ys_in, E, pe, x, L, math.sqrt(D), pp, sp)
        ctxs = []
        for layer in self.decoders:
            x, c = layer.fwd(x, mem, B, L, Tm, ys_in_lens_i32, hlens_i32, seeds, training)
            ctxs.append(c)
        y, c_after = self.after_norm.fwd(x)
        logits = self.output_layer.fwd(y)
        return logits, Ctx(ys_in=ys_in, pp=pp, sp=sp, layers=ctxs, after=c_after, y=y, B=B, L=L, Tm=Tm, mem=mem)

    def run_backward(self, saved, dlogits, dmem, grad_hook=None):
        """dlogits (B*L, V); dmem (B*Tm, D) accumulated (+=)."""
        dy = self.output_layer.bwd(dlogits, saved.y)
        d = self.after_norm.bwd_new(saved.after, dy)
        if grad_hook is not None:
            grad_hook(self.output_layer)
            grad_hook(self.after_norm)
        for i in range(len(self.decoders) - 1, -1, -1):
            d = self.decoders[i].bwd(saved.layers[i], d, dmem)
            saved.layers[i] = None
            if grad_hook is not None:
                grad_hook(self.decoders[i])
        K.embed_bwd(saved.ys_in, d, self.embed[0].weight.grad, math.sqrt(self.D), saved.pp, saved.sp)
        if grad_hook is not None:
            grad_hook(self.embed)

    def forward(self, hs_pad: torch.Tensor, hlens: torch.Tensor, ys_in_pad: torch.Tensor,
                ys_in_lens: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Inference-style forward (no parameter gradients): returns (logits, olens)."""
        from ..encoder.abs_encoder import draw_seed
        with torch.no_grad():
            logits, _ = self.run_forward(hs_pad.contiguous(), hlens.to(torch.int32).to(hs_pad.device),
                                         ys_in_pad.to(hs_pad.device), ys_in_lens.to(torch.int32).to(hs_pad.device),
                                         Seeds(draw_seed()), self.training)
        B, L = ys_in_pad.shape
        return logits.view(B, L, -1), ys_in_lens

    # ------------------------------------------------------------------ incremental inference
    def _eval_only(self, what: str):
        if self.training:
            raise RuntimeError(f"TransformerDecoder.{what}: the one-step decoder is inference only (call .eval())")

    def init_cache(self, rows: int = 1, capacity: int = 32) -> DecoderCache:
        """An empty self-attention cache for `rows` decode rows with room for `capacity` positions."""
        return DecoderCache(len(self.decoders), self.D, self.embed[0].weight.device, rows=rows, capacity=capacity)

    def prepare_memory(self, hs_pad: torch.Tensor, hlens) -> PreparedMemory:
        """hs_pad (U, T, D), hlens (U,) -> every layer's source-attention keys and values of the memory, one
        linear_k | linear_v GEMM per layer over the U*T rows.  Computed once per batch of utterances."""
        self._eval_only("prepare_memory")
        U, T, D = hs_pad.shape
        hl = np.asarray(torch.as_tensor(hlens).cpu(), dtype=np.int32).reshape(-1)
        if hl.shape[0] != U or hl.min() < 1 or hl.max() > T:
            raise ValueError(f"prepare_memory: hlens {hl.tolist()} for a memory of shape {tuple(hs_pad.shape)}")
        with torch.no_grad():
            mem = hs_pad.to(torch.float32).contiguous().view(U * T, D)
            kv = torch.empty(len(self.decoders), U * T, 2 * D, dtype=torch.float32, device=mem.device)
            for l, layer in enumerate(self.decoders):
                w, b = layer.src_attn._w(("linear_k", "linear_v"))
                K.linear_fwd(mem, w, b, kv[l])
        return PreparedMemory(kv, hl, U, T)

    def _resolve_memory(self, memory, N: int) -> Tuple[PreparedMemory, np.ndarray]:
        rows = None
        if isinstance(memory, (tuple, list)):
            memory, rows = memory
        if torch.is_tensor(memory):  # plain (N, T, D) memory: projected on the spot (correct, slow)
            if memory.dim() == 2:
                memory = memory.unsqueeze(0)
            memory = self.prepare_memory(memory, [memory.shape[1]] * memory.shape[0])
        if rows is None:
            if memory.U not in (1, N):
                raise ValueError(f"{N} decode rows over a memory of {memory.U} utterances need a row -> utterance index")
            rows = np.arange(N) if memory.U == N else np.zeros(N)
        elif torch.is_tensor(rows):
            rows = rows.cpu().numpy()
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        if rows.shape[0] != N:
            raise ValueError(f"row -> utterance index of {rows.shape[0]} entries for {N} decode rows")
        return memory, rows

    def _step(self, tok: torch.Tensor, mem: PreparedMemory, rows: np.ndarray, cache: DecoderCache,
              want_logp: bool = True) -> Optional[torch.Tensor]:
        """One position (cache.len) of every decode row: tok (N,) int64 device, the row's token there."""
        N, D, pos = tok.shape[0], self.D, cache.len
        H = self.decoders[0].self_attn.h
        dk = D // H
        dev = tok.device
        cache.ensure(N, pos + 1)
        pe = pos_table("abs", max(512, 1 << pos.bit_length()), D, dev)
        x = torch.empty(N, D, dtype=torch.float32, device=dev)
        K.embed_fwd(tok, self.embed[0].weight, pe[pos:pos + 1], x, 1, math.sqrt(D), 0.0, 0)
        self_idx = K.DecodeIndex(np.arange(N), pos + 1, dev)
        src_idx = mem.index(rows)
        seeds = Seeds(0)
        R, C = cache.row_capacity, cache.capacity
        for l, layer in enumerate(self.decoders):
            sa, ca = layer.self_attn, layer.src_attn
            h, _ = layer.norm1.fwd(x)
            w, b = sa._w(("linear_q", "linear_k", "linear_v"))
            qkv = empty(N, 3 * D, like=x)
            K.linear_fwd(h, w, b, qkv)
            cb = cache.buf[l]
            cb[:N, pos] = qkv[:, D:]
            ctx = empty(N, D, like=x)
            K.decode_attn(qkv, 3 * D, 0, cb, 2 * D, C * 2 * D, 0, cb, 2 * D, C * 2 * D, D, ctx, D, 0, self_idx, H, dk,
                          R, C)
            x = sa.linear_out.fwd(ctx, R=x, beta=1.0)
            h, _ = layer.norm2.fwd(x)
            q = ca.linear_q.fwd(h)
            kv = mem.kv[l]
            K.decode_attn(q, D, 0, kv, 2 * D, mem.T * 2 * D, 0, kv, 2 * D, mem.T * 2 * D, D, ctx, D, 0, src_idx, H, dk,
                          mem.U, mem.T)
            x = ca.linear_out.fwd(ctx, R=x, beta=1.0)
            h, _ = layer.norm3.fwd(x)
            x, _ = layer.feed_forward.fwd(h, x, 1.0, 0.0, seeds, False)
        cache.len = pos + 1
        if not want_logp:
            return None
        y, _ = self.after_norm.fwd(x)
        logits = self.output_layer.fwd(y)
        logp = torch.empty_like(logits)
        K.log_softmax(logits, logp, N, logits.shape[1])
        return logp

    def forward_one_step(self, tgt: torch.Tensor, tgt_mask, memory, cache: Optional[DecoderCache] = None
                         ) -> Tuple[torch.Tensor, DecoderCache]:
        """tgt (N, L) prefixes -> (log p(. | prefix) (N, V), cache); only position L-1 is computed.

        tgt_mask is accepted for the reference's signature and ignored: the step is causal by construction
        (position L-1 attends the L cached positions).  memory: a PreparedMemory (U = N or U = 1), a pair
        (PreparedMemory, row -> utterance index), or a plain (N, T, D) tensor, which is projected on the spot
        (correct but slow).  cache: what an earlier step returned, its rows already in tgt's order
        (DecoderCache.reorder); None (or an empty cache) computes the earlier positions one by one first."""
        self._eval_only("forward_one_step")
        N, L = tgt.shape
        with torch.no_grad():
            mem, rows = self._resolve_memory(memory, N)
            dev = mem.kv.device
            if cache is None:
                cache = self.init_cache(N)
            if cache.len == 0:
                cache.n = N
            if cache.n != N or cache.len > L - 1:
                raise ValueError(f"forward_one_step: cache of {cache.n} rows x {cache.len} positions for tgt {N} x {L}")
            tgt = K.h2d(tgt.to(torch.int64), dev)
            while cache.len < L - 1:
                self._step(tgt[:, cache.len].contiguous(), mem, rows, cache, want_logp=False)
            return self._step(tgt[:, L - 1].contiguous(), mem, rows, cache), cache

    def score(self, ys: torch.Tensor, state: Optional[DecoderCache], x) -> Tuple[torch.Tensor, DecoderCache]:
        """ys (L,), state (None at first), x (T, D) memory or a PreparedMemory of one utterance -> (logp (V,), state)."""
        logp, state = self.forward_one_step(ys.unsqueeze(0), None, x, cache=state)
        return logp[0], state

    def batch_score(self, ys: torch.Tensor, states, xs) -> Tuple[torch.Tensor, Any]:
        """ys (N, L), states, xs -> (logp (N, V), states).  states: a DecoderCache whose rows are ys' rows (or None
        at the first step) -- returned as a DecoderCache; or the reference's list form, one entry per hypothesis
        (None at first, then the RowState entries an earlier call returned, in any order and from any call) --
        returned as a list.  The list form gathers the rows into a new cache (one gather per distinct source
        cache, no loop over hypotheses on the device).  xs as forward_one_step's memory."""
        self._eval_only("batch_score")
        if states is None or isinstance(states, DecoderCache):
            return self.forward_one_step(ys, None, xs, cache=states)
        cache = merge_row_states(states, ys.shape[0], self.init_cache)
        logp, cache = self.forward_one_step(ys, None, xs, cache=cache)
        return logp, [RowState(cache, i) for i in range(ys.shape[0])]
