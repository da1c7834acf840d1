"""AbsEncoder (espnet2/asr/encoder/abs_encoder.py:7-19) and shared encoder plumbing."""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from typing import Dict, Optional, Tuple

import torch

from ... import kernels as K
from ...blocks import Ctx, MultiHeadedAttention, RelPositionMultiHeadedAttention, Seeds


class AbsEncoder(torch.nn.Module, ABC):
    @abstractmethod
    def output_size(self) -> int:
        raise NotImplementedError

    @abstractmethod
    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states: torch.Tensor = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        raise NotImplementedError


class TooShortUttError(Exception):
    """subsampling.py:14-29."""

    def __init__(self, message, actual_size, limit):
        super().__init__(message)
        self.actual_size = actual_size
        self.limit = limit


# second-stage (cut, stride) of the mask slicing per input_layer: conv2d `[:, :, :-2:2]` (subsampling.py:87),
# conv2d6 `[:, :, :-4:3]` (subsampling.py:146); the first stage is `[:, :, :-2:2]` for both
_MASK_STAGE2 = {"conv2d": (2, 2), "conv2d6": (4, 3)}


def subsampled_lengths(ilens_cpu: torch.Tensor, T: int, input_layer: str = "conv2d") -> torch.Tensor:
    """Valid-frame counts of `mask[:, :, :-2:2][:, :, :-c:s]` (subsampling.py:87 / :146): frame i
    survives the first stage iff i even, i < T-2, i < len; the second iff j % s == 0, j < T1 - c,
    j < len1.  Not the conv output-size formula."""
    cut, st = _MASK_STAGE2[input_layer]
    lens = ilens_cpu.long().clamp(max=T)
    T1 = len(range(0, T - 2, 2))
    l1 = torch.clamp((lens + 1) // 2, max=T1)
    l2 = torch.clamp((l1 + st - 1) // st, max=len(range(0, T1 - cut, st)))
    return l2


# ------------------------------------------------------------------ positional tables
_PE_CACHE: Dict[tuple, torch.Tensor] = {}


def _pe_rows(positions: torch.Tensor, d: int) -> torch.Tensor:
    """sin/cos rows computed exactly as embedding.py:66-80 (fp32, CPU)."""
    pe = torch.zeros(positions.numel(), d)
    position = positions.to(torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def pos_table(kind: str, T: int, d: int, device, max_len: int = 5000) -> torch.Tensor:
    """Constant positional tables, host-built once per (kind, T, d) and kept resident in HBM.

    abs    : PositionalEncoding pe[:T]                         (embedding.py:35-94)
    latest : RelPositionalEncoding, rows k = PE(T-1-k), 2T-1    (embedding.py:173-244)
    legacy : LegacyRelPositionalEncoding, rows k = PE(max-1-k)  (embedding.py:133-170)
    """
    key = (kind, T, d, str(device), max_len)
    t = _PE_CACHE.get(key)
    if t is not None:
        return t
    n = max(max_len, T)
    if kind == "abs":
        tab = _pe_rows(torch.arange(0, n, dtype=torch.float32), d)[:T]
    elif kind == "legacy":
        tab = _pe_rows(torch.arange(n - 1, -1, -1.0, dtype=torch.float32), d)[:T]
    elif kind == "latest":
        position = torch.arange(0, n, dtype=torch.float32)
        pos = _pe_rows(position, d)
        neg = torch.zeros(n, d)
        div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
        neg[:, 0::2] = torch.sin(-1 * position.unsqueeze(1) * div_term)
        neg[:, 1::2] = torch.cos(-1 * position.unsqueeze(1) * div_term)
        full = torch.cat([torch.flip(pos, [0]), neg[1:]], dim=0)
        c = full.size(0) // 2
        tab = full[c - T + 1: c + T]
    else:
        raise ValueError(kind)
    t = tab.contiguous().to(device)
    _PE_CACHE[key] = t
    return t


def draw_seed() -> int:
    """64-bit dropout key from torch's CPU generator (reproducible under torch.manual_seed)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def lengths_to_device(lens: torch.Tensor, device) -> torch.Tensor:
    return K.h2d(lens.to(torch.int32), device)


class EncoderFn(torch.autograd.Function):
    """Runs an encoder's explicit forward; its backward writes parameter gradients into the
    flat gradient buffer (flat.py) and returns no input gradient (fbank needs none)."""

    @staticmethod
    def forward(ctx, feats, anchor, enc, ilens_cpu, seed, grad_hook, klen=None, tvalid=None, inter=None):
        hs, olens, saved = enc.run_forward(feats, ilens_cpu, Seeds(seed), enc.training, klen=klen, tvalid=tvalid,
                                           inter=inter)
        ctx.enc = enc
        ctx.saved = saved
        ctx.grad_hook = grad_hook
        ctx.olens = olens
        return hs

    @staticmethod
    def backward(ctx, dhs):
        ctx.enc.run_backward(ctx.saved, dhs.contiguous(), ctx.grad_hook)
        ctx.saved = None
        return None, None, None, None, None, None, None, None, None


class StackedEncoder(AbsEncoder):
    """embed (Conv2dSubsampling) -> a positional step -> encoders (a ModuleList of layers with fwd / bwd) ->
    after_norm, with an explicit backward (EncoderFn).  A subclass's constructor registers embed, encoders and
    after_norm, in that order (rel-pos encoders also set legacy and max_pos_emb_len); its
    run_forward(feats, ilens_cpu, seeds, training, klen=None, tvalid=None, inter=None) -> (hs (B, T', D), olens,
    saved) is written from the helpers below, and so is run_backward where the plain one does not fit."""

    def __init__(self, output_size: int, positional_dropout_rate: float):
        super().__init__()
        self._output_size = output_size
        self.positional_dropout_rate = positional_dropout_rate
        self.flat = None

    def output_size(self) -> int:
        return self._output_size

    def output_lengths(self, ilens_cpu: torch.Tensor, T: int) -> torch.Tensor:
        """Valid output frames per utterance (host, no device round trip)."""
        return subsampled_lengths(ilens_cpu, T, self.embed.input_layer)

    def attach_flat(self, flat):
        self.flat = flat
        for m in self.encoders.modules():
            if isinstance(m, (MultiHeadedAttention, RelPositionMultiHeadedAttention)):
                m.flat = flat

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states: torch.Tensor = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        assert self.flat is not None, "call espnet_slurp_amd.flatten_model(model) before running"
        ilens_cpu = ilens.detach().cpu()
        feats = xs_pad.contiguous().float()
        olens = self.output_lengths(ilens_cpu, feats.shape[1])
        hs = self.forward_prepared(feats, ilens_cpu, lengths_to_device(olens, feats.device), draw_seed())
        return hs, K.h2d(olens, xs_pad.device), None

    def forward_prepared(self, feats: torch.Tensor, ilens_cpu: torch.Tensor, klen: torch.Tensor, seed: int,
                         tvalid: torch.Tensor = None, inter=None):
        """Encoder output hs (B, T', D) from device-resident inputs only (klen: int32 output
        lengths on device): no host->device traffic, so it can be captured in a HIP graph.
        tvalid, inter: as run_forward takes them (length buckets; the model's intermediate-CTC request)."""
        anchor = self.after_norm.weight
        hook = getattr(self, "_grad_hook", None)
        if torch.is_grad_enabled() and anchor.requires_grad:
            return EncoderFn.apply(feats, anchor, self, ilens_cpu, seed, hook, klen, tvalid, inter)
        return self.run_forward(feats, ilens_cpu, Seeds(seed), self.training, klen=klen, tvalid=tvalid,
                                inter=inter)[0]

    # ---------------------------------------------------------------- the pieces of run_forward / run_backward
    def _begin(self, feats, ilens_cpu):
        """check_short_utt (subsampling.py:31-39) -> (B, olens)."""
        B, T, _ = feats.shape
        lim = self.embed.min_frames
        if T < lim:
            raise TooShortUttError(
                f"has {T} frames and is too short for subsampling (it needs more than {lim} frames), return empty results",
                T, lim)
        return B, self.output_lengths(ilens_cpu, T)

    @staticmethod
    def _klen(klen, olens, device):
        """The key lengths on the device: the caller's, or olens uploaded."""
        return lengths_to_device(olens, device) if klen is None else klen

    def _embed_rel(self, feats, seeds: Seeds, training: bool):
        """Rel-pos step (embedding.py:133-244): x*sqrt(D) with dropout in the embed's epilogue, and the table
        with a dropout of its own -> (x (B*T', D), pos, c_emb).  The table is a constant: no adjoint."""
        D = self._output_size
        x, c_emb = self.embed.fwd(feats, math.sqrt(D), self.positional_dropout_rate, seeds, training)
        pos = pos_table("legacy" if self.legacy else "latest", c_emb.T2, D, feats.device, self.max_pos_emb_len)
        pp = self.positional_dropout_rate if training else 0.0
        sp = seeds.next()
        if pp > 0:
            tab, pos = pos, torch.empty_like(pos)
            K.scale_dropout(tab, pos, drop_p=pp, seed=sp)
        return x, pos, c_emb

    def _embed_abs(self, feats, seeds: Seeds, training: bool):
        """Abs-pos step (embedding.py:81-94): x*sqrt(D) from the embed's epilogue, + pe per utterance by a
        residual-add pass, then dropout over the whole tensor -> (x (B*T', D), c_emb); c_emb.pos_drop keeps the
        mask's (rate, seed) for _embed_bwd."""
        D = self._output_size
        x, c_emb = self.embed.fwd(feats, math.sqrt(D), 0.0, seeds, training)
        B, T2 = feats.shape[0], c_emb.T2
        pe = pos_table("abs", T2, D, feats.device)
        pp, sp = c_emb.pos_drop = (self.positional_dropout_rate if training else 0.0, seeds.next())
        x3 = x.view(B, T2, D)
        y = torch.empty_like(x)
        for b in range(B):
            K.scale_dropout(pe, y[b * T2:(b + 1) * T2], alpha=1.0, drop_p=0.0, seed=0, r=x3[b], beta=1.0)
        if pp > 0:
            K.scale_dropout(y, y, drop_p=pp, seed=sp)
        return y, c_emb

    def _embed_bwd(self, c_emb, d, grad_hook=None, dfeats=None):
        """The adjoint of either positional step and of embed, then embed's module-done hook."""
        pp, sp = c_emb.get("pos_drop", (0.0, 0))  # set by _embed_abs alone
        if pp > 0:
            K.scale_dropout(d, d, drop_p=pp, seed=sp)
        self.embed.bwd(c_emb, d, dfeats=dfeats)
        if grad_hook is not None:
            grad_hook(self.embed)

    def _layers_fwd(self, x, *args, **kw):
        """x through every layer.fwd(x, *args, **kw) -> (x, the layers' contexts)."""
        ctxs = []
        for layer in self.encoders:
            x, c = layer.fwd(x, *args, **kw)
            ctxs.append(c)
        return x, ctxs

    def _finish(self, x, B: int, olens, **saved):
        """after_norm -> run_forward's (hs, olens, saved)."""
        hs, c_after = self.after_norm.fwd(x)
        return hs.view(B, -1, self._output_size), olens, Ctx(after=c_after, **saved)

    def _layers_bwd(self, saved, dhs, grad_hook=None):
        """after_norm and the layers, last first, each context released and each module hooked when done
        -> the gradient at the first layer's input."""
        d = self.after_norm.bwd_new(saved.after, dhs.view(-1, self._output_size))
        if grad_hook is not None:
            grad_hook(self.after_norm)
        for i in range(len(self.encoders) - 1, -1, -1):
            d = self.encoders[i].bwd(saved.layers[i], d)
            saved.layers[i] = None
            if grad_hook is not None:
                grad_hook(self.encoders[i])
        return d

    def run_backward(self, saved, dhs, grad_hook=None):
        self._embed_bwd(saved.emb, self._layers_bwd(saved, dhs, grad_hook), grad_hook)
