"""TransducerDecoder — drop-in for espnet2/asr/decoder/transducer_decoder.py:12-296 (the RNN-T predictor).

Embedding(vocab, H, padding_idx=embed_pad) -> num_layers x LSTM(H, H) -> per-layer dropout, with the reference's
state_dict keys (embed.weight, decoder.{l}.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0).  The LSTM runs over
the blank-padded decoder input without length masking, as the reference's does.  Each layer's input projection is one
GEMM for all B * U1 rows; the recurrence is one esp_lstm_cell_fwd / _bwd launch per step (csrc/lstm.hip), which adds
h_{u-1} W_hh^T inside the kernel; the weight gradients are one GEMM each after the loop (dW_hh against the shifted h).
`rnn_type: gru` is not served.

Training: run_forward / run_backward (explicit kernel sequences, gradients into the flat views).  Inference:
init_state / score / batch_score / select_state / create_batch_states with the reference's cache semantics.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from ... import kernels as K
from ...blocks import Ctx, Seeds, empty
from .transformer_decoder import AbsDecoder


class LSTMLayer(nn.Module):
    """One torch.nn.LSTM(idim, H, 1, batch_first=True) layer: its parameters (names, shapes, init), our kernels."""

    def __init__(self, idim: int, hidden_size: int):
        super().__init__()
        ref = nn.LSTM(idim, hidden_size, 1, batch_first=True)
        self.weight_ih_l0 = ref.weight_ih_l0
        self.weight_hh_l0 = ref.weight_hh_l0
        self.bias_ih_l0 = ref.bias_ih_l0
        self.bias_hh_l0 = ref.bias_hh_l0
        self.H = hidden_size

    def _xproj(self, x2d):
        """x W_ih^T + b_ih + b_hh for every row."""
        bsum = torch.empty_like(self.bias_ih_l0)
        K.scale_dropout(self.bias_ih_l0.detach(), bsum, r=self.bias_hh_l0.detach())
        return K.linear_fwd(x2d, self.weight_ih_l0, bsum, empty(x2d.shape[0], 4 * self.H, like=x2d))

    def fwd(self, x2d, B: int, U1: int, keep: bool = True):
        """x2d (B*U1, idim) rows (b, u) -> out (B*U1, H); zero initial state."""
        H = self.H
        xp = self._xproj(x2d).view(B, U1, 4 * H)
        out = empty(B, U1, H, like=x2d)
        cs = empty(B, U1, H, like=x2d)
        acts = empty(B, U1, 4 * H, like=x2d) if keep else None
        # h shifted by one step (row (b, u) holds h_{u-1}; zeros at u = 0): the operand of dW_hh's one GEMM
        hprev = torch.zeros(B, U1, H, dtype=torch.float32, device=x2d.device) if keep else None
        W = self.weight_hh_l0.detach()
        for u in range(U1):
            K.lstm_cell_fwd(xp[:, u], out[:, u - 1] if u else None, cs[:, u - 1] if u else None, W,
                            acts[:, u] if keep else None, out[:, u],
                            hprev[:, u + 1] if keep and u + 1 < U1 else None, cs[:, u])
        return out.view(B * U1, H), (Ctx(x=x2d, acts=acts, cs=cs, hprev=hprev, B=B, U1=U1) if keep else None)

    def bwd(self, c, dout2d, need_dx: bool = True):
        """dout2d (B*U1, H) -> dx (B*U1, idim); parameter gradients accumulated."""
        B, U1, H = c.B, c.U1, self.H
        dout = dout2d.view(B, U1, H)
        dg = empty(B, U1, 4 * H, like=dout2d)
        dc = empty(B, H, like=dout2d)
        W = self.weight_hh_l0.detach()
        for u in range(U1 - 1, -1, -1):
            last = u + 1 == U1
            K.lstm_cell_bwd(dout[:, u], None if last else dg[:, u + 1], W, c.acts[:, u], c.cs[:, u],
                            c.cs[:, u - 1] if u else None, None if last else dc, dc, dg[:, u])
        dg2d = dg.view(B * U1, 4 * H)
        K.linear_bwd_weight(dg2d, c.x, self.weight_ih_l0.grad, self.bias_ih_l0.grad)
        K.linear_bwd_weight(dg2d, c.hprev.view(B * U1, H), self.weight_hh_l0.grad, self.bias_hh_l0.grad)
        if not need_dx:
            return None
        return K.linear_bwd_data(dg2d, self.weight_ih_l0, empty(B * U1, c.x.shape[1], like=dout2d))

    def step(self, x2d, h_prev, c_prev, h_next, c_next):
        """One step from a carried state: x2d (n, idim), h_prev / c_prev (n, H) -> h_next / c_next (n, H) written."""
        K.lstm_cell_fwd(self._xproj(x2d), h_prev, c_prev, self.weight_hh_l0.detach(), None, h_next, None, c_next)
        return h_next


class TransducerDecoder(AbsDecoder):
    def __init__(self, vocab_size: int, rnn_type: str = "lstm", num_layers: int = 1, hidden_size: int = 320,
                 dropout: float = 0.0, dropout_embed: float = 0.0, embed_pad: int = 0):
        if rnn_type not in {"lstm", "gru"}:
            raise ValueError(f"Not supported: rnn_type={rnn_type}")
        if rnn_type == "gru":
            raise NotImplementedError("rnn_type: gru -- the predictor's recurrence kernels are the LSTM's (rnn_type: lstm)")
        super().__init__()
        self.embed = nn.Embedding(vocab_size, hidden_size, padding_idx=embed_pad)
        self.decoder = nn.ModuleList([LSTMLayer(hidden_size, hidden_size) for _ in range(num_layers)])
        self.dropout = dropout
        self.dropout_embed = dropout_embed
        self.dlayers = num_layers
        self.dunits = hidden_size
        self.dtype = rnn_type
        self.odim = vocab_size
        self.ignore_id = -1
        self.blank_id = embed_pad
        self.device = next(self.parameters()).device
        self.flat = None

    def attach_flat(self, flat):
        self.flat = flat

    def set_device(self, device: torch.device):
        self.device = device

    # ------------------------------------------------------------------ training
    def _embed(self, tok, n, p=0.0, seed=0):
        x = torch.empty(n, self.dunits, dtype=torch.float32, device=tok.device)
        zero_pe = torch.zeros(1, self.dunits, dtype=torch.float32, device=tok.device)
        K.embed_fwd(tok, self.embed.weight, zero_pe, x, 1, 1.0, p, seed)
        return x

    def run_forward(self, dec_in, dec_in_grad, seeds: Seeds, training: bool, keep: bool = True):
        """dec_in (B, U1) int64 ([blank] + y, blank-padded); dec_in_grad: the same with embed_pad replaced by -1
        (the rows whose embedding gets a gradient).  Returns dec_out (B*U1, H) and the saved context."""
        B, U1 = dec_in.shape
        pe_, se = (self.dropout_embed if training else 0.0), seeds.next()
        x = self._embed(dec_in, B * U1, pe_, se)
        p = self.dropout if training else 0.0
        layers, dseeds = [], []
        for layer in self.decoder:
            x, c = layer.fwd(x, B, U1, keep)
            s = seeds.next()
            if p > 0.0:
                x = K.scale_dropout(x, torch.empty_like(x), drop_p=p, seed=s)
            layers.append(c)
            dseeds.append(s)
        return x, Ctx(tok=dec_in_grad, pe=pe_, se=se, p=p, layers=layers, dseeds=dseeds)

    def run_backward(self, saved, ddec, grad_hook=None):
        """ddec (B*U1, H): the gradient of dec_out."""
        d = ddec
        for i in range(len(self.decoder) - 1, -1, -1):
            if saved.p > 0.0:
                d = K.scale_dropout(d, torch.empty_like(d), drop_p=saved.p, seed=saved.dseeds[i])
            d = self.decoder[i].bwd(saved.layers[i], d)
            saved.layers[i] = None
        K.embed_bwd(saved.tok, d, self.embed.weight.grad, 1.0, saved.pe, saved.se)
        if grad_hook is not None:
            grad_hook(self)

    def forward(self, labels: torch.Tensor) -> torch.Tensor:
        """Inference-style forward (no parameter gradients): labels (B, L) -> dec_out (B, L, H)."""
        from ..encoder.abs_encoder import draw_seed
        labels = labels.to(self.embed.weight.device).long().contiguous()
        with torch.no_grad():
            out, _ = self.run_forward(labels, None, Seeds(draw_seed()), self.training, keep=False)
        return out.view(labels.shape[0], labels.shape[1], self.dunits)

    # ------------------------------------------------------------------ inference
    def init_state(self, batch_size: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        dev = self.embed.weight.device
        return (torch.zeros(self.dlayers, batch_size, self.dunits, device=dev),
                torch.zeros(self.dlayers, batch_size, self.dunits, device=dev))

    def rnn_forward(self, sequence: torch.Tensor, state):
        """One step: sequence (n, 1, H) embeddings, state ((N, n, H), (N, n, H)) -> (n, 1, H), new state."""
        h_prev, c_prev = state
        n = sequence.shape[0]
        h_next, c_next = self.init_state(n)
        x = sequence.reshape(n, self.dunits)
        with torch.no_grad():
            for l, layer in enumerate(self.decoder):
                x = layer.step(x, h_prev[l], c_prev[l], h_next[l], c_next[l])
        return x.view(n, 1, self.dunits), (h_next, c_next)

    def _embed_labels(self, labels: List[int]) -> torch.Tensor:
        tok = K.h2d(torch.tensor(labels, dtype=torch.long), self.embed.weight.device)
        with torch.no_grad():
            return self._embed(tok, len(labels)).view(len(labels), 1, self.dunits)

    def score(self, hyp, cache: Dict[str, Any]):
        """transducer_decoder.py:161-188: (dec_out (H,), new state, label (1,))."""
        label = torch.full((1,), hyp.yseq[-1], dtype=torch.long)
        str_labels = "_".join(list(map(str, hyp.yseq)))
        if str_labels in cache:
            dec_out, dec_state = cache[str_labels]
        else:
            dec_out, dec_state = self.rnn_forward(self._embed_labels([hyp.yseq[-1]]), hyp.dec_state)
            cache[str_labels] = (dec_out, dec_state)
        return dec_out[0][0], dec_state, label

    def batch_score(self, hyps, dec_states, cache: Dict[str, Any], use_lm: bool):
        """transducer_decoder.py:190-253.  use_lm: the reference's argument; no LM is served with a transducer, so
        the third return value is always None."""
        final_batch = len(hyps)
        process = []
        done = [None] * final_batch
        for i, hyp in enumerate(hyps):
            str_labels = "_".join(list(map(str, hyp.yseq)))
            if str_labels in cache:
                done[i] = cache[str_labels]
            else:
                process.append((str_labels, hyp.yseq[-1], hyp.dec_state))
        if process:
            p_dec_states = self.create_batch_states(self.init_state(len(process)), [p[2] for p in process])
            dec_out, new_states = self.rnn_forward(self._embed_labels([p[1] for p in process]), p_dec_states)
        j = 0
        for i in range(final_batch):
            if done[i] is None:
                state = self.select_state(new_states, j)
                done[i] = (dec_out[j], state)
                cache[process[j][0]] = (dec_out[j], state)
                j += 1
        dec_out = torch.cat([d[0] for d in done], dim=0)
        dec_states = self.create_batch_states(dec_states, [d[1] for d in done])
        return dec_out, dec_states, None

    def select_state(self, states, idx: int):
        return (states[0][:, idx:idx + 1, :].contiguous(), states[1][:, idx:idx + 1, :].contiguous())

    def create_batch_states(self, states, new_states, check_list: Optional[List] = None):
        return (torch.cat([s[0] for s in new_states], dim=1).contiguous(),
                torch.cat([s[1] for s in new_states], dim=1).contiguous())
