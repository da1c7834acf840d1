"""ESPnetLanguageModel -- espnet2/lm/espnet_model.py:13-136: the negative log-likelihood of token sequences under
an LM (perplexity, validation loss) and the LM training step.  sos = eos = vocab_size - 1; ignore_id 0 is the
padding id.

Training (the LM in .train() mode, gradients enabled): forward = prepare (host: the '<sos> w1 w2' / 'w1 w2 <eos>'
pair, lengths, seeds) + forward_prepared (device only, capturable by torch.cuda.graph): TransformerLM.run_forward,
then esp_label_smoothing with smoothing 0 (cross-entropy and its gradient in one pass) and esp_reduce_losses, which
divides by the batch's own count of non-padded targets on the device (= ntokens; a replayed graph must not bake a
host value).  Padded target rows carry PAD_TARGET, an id no token has, as the loss kernel's `ignore`: the reference
masks padding by position, so a real target equal to ignore_id still counts.  LMFn anchors the step on a parameter:
loss.backward() runs TransformerLM.run_backward, which fills flat.grad."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import kernels as K
from ..asr.encoder.abs_encoder import draw_seed
from ..asr.espnet_model import AbsESPnetModel, Prepared
from ..blocks import Ctx, Seeds, empty
from .transformer_lm import AbsLM

PAD_TARGET = -1  # the target of a padded row: esp_label_smoothing's `ignore`


class LMFn(torch.autograd.Function):
    """The LM training step of one prepared batch; backward writes the parameter gradients into flat.grad (the
    anchor parameter only ties the node into the autograd graph)."""

    @staticmethod
    def forward(ctx, anchor, model, prep):
        loss, state = model._step_forward(prep, True)
        ctx.model, ctx.state = model, state
        return loss.clone()

    @staticmethod
    def backward(ctx, g_loss):
        ctx.model._step_backward(ctx.state, g_loss.contiguous())
        ctx.state = None
        return None, None, None


class ESPnetLanguageModel(AbsESPnetModel):
    def __init__(self, lm: AbsLM, vocab_size: int, ignore_id: int = 0):
        super().__init__()
        self.lm = lm
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        self.ignore_id = ignore_id  # may be assumed 0, shared with the CTC blank of the ASR model

    def flatten(self, device=None):
        return self.lm.flatten(device)

    @property
    def flat(self):
        """The LM's flat parameter / gradient buffers (what Trainer and FusedAdam read)."""
        return self.lm.flat

    # ------------------------------------------------------------------ training step
    def _pair(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None):
        """'<sos> w1 w2 w3' and 'w1 w2 w3 <eos>' on the host (espnet_model.py:49-57): x padded with 0 (the LM's key
        mask), t with ignore_id; x_lengths = text_lengths + 1; pad: the positions past a row's length."""
        text_lengths = text_lengths.to("cpu", torch.int64)
        text = text.to("cpu", torch.int64)
        text = text[:, : int(text_lengths.max())] if max_length is None else text[:, : int(max_length)]
        x = F.pad(text, [1, 0], "constant", self.eos)
        t = F.pad(text, [0, 1], "constant", self.ignore_id)
        for i, l in enumerate(text_lengths):
            t[i, l] = self.sos
        x_lengths = text_lengths + 1
        pad = torch.arange(x.shape[1])[None, :] >= x_lengths[:, None]
        x = x.masked_fill(pad, 0)  # the reference's batches pad with 0 as well: the LM's key mask
        return x, t, x_lengths, pad

    def prepare(self, text: torch.Tensor, text_lengths: torch.Tensor, l_bucket: Optional[int] = None) -> Prepared:
        """All host-side work of a training step.  l_bucket: pad the token axis to l_bucket columns (x with 0, the
        targets with PAD_TARGET: rows that nothing reads), so batches of one bucket share a captured graph."""
        x, t, x_lengths, pad = self._pair(text, text_lengths)
        if not bool(((x != 0) == ~pad).all()) or int(x_lengths.min()) < 1:
            raise ValueError("ESPnetLanguageModel.prepare: token 0 is padding and may only trail a row (the "
                             "reference masks every key whose id is 0)")
        t = t.masked_fill(pad, PAD_TARGET)
        B, L = x.shape
        if l_bucket is not None and int(l_bucket) > L:
            extra = int(l_bucket) - L
            x = F.pad(x, [0, extra], "constant", 0)
            t = F.pad(t, [0, extra], "constant", PAD_TARGET)
            L = int(l_bucket)
        ntokens = x_lengths.sum()
        host = dict(x=x.reshape(-1).contiguous(), t=t.reshape(-1).contiguous(), klen=x_lengths.to(torch.int32),
                    weight=ntokens.view(1))
        return Prepared(B=B, L=L, host=host, seed=draw_seed(), ntokens=int(ntokens))

    def _step_forward(self, prep: Prepared, want_grad: bool):
        d = prep.dev
        B, L = prep.B, prep.L
        lm = self.lm
        logits, saved = lm.run_forward(d["x"], d["klen"], B, L, Seeds(prep.seed), lm.training)
        R, V = logits.shape
        grad = empty(R, V, like=logits) if want_grad else None
        row_loss = torch.empty(R, dtype=torch.float64, device=logits.device)
        row_stat = torch.empty(2 * R, dtype=torch.int32, device=logits.device)
        # smoothing 0: cross-entropy; gscale 1: the 1 / ntokens comes from the device count below
        K.label_smoothing(logits, d["t"], V, PAD_TARGET, 0.0, 1.0, grad, row_loss, row_stat)
        out = empty(5, like=logits)
        # denom 0: sum(nll) / (the rows whose target is not PAD_TARGET) = nll.sum() / ntokens; out[4] its reciprocal
        K.reduce_losses(None, B, True, row_loss, row_stat, R, 0.0, 0.0, out)
        return out[3:4], Ctx(saved=saved, grad=grad, inv=out[4:5])

    def _step_backward(self, state, g_loss: torch.Tensor) -> None:
        g = state.grad
        K.scale_by_dev(g, state.inv)
        K.scale_by_dev(g, g_loss)
        self.lm.run_backward(state.saved, g)

    def forward_prepared(self, prep: Prepared):
        """The step's device work from a prepared batch (prep.to_device(...) done): no host->device traffic and no
        host synchronisation, so forward + backward can be captured as one graph and re-targeted at another batch
        of the same shape with Prepared.copy_into."""
        anchor = self.lm.decoder.weight
        if torch.is_grad_enabled() and anchor.requires_grad:
            loss = LMFn.apply(anchor, self, prep)
        else:
            loss, _ = self._step_forward(prep, False)
        return loss, dict(loss=loss.detach()), prep.dev["weight"]

    def nll(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
        """text (B, L), text_lengths (B,) -> (nll (B, L + 1), zero past each row's length + 1; x_lengths (B,))."""
        batch_size = text.size(0)
        x, t, x_lengths, pad = self._pair(text, text_lengths, max_length)
        y, _ = self.lm(x, None)
        V = y.shape[-1]
        logits = y.reshape(-1, V).contiguous()
        logp = torch.empty_like(logits)
        K.log_softmax(logits, logp, logits.shape[0], V)
        nll = -logp.gather(1, t.reshape(-1, 1).to(logp.device)).reshape(-1)
        nll = nll.masked_fill(pad.reshape(-1).to(nll.device), 0.0)
        return nll.view(batch_size, -1), x_lengths

    def batchify_nll(self, text: torch.Tensor, text_lengths: torch.Tensor, batch_size: int = 100
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """nll over the rows in batches of batch_size (all padded to the longest row)."""
        total_num = text.size(0)
        if total_num <= batch_size:
            return self.nll(text, text_lengths)
        nlls, x_lengths = [], []
        max_length = int(text_lengths.max())
        for start in range(0, total_num, batch_size):
            end = min(start + batch_size, total_num)
            batch_nll, batch_x_lengths = self.nll(text[start:end], text_lengths[start:end], max_length=max_length)
            nlls.append(batch_nll)
            x_lengths.append(batch_x_lengths)
        nll, x_lengths = torch.cat(nlls), torch.cat(x_lengths)
        assert nll.size(0) == total_num and x_lengths.size(0) == total_num
        return nll, x_lengths

    def forward(self, text: torch.Tensor, text_lengths: torch.Tensor, **kwargs
                ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if not self.lm.training:
                raise NotImplementedError("ESPnetLanguageModel.forward: gradients are implemented in training mode "
                                          "only; call .train() first, or call it under torch.no_grad() for the "
                                          "validation loss")
            dev = self.lm._ready()
            self.flat.ensure_grads()  # after a torch optimizer's zero_grad(set_to_none=True)
            return self.forward_prepared(self.prepare(text, text_lengths).to_device(dev))
        nll, y_lengths = self.nll(text, text_lengths)
        ntokens = y_lengths.sum()
        loss = nll.sum() / ntokens.to(nll.device)
        stats = dict(loss=loss.detach())
        return loss, stats, ntokens.to(loss.device)

    def collect_feats(self, text: torch.Tensor, text_lengths: torch.Tensor, **kwargs) -> Dict[str, torch.Tensor]:
        return {}
