"""ESPnetLanguageModel -- espnet2/lm/espnet_model.py:13-136: the negative log-likelihood of token sequences under
an LM (perplexity, validation loss).  sos = eos = vocab_size - 1; ignore_id 0 is the padding id.  Training the LM
(a backward pass) is not implemented: forward raises when it would be asked for gradients."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import kernels as K
from ..asr.espnet_model import AbsESPnetModel
from .transformer_lm import AbsLM


class ESPnetLanguageModel(AbsESPnetModel):
    def __init__(self, lm: AbsLM, vocab_size: int, ignore_id: int = 0):
        super().__init__()
        self.lm = lm
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        self.ignore_id = ignore_id  # may be assumed 0, shared with the CTC blank of the ASR model

    def flatten(self, device=None):
        return self.lm.flatten(device)

    def nll(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
        """text (B, L), text_lengths (B,) -> (nll (B, L + 1), zero past each row's length + 1; x_lengths (B,))."""
        batch_size = text.size(0)
        text_lengths = text_lengths.to("cpu", torch.int64)
        text = text.to("cpu", torch.int64)
        text = text[:, : int(text_lengths.max())] if max_length is None else text[:, : int(max_length)]
        # '<sos> w1 w2 w3' and 'w1 w2 w3 <eos>'
        x = F.pad(text, [1, 0], "constant", self.eos)
        t = F.pad(text, [0, 1], "constant", self.ignore_id)
        for i, l in enumerate(text_lengths):
            t[i, l] = self.sos
        x_lengths = text_lengths + 1
        pad = torch.arange(x.shape[1])[None, :] >= x_lengths[:, None]
        x = x.masked_fill(pad, 0)  # the reference's batches pad with 0 as well: the LM's key mask
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
            raise NotImplementedError("ESPnetLanguageModel.forward: LM training (backward) is not implemented; call it "
                                      "under torch.no_grad() for the validation loss")
        nll, y_lengths = self.nll(text, text_lengths)
        ntokens = y_lengths.sum()
        loss = nll.sum() / ntokens.to(nll.device)
        stats = dict(loss=loss.detach())
        return loss, stats, ntokens.to(loss.device)

    def collect_feats(self, text: torch.Tensor, text_lengths: torch.Tensor, **kwargs) -> Dict[str, torch.Tensor]:
        return {}
