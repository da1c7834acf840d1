"""MaskCTCModel / MaskCTCInference — drop-in for espnet2/asr/maskctc_model.py (Mask-CTC: CTC + masked-LM decoder,
non-autoregressive mask-predict decoding).

Training is ESPnetASRModel's step with other decoder targets: mask_uniform (add_mask_token.py:13-39) replaces
add_sos_eos, the decoder is an MLMDecoder (non-causal, vocab_size + 1 classes) and the label-smoothing loss runs over
vocab_size + 1 classes with the unmasked positions ignored.  Everything else (CTC branch, intermediate CTC, the
loss kernels, the explicit backward, forward_prepared / forward_explicit, the HIP-graph trainer path) is inherited:
the masks are host tensors of `prep.host` like every other per-step input.

Decoding (MaskCTCInference.forward, maskctc_model.py:284-346) runs on the device: esp_maskctc_init turns the CTC
posteriors into the masked input, each refinement pass is one MLMDecoder.forward_masked over source-attention keys
and values projected once, and esp_maskctc_fill takes the pass's decisions in place.  The host reads two numbers
before the loop (L and mask_num) and the token ids after it.

MaskCTCInference.forward_batch decodes U ragged utterances through the same launches: esp_maskctc_init_batch /
esp_maskctc_fill_batch run one workgroup per utterance and keep each utterance's pass plan on the device, and
MLMDecoder.forward_masked_batch runs a pass of all active utterances at once.  The host reads the U plans before the
loop and the token rows after it.
"""
from __future__ import annotations

import logging
from typing import List, Optional, Sequence, Tuple, Union

import numpy
import torch
from torch import nn

from .. import kernels as K
from ..blocks import Seeds
from .beam_search import Hypothesis
from .decoder.mlm_decoder import MLMDecoder
from .error_calculator import ErrorCalculator
from .espnet_model import ESPnetASRModel


def mask_uniform(ys_pad: torch.Tensor, mask_token: int, eos: int, ignore_id: int,
                 draws: Optional[Sequence] = None, width: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """add_mask_token.py:13-39 on the host: per utterance a uniformly drawn number of positions (1 .. its length) is
    drawn with replacement and replaced by <mask> in ys_in; ys_out holds the original token there and ignore_id
    everywhere else.  ys_in is padded with eos, ys_out with ignore_id.

    draws None: numpy.random.randint(1, len + 1) then numpy.random.choice(len, n) per utterance, in the reference's
    order on NumPy's global generator (the same NumPy seed gives the reference's masks).  draws: the position
    arrays themselves, one per utterance (repeats allowed, as choice() returns them).  width: pad to this many
    columns (>= the longest target) instead of the longest target."""
    ys = [row[row != ignore_id] for row in ys_pad]
    B = len(ys)
    if draws is not None and len(draws) != B:
        raise ValueError(f"mask_uniform: {len(draws)} mask draws for {B} utterances")
    longest = max(int(y.numel()) for y in ys)
    L = longest if width is None else int(width)
    if L < longest:
        raise ValueError(f"mask_uniform: width {L} below the longest target ({longest})")
    ys_in = torch.full((B, L), eos, dtype=torch.long)
    ys_out = torch.full((B, L), ignore_id, dtype=torch.long)
    for i, y in enumerate(ys):
        n = int(y.numel())
        if draws is None:
            num = numpy.random.randint(1, n + 1)
            idx = numpy.random.choice(n, num)
        else:
            idx = numpy.asarray(draws[i], dtype=numpy.int64).reshape(-1)
            if idx.size == 0 or idx.min() < 0 or idx.max() >= n:
                raise ValueError(f"mask_uniform: mask draws {idx.tolist()} for a target of {n} tokens")
        idx = torch.from_numpy(numpy.asarray(idx, dtype=numpy.int64))
        ys_in[i, :n] = y
        ys_in[i, idx] = mask_token
        ys_out[i, idx] = y[idx]
    return ys_in, ys_out


class MaskCTCModel(ESPnetASRModel):
    """Hybrid CTC / masked-LM model.  vocab_size and token_list are the CTC's (without <mask>); the model appends
    sym_mask (to its own copy: the caller's list is left alone), so self.vocab_size = vocab_size + 1 and
    self.mask_token = vocab_size.  The decoder must be an MLMDecoder built with the unextended vocab_size.

    forward(..., mask_draws=) / prepare(..., mask_draws=) take the mask positions explicitly (mask_uniform's draws),
    as specaug_draws does for SpecAug."""

    target_draw_args = ("mask_draws",)

    def __init__(self, vocab_size: int, token_list: Union[Tuple[str, ...], List[str]], frontend, specaug, normalize,
                 preencoder, encoder, postencoder, decoder, ctc, joint_network=None, ctc_weight: float = 0.5,
                 interctc_weight: float = 0.0, ignore_id: int = -1, lsm_weight: float = 0.0,
                 length_normalized_loss: bool = False, report_cer: bool = True, report_wer: bool = True,
                 sym_space: str = "<space>", sym_blank: str = "<blank>", sym_mask: str = "<mask>",
                 extract_feats_in_collect_stats: bool = True):
        if decoder is not None and not isinstance(decoder, MLMDecoder):
            raise TypeError(f"MaskCTCModel needs an MLMDecoder (decoder: mlm), got {type(decoder).__name__}")
        super().__init__(vocab_size=vocab_size, token_list=token_list, frontend=frontend, specaug=specaug,
                         normalize=normalize, preencoder=preencoder, encoder=encoder, postencoder=postencoder,
                         decoder=decoder, ctc=ctc, joint_network=joint_network, ctc_weight=ctc_weight,
                         interctc_weight=interctc_weight, ignore_id=ignore_id, lsm_weight=lsm_weight,
                         length_normalized_loss=length_normalized_loss, report_cer=report_cer, report_wer=report_wer,
                         sym_space=sym_space, sym_blank=sym_blank,
                         extract_feats_in_collect_stats=extract_feats_in_collect_stats)
        # <mask> joins the vocabulary of the decoder and of the MLM loss; the CTC keeps the unextended one
        self.token_list = list(token_list) + [sym_mask]
        self.vocab_size = vocab_size + 1
        self.mask_token = self.vocab_size - 1
        if self.decoder is not None and self.decoder.vocab_size != self.vocab_size:
            raise ValueError(f"MLMDecoder of {self.decoder.vocab_size} classes for a vocabulary of {vocab_size} + <mask>")
        self.error_calculator = (ErrorCalculator(self.token_list, sym_space, sym_blank, report_cer, report_wer)
                                 if report_cer or report_wer else None)

    def _decoder_targets(self, text_cpu, tl_cpu, u_bucket, mask_draws=None):
        """mask_uniform instead of add_sos_eos: L = Umax columns (u_bucket columns when bucketed), no sos / eos
        position, ys_in_lens = text_lengths."""
        ys_in, ys_out = mask_uniform(text_cpu, self.mask_token, self.eos, self.ignore_id, draws=mask_draws,
                                     width=None if u_bucket is None else max(int(u_bucket), int(text_cpu.shape[1])))
        return ys_in, ys_out, tl_cpu.to(torch.long)

    def _stats(self, loss, others, inter, detach: bool):
        """maskctc_model.py:144-209: loss_ctc / cer_ctc only with a CTC branch, loss_mlm, acc_mlm, loss."""
        stats = {}
        if self.ctc is not None:
            stats["loss_ctc"] = others[0:1]
            stats["cer_ctc"] = None
        if inter:
            stats.update(inter["stats"])
            stats.update({"cer" + k[len("loss"):]: None for k in inter["stats"] if k.startswith("loss_interctc_layer")})
        stats["loss_mlm"] = others[1:2] if self.decoder is not None else None
        stats["acc_mlm"] = others[2:3] if self.decoder is not None else None
        stats["loss"] = loss
        if detach:
            stats = {k: t if t is None else t.detach() for k, t in stats.items()}
        return stats

    def _error_rates(self, encoder_out, prep):
        """Eval mode: the greedy-CTC error rate only (no decoder-argmax cer / wer: the MLM rows are not a
        transcript)."""
        prep.pop("eval_logits", None)
        if self.ctc is None:
            return {}
        ys_hat = self.ctc.argmax(encoder_out).cpu()
        cer = self.error_calculator(ys_hat, prep.ys_pad_cpu, is_ctc=True)
        return {"cer_ctc": None if cer is None else torch.tensor([cer], dtype=torch.float32, device=encoder_out.device)}

    def nll(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens):
        raise NotImplementedError

    def batchify_nll(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, batch_size: int = 100):
        raise NotImplementedError


class MaskCTCInference(nn.Module):
    """Mask-CTC mask-predict decoding of one utterance (maskctc_model.py:262-346), or of a batch of them
    (forward_batch).

    forward(enc_out (T, D) on the device) -> Hypothesis(yseq = [<mask>] + tokens + [<mask>]), yseq on the host.
    Reference behaviour kept as it is: a pass's argmax runs over all vocab_size + 1 classes (a position may be
    "filled" with <mask> and stays masked), the number of positions filled per pass is fixed at mask_num //
    num_iter, and the confidence ranking a pass's fills is the raw logit maximum, not a probability.

    Host traffic: one read of (L, mask_num) before the loop (the decoder's shapes and the pass count depend on
    them), none inside it, one read of the tokens after it.  L == 0 (all blank) and mask_num == 0 return without
    running the decoder.  `last` keeps the counts of the latest utterance (L, mask_num, num_iter)."""

    def __init__(self, asr_model: MaskCTCModel, n_iterations: int, threshold_probability: float):
        super().__init__()
        if asr_model.ctc is None or asr_model.decoder is None:
            raise ValueError("MaskCTCInference needs the model's CTC and its MLM decoder (0 < ctc_weight < 1)")
        self.ctc = asr_model.ctc
        self.mlm = asr_model.decoder
        self.mask_token = asr_model.mask_token
        self.blank_id = asr_model.blank_id
        self.n_iterations = n_iterations
        self.threshold_probability = threshold_probability
        self.token_list = list(asr_model.token_list)
        dk = self.mlm.D // self.mlm.decoders[0].self_attn.h
        # esp_decode_attn takes head sizes 16 / 32 / 64; another one runs every pass through MLMDecoder.run_forward
        # (the training forward in eval mode: it projects the memory again in every pass)
        self.prepared_memory = dk in (16, 32, 64)
        if not self.prepared_memory:
            logging.warning("MaskCTCInference: head size %d is not served by esp_decode_attn; every pass runs "
                            "MLMDecoder.run_forward and projects the memory again", dk)
        self.last = dict(L=0, mask_num=0, num_iter=0)
        self.last_batch: List[dict] = []

    def ids2text(self, ids: List[int]) -> str:
        text = "".join(self.token_list[i] for i in ids)
        return text.replace("<mask>", "_").replace("<space>", " ")

    def _logits(self, y: torch.Tensor, enc_out: torch.Tensor, mem) -> torch.Tensor:
        if mem is not None:
            return self.mlm.forward_masked(y, mem)
        T, L, dev = enc_out.shape[0], y.shape[0], enc_out.device
        logits, _ = self.mlm.run_forward(enc_out.unsqueeze(0), K.h2d(torch.tensor([T], dtype=torch.int32), dev),
                                         y.unsqueeze(0), K.h2d(torch.tensor([L], dtype=torch.int32), dev), Seeds(0),
                                         False)
        return logits

    @torch.no_grad()
    def forward(self, enc_out: torch.Tensor, trace: Optional[list] = None) -> Hypothesis:
        """trace: a list that receives the device token row after the masking and after every pass (clones; reading
        them is the caller's business, nothing is synchronised here)."""
        if self.mlm.training or self.ctc.training:
            raise RuntimeError("MaskCTCInference.forward: inference only (call .eval() on the model)")
        enc_out = enc_out.to(torch.float32).contiguous()
        lp = self.ctc.log_softmax(enc_out.unsqueeze(0))[0]
        y_in, _, tok_prob, counts = K.maskctc_init(lp, self.mask_token, self.threshold_probability, self.blank_id)
        L, mask_num = (int(v) for v in counts.tolist())  # the one read before the loop
        self.last = dict(L=L, mask_num=mask_num, num_iter=0, tok_prob=tok_prob[:L])
        if L == 0:
            return Hypothesis(yseq=torch.tensor([self.mask_token, self.mask_token], dtype=torch.long))
        y = y_in[:L]
        if trace is not None:
            trace.append(y.clone())
        if mask_num > 0:
            n = self.n_iterations
            num_iter = n if mask_num >= n and n > 0 else mask_num
            self.last["num_iter"] = num_iter
            mem = self.mlm.prepare_memory(enc_out.unsqueeze(0), [enc_out.shape[0]]) if self.prepared_memory else None
            for t in range(num_iter):
                logits = self._logits(y, enc_out, mem)
                # the last pass fills whatever is still masked (k = 0)
                K.maskctc_fill(logits, y, self.mask_token, mask_num // num_iter if t < num_iter - 1 else 0)
                if trace is not None:
                    trace.append(y.clone())
        tokens = y.cpu().tolist()  # the read after the loop
        return Hypothesis(yseq=torch.tensor([self.mask_token] + tokens + [self.mask_token], dtype=torch.long))

    @torch.no_grad()
    def forward_batch(self, enc_pad: torch.Tensor, enc_lens, trace: Optional[list] = None) -> List[Hypothesis]:
        """forward for U utterances through the same launches: enc_pad (U, Tmax, D) on the device, enc_lens (U,) on
        the host -> one Hypothesis per utterance, what forward returns for enc_pad[u, :enc_lens[u]].

        esp_maskctc_init_batch masks every utterance and leaves each one's pass plan {L, mask_num, num_iter, k} on
        the device; the host reads all plans once.  The utterances with a pass to run (the active set) go through
        MLMDecoder.forward_masked_batch as one batch of the longest active L, once per pass for the largest num_iter;
        esp_maskctc_fill_batch applies pass t by each utterance's own plan, so an utterance whose passes are done
        idles in the batch untouched.  Utterances with L == 0 or mask_num == 0 never reach the decoder.  No host read
        inside the loop, one read of the token rows after it.

        trace: receives the (U, Tmax) device token array after the masking and after every pass (clones; row u is
        valid up to L_u).  `last_batch` keeps every utterance's {L, mask_num, num_iter}."""
        if self.mlm.training or self.ctc.training:
            raise RuntimeError("MaskCTCInference.forward_batch: inference only (call .eval() on the model)")
        if enc_pad.dim() != 3:
            raise ValueError(f"forward_batch: enc_pad of shape {tuple(enc_pad.shape)}, expected (U, Tmax, D)")
        U, Tmax, dev = int(enc_pad.shape[0]), int(enc_pad.shape[1]), enc_pad.device
        lens = numpy.asarray(torch.as_tensor(enc_lens).cpu(), dtype=numpy.int32).reshape(-1)
        if U < 1 or lens.shape[0] != U or lens.min() < 1 or lens.max() > Tmax:
            raise ValueError(f"forward_batch: enc_lens {lens.tolist()} for enc_pad of shape {tuple(enc_pad.shape)}")
        enc_pad = enc_pad.to(torch.float32).contiguous()
        lp = self.ctc.log_softmax(enc_pad)
        tlens = K.h2d(torch.from_numpy(lens), dev)
        y_all, _, _, counts = K.maskctc_init_batch(lp, tlens, self.mask_token, self.threshold_probability,
                                                   self.n_iterations, self.blank_id)
        plan = counts.cpu().numpy()  # the one read before the loop
        self.last_batch = [dict(L=int(r[0]), mask_num=int(r[1]), num_iter=int(r[2])) for r in plan]
        if trace is not None:
            trace.append(y_all.clone())
        active = numpy.nonzero(plan[:, 2] > 0)[0].astype(numpy.int32)
        if active.size:
            Lmax, passes = int(plan[active, 0].max()), int(plan[active, 2].max())
            ylens = plan[active, 0].astype(numpy.int32)
            rows32 = K.h2d(torch.from_numpy(active), dev)
            rows64 = rows32.to(torch.int64)
            y_view = y_all[:, :Lmax]
            if self.prepared_memory:
                mem = self.mlm.prepare_memory(enc_pad, lens)
            else:
                hs, hl = enc_pad.index_select(0, rows64), K.h2d(torch.from_numpy(lens[active]), dev)
                yl = K.h2d(torch.from_numpy(ylens), dev)
            for t in range(passes):
                y = y_view.index_select(0, rows64)  # (Ua, Lmax), contiguous
                if self.prepared_memory:
                    logits = self.mlm.forward_masked_batch(y, ylens, mem, active)
                else:
                    logits, _ = self.mlm.run_forward(hs, hl, y, yl, Seeds(0), False)
                K.maskctc_fill_batch(logits.view(active.size, Lmax, -1), y_all, counts, rows32, self.mask_token, t)
                if trace is not None:
                    trace.append(y_all.clone())
        tokens = y_all.cpu().numpy()  # the read after the loop
        m = self.mask_token
        return [Hypothesis(yseq=torch.tensor([m] + tokens[u, :int(plan[u, 0])].tolist() + [m], dtype=torch.long))
                for u in range(U)]
