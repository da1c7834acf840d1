"""BeamSearchTransducer — espnet2/asr/transducer/beam_search_transducer.py:43-354 (greedy and `default`).

`beam_size <= 1` is greedy_search (at most one label per frame, as the reference's loop), `search_type="default"` is
default_beam_search with its duplicate hypotheses, `score_norm` and `nbest`.  lin_enc is applied once to all frames; a
step is LSTM cell(s) -> lin_dec -> activation -> lin_out -> log-softmax on the device, and the host reads one (V,) row
of log-probabilities back per expansion (the hypothesis bookkeeping is the reference's host code).  The other search
types (tsd, alsd, nsc, maes) and an LM are not served and raise by name.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional

import torch


@dataclass
class Hypothesis:
    """Default hypothesis definition for Transducer search algorithms."""
    score: float
    yseq: List[int]
    dec_state: Any
    lm_state: Any = None


def default_beam_search(logp_fn: Callable[[Hypothesis, int, Dict], tuple], n_frames: int, init_state, beam_size: int,
                        vocab_size: int, blank_id: int = 0, trace: Optional[Callable[[str, float], None]] = None
                        ) -> List[Hypothesis]:
    """The host side of default_beam_search (beam_search_transducer.py:255-352).  logp_fn(hyp, t, cache) returns
    (logp (V,) host float tensor of frame t after hyp's labels, decoder state after hyp's last label).
    trace(kind, margin): told the margin of every decision that depends on a score comparison -- "max" (the
    expanded hypothesis against the runner-up), "topk" (the last label kept against the first one cut) and
    "hyps_max" (each kept hypothesis against the best open one); the fixture generator records their minimum."""
    beam = min(beam_size, vocab_size)
    beam_k = min(beam, vocab_size - 1)
    kept_hyps = [Hypothesis(score=0.0, yseq=[blank_id], dec_state=init_state)]
    cache: Dict[str, Any] = {}
    for t in range(n_frames):
        hyps = kept_hyps
        kept_hyps = []
        while True:
            max_hyp = max(hyps, key=lambda x: x.score)
            hyps.remove(max_hyp)
            logp, state = logp_fn(max_hyp, t, cache)
            top_k = logp[1:].topk(beam_k, dim=-1)
            if trace is not None:
                if hyps:
                    trace("max", float(max_hyp.score) - max(float(h.score) for h in hyps))
                if beam_k < vocab_size - 1:
                    srt = logp[1:].sort(descending=True)[0]
                    trace("topk", float(srt[beam_k - 1] - srt[beam_k]))
            kept_hyps.append(Hypothesis(score=(max_hyp.score + float(logp[0:1])), yseq=max_hyp.yseq[:],
                                        dec_state=max_hyp.dec_state, lm_state=max_hyp.lm_state))
            for lp, k in zip(*top_k):
                hyps.append(Hypothesis(score=max_hyp.score + float(lp), yseq=max_hyp.yseq[:] + [int(k + 1)],
                                       dec_state=state, lm_state=max_hyp.lm_state))
            hyps_max = float(max(hyps, key=lambda x: x.score).score)
            if trace is not None:
                for hyp in kept_hyps:
                    trace("hyps_max", abs(float(hyp.score) - hyps_max))
            kept_most_prob = sorted([hyp for hyp in kept_hyps if hyp.score > hyps_max], key=lambda x: x.score)
            if len(kept_most_prob) >= beam:
                kept_hyps = kept_most_prob
                break
    return kept_hyps


class BeamSearchTransducer:
    def __init__(self, decoder, joint_network, beam_size: int, lm=None, lm_weight: float = 0.1,
                 search_type: str = "default", max_sym_exp: int = 2, u_max: int = 50, nstep: int = 1,
                 prefix_alpha: int = 1, expansion_gamma: float = 2.3, expansion_beta: int = 2, score_norm: bool = True,
                 nbest: int = 1, token_list: Optional[List[str]] = None):
        # (the reference's signature: lm_weight and the other searches' parameters are accepted and unused)
        if lm is not None:
            raise NotImplementedError("BeamSearchTransducer: lm (shallow fusion with a transducer) is not served")
        self.decoder = decoder
        self.joint_network = joint_network
        self.beam_size = beam_size
        self.vocab_size = decoder.odim
        self.token_list = token_list
        self.blank_id = decoder.blank_id
        if self.beam_size <= 1:
            self.search_algorithm = self.greedy_search
        elif search_type == "default":
            self.search_algorithm = self.default_beam_search
        elif search_type in ("tsd", "alsd", "nsc", "maes"):
            raise NotImplementedError(f"search_type={search_type}: only greedy (beam_size <= 1) and `default` are served")
        else:
            raise NotImplementedError(f"search_type={search_type}")
        self.score_norm = score_norm
        self.nbest = nbest

    def __call__(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, D_enc) on the device -> n-best hypotheses (yseq starts with the blank)."""
        self.decoder.set_device(enc_out.device)
        return self.search_algorithm(enc_out)

    def sort_nbest(self, hyps: List[Hypothesis]) -> List[Hypothesis]:
        if self.score_norm:
            hyps.sort(key=lambda x: x.score / len(x.yseq), reverse=True)
        else:
            hyps.sort(key=lambda x: x.score, reverse=True)
        return hyps[: self.nbest]

    def _logp(self, pe: torch.Tensor, t: int, dec_out: torch.Tensor) -> torch.Tensor:
        """Frame t's log-probabilities after dec_out (H,), on the host."""
        return self.joint_network.step_logp(pe[t:t + 1], dec_out.view(1, -1))[0].cpu()

    def greedy_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        pe = self.joint_network.project_enc(enc_out)
        hyp = Hypothesis(score=0.0, yseq=[self.blank_id], dec_state=self.decoder.init_state(1))
        cache: Dict[str, Any] = {}
        dec_out, state, _ = self.decoder.score(hyp, cache)
        for t in range(enc_out.shape[0]):
            logp = self._logp(pe, t, dec_out)
            top_logp, pred = torch.max(logp, dim=-1)
            if pred != self.blank_id:
                hyp.yseq.append(int(pred))
                hyp.score += float(top_logp)
                hyp.dec_state = state
                dec_out, state, _ = self.decoder.score(hyp, cache)
        return [hyp]

    def default_beam_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        pe = self.joint_network.project_enc(enc_out)

        def logp_fn(hyp, t, cache):
            dec_out, state, _ = self.decoder.score(hyp, cache)
            return self._logp(pe, t, dec_out), state

        kept = default_beam_search(logp_fn, enc_out.shape[0], self.decoder.init_state(1), self.beam_size,
                                   self.vocab_size, self.blank_id)
        return self.sort_nbest(kept)
