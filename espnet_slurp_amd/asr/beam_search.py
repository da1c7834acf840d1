"""Joint CTC/attention beam search (espnet/nets/beam_search.py:20-512 with
espnet/nets/scorers/ctc.py, espnet/nets/scorers/length_bonus.py, e2e_asr_common.end_detect).

Same search as the reference's BeamSearch (what Speech2Text runs, as BatchBeamSearch, for an
ESPnet2 ASR model): per running hypothesis the full scorers (decoder log-softmax, length
bonus, and the neural LM of shallow fusion when one is given: scorer "lm") are weighted and
summed, the pre-beam keeps int(pre_beam_ratio * beam) labels by that
sum ("full" key), the CTC prefix scorer scores only those, the hypothesis score is added, the
top `beam` of every hypothesis are pooled, stably sorted and pruned to `beam`; hypotheses that
emit <eos> (or reach maxlen) end, and end_detect stops the search when maxlenratio == 0.

MI355X-side: all running hypotheses are scored together — ONE decoder pass over the stacked
prefixes (the HIP decoder kernels, encoder memory repeated per hypothesis) and ONE launch of
the CTC prefix kernel (esp_ctc_prefix_score: a thread per (hypothesis, candidate)) per output
step; the hypothesis bookkeeping (tiny) happens on the host after one device->host copy.
The decoder is re-run on the full prefix each step (the reference caches layer outputs in
forward_one_step; the last position's output is the same function of the prefix).

BatchBeamSearch (below) is the reference's batch search on the cached one-step decoder
(TransformerDecoder.batch_score: only the newest position is computed, the memory's source-attention
K/V are projected once), for one utterance or for several in lockstep (forward_batch).

BatchBeamSearchOnlineSim (last) is the reference's block-synchronous search for simulated streaming decoding
(espnet/nets/batch_beam_search_online_sim.py), on the same machinery at one utterance: the scorers see the encoder
output up to a block boundary that moves on as hypotheses end or repeat.
"""
import math
from itertools import chain
from typing import Any, Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import kernels as K


class Hypothesis(NamedTuple):
    yseq: torch.Tensor
    score: float = 0.0
    scores: Dict[str, float] = dict()
    states: Dict[str, Any] = dict()

    def asdict(self) -> dict:
        return dict(yseq=self.yseq.tolist(), score=float(self.score), scores={k: float(v) for k, v in self.scores.items()})


def end_detect(ended_hyps, i, M=3, D_end=np.log(1 * np.exp(-10))):
    """e2e_asr_common.py:19-49: stop when, for each of the last M lengths, the best ended
    hypothesis of that length is worse than the overall best by more than |D_end|."""
    if len(ended_hyps) == 0:
        return False
    best = max(h["score"] for h in ended_hyps)
    count = 0
    for m in range(M):
        same = [h["score"] for h in ended_hyps if len(h["yseq"]) == i - m]
        if same and max(same) - best < D_end:
            count += 1
    return count == M


class DecoderScorer:
    """Full scorer: log p(. | prefix, x) of the attention decoder for all hypotheses at once."""

    def __init__(self, decoder):
        self.decoder = decoder

    def batch_score(self, yseqs: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        NH, L = yseqs.shape
        T, D = x.shape
        mem = x.unsqueeze(0).expand(NH, T, D).contiguous()
        hl = torch.full((NH,), T, dtype=torch.int64)
        yl = torch.full((NH,), L, dtype=torch.int64)
        logits, _ = self.decoder(mem, hl, yseqs, yl)
        last = logits[:, -1, :].contiguous()
        lp = torch.empty_like(last)
        K.log_softmax(last, lp, NH, last.shape[1])
        return lp


class LengthBonus:
    """Full scorer: +1 for every label (scorers/length_bonus.py:9-61), weighted by `penalty`."""

    @staticmethod
    def final_score(state) -> float:
        return 0.0


class CTCPrefixScorer:
    """Partial scorer (scorers/ctc.py:9-71 + ctc_prefix_score.py CTCPrefixScore).  State per
    hypothesis: (prefix log-prob psi of the hypothesis, its (T, 2) forward variables)."""

    def __init__(self, ctc, eos: int, blank: int = 0):
        self.ctc, self.eos, self.blank = ctc, eos, blank
        self.lp = None

    def init_state(self, x: torch.Tensor):
        self.lp = self.ctc.log_softmax(x.unsqueeze(0))[0].contiguous()
        return 0.0, K.ctc_prefix_init(self.lp, self.blank)

    def batch_score_partial(self, yseqs: torch.Tensor, ids: torch.Tensor, states: List[Any]):
        """ids (NH, C) labels per hypothesis -> (score deltas (NH, C), log_psi (NH, C), r (NH, C, T, 2))."""
        NH = yseqs.shape[0]
        dev = self.lp.device
        r_prev = torch.stack([s[1] for s in states]).contiguous()
        prev = torch.tensor([s[0] for s in states], dtype=torch.float32, device=dev)
        last = yseqs[:, -1].to(dev).contiguous()
        psi, r_new = K.ctc_prefix_score(self.lp, r_prev, last, yseqs.shape[1] - 1, ids.to(dev).contiguous(),
                                        self.blank, self.eos)
        return psi - prev[:, None], psi, r_new

    @staticmethod
    def final_score(state) -> float:
        return 0.0


class BeamSearch:
    def __init__(self, scorers: Dict[str, Any], weights: Dict[str, float], beam_size: int, vocab_size: int,
                 sos: int, eos: int, token_list: Optional[List[str]] = None, pre_beam_ratio: float = 1.5,
                 pre_beam_score_key: Optional[str] = "full"):
        self.weights = weights
        self.full_scorers, self.part_scorers = {}, {}
        for k, v in scorers.items():
            if v is None or weights.get(k, 0) == 0:
                continue
            if k == "ctc":
                self.part_scorers[k] = v
            else:
                self.full_scorers[k] = v
        self.sos, self.eos = sos, eos
        self.token_list = token_list
        self.beam_size = beam_size
        self.n_vocab = vocab_size
        self.pre_beam_size = int(pre_beam_ratio * beam_size)
        self.pre_beam_score_key = pre_beam_score_key
        self.do_pre_beam = (pre_beam_score_key is not None and self.pre_beam_size < self.n_vocab
                            and len(self.part_scorers) > 0)

    def init_hyp(self, x: torch.Tensor) -> List[Hypothesis]:
        states = {k: (d.init_state(x) if hasattr(d, "init_state") else None)
                  for k, d in chain(self.full_scorers.items(), self.part_scorers.items())}
        return [Hypothesis(yseq=torch.tensor([self.sos], dtype=torch.int64), score=0.0,
                           scores={k: 0.0 for k in chain(self.full_scorers, self.part_scorers)}, states=states)]

    def search(self, running: List[Hypothesis], x: torch.Tensor) -> List[Hypothesis]:
        NH, V, dev = len(running), self.n_vocab, x.device
        yseqs = torch.stack([h.yseq for h in running])
        full = {}
        weighted = torch.zeros(NH, V, dtype=torch.float32, device=dev)
        lm_states = None
        for k, d in self.full_scorers.items():
            if k == "decoder":
                full[k] = d.batch_score(yseqs.to(dev), x)
            elif k == "lm":  # a neural LM (lm/transformer_lm.py): the reference's list-of-states form
                full[k], lm_states = d.batch_score(yseqs, [h.states[k] for h in running], None)
            else:
                full[k] = torch.ones(NH, V, device=dev)
            weighted += self.weights[k] * full[k]
        if self.do_pre_beam:
            pre = weighted if self.pre_beam_score_key == "full" else full[self.pre_beam_score_key]
            part_ids = torch.topk(pre, self.pre_beam_size, dim=1)[1]
        else:
            part_ids = torch.arange(V, device=dev).expand(NH, V)
        part, part_states = {}, {}
        for k, d in self.part_scorers.items():
            delta, psi, r_new = d.batch_score_partial(yseqs, part_ids, [h.states[k] for h in running])
            part[k] = delta
            part_states[k] = (psi, r_new)
            weighted.scatter_add_(1, part_ids, self.weights[k] * delta)
        weighted += torch.tensor([float(h.score) for h in running], dtype=torch.float32, device=dev)[:, None]
        # per hypothesis: top `beam` over the pre-beam survivors (others masked to -inf)
        if part_ids.shape[1] < V:
            masked = torch.full_like(weighted, -float("inf"))
            masked.scatter_(1, part_ids, weighted.gather(1, part_ids))
        else:
            masked = weighted
        top_ids = torch.topk(masked, self.beam_size, dim=1)[1]
        local_ids = torch.topk(masked.gather(1, part_ids), self.beam_size, dim=1)[1] \
            if part_ids.shape[1] < V else top_ids
        # one device->host copy of everything the bookkeeping needs
        h_top, h_loc = top_ids.cpu(), local_ids.cpu()
        h_w = weighted.gather(1, top_ids).cpu()
        h_full = {k: v.gather(1, top_ids).cpu() for k, v in full.items()}
        h_part = {k: v.gather(1, local_ids).cpu() for k, v in part.items()}
        best = []
        for n, hyp in enumerate(running):
            for b in range(self.beam_size):
                j, pj = int(h_top[n, b]), int(h_loc[n, b])
                scores = {k: hyp.scores[k] + float(h_full[k][n, b]) for k in self.full_scorers}
                for k in self.part_scorers:
                    scores[k] = hyp.scores[k] + float(h_part[k][n, b])
                states = dict(hyp.states)
                if lm_states is not None:
                    states["lm"] = lm_states[n]
                for k in self.part_scorers:
                    psi, r_new = part_states[k]
                    states[k] = (float(psi[n, pj]), r_new[n, pj])
                best.append(Hypothesis(score=float(h_w[n, b]), yseq=torch.cat([hyp.yseq, torch.tensor([j])]),
                                       scores=scores, states=states))
        # stable sort (the reference sorts after each hypothesis; pooled then sorted is the same set)
        return sorted(best, key=lambda h: h.score, reverse=True)[: min(len(best), self.beam_size)]

    def post_process(self, i: int, maxlen: int, running: List[Hypothesis], ended: List[Hypothesis]):
        if i == maxlen - 1:
            running = [h._replace(yseq=torch.cat([h.yseq, torch.tensor([self.eos])])) for h in running]
        remained = []
        for hyp in running:
            if int(hyp.yseq[-1]) == self.eos:
                for k, d in chain(self.full_scorers.items(), self.part_scorers.items()):
                    s = d.final_score(hyp.states[k]) if hasattr(d, "final_score") else 0.0
                    hyp.scores[k] += s
                    hyp = hyp._replace(score=hyp.score + self.weights[k] * s)
                ended.append(hyp)
            else:
                remained.append(hyp)
        return remained

    def forward(self, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> List[Hypothesis]:
        maxlen = x.shape[0] if maxlenratio == 0 else max(1, int(maxlenratio * x.size(0)))
        running = self.init_hyp(x)
        ended: List[Hypothesis] = []
        with torch.no_grad():
            for i in range(maxlen):
                best = self.search(running, x)
                running = self.post_process(i, maxlen, best, ended)
                if maxlenratio == 0.0 and end_detect([h.asdict() for h in ended], i):
                    break
                if len(running) == 0:
                    break
        nbest = sorted(ended, key=lambda h: h.score, reverse=True)
        if not nbest:
            return [] if minlenratio < 0.1 else self.forward(x, maxlenratio, max(0.0, minlenratio - 0.1))
        return nbest


class BatchBeamSearch(BeamSearch):
    """The reference's BatchBeamSearch (espnet/nets/batch_beam_search.py:85-340 with the batch CTC scorer,
    scorers/ctc.py:88-140 + CTCPrefixScoreTH), which is what its Speech2Text runs, on the cached one-step decoder.

    Batch semantics, where they differ from BeamSearch above: the top `beam` are taken over the flattened
    (hypothesis x vocabulary) weighted scores of an utterance; the partial (CTC) scorer returns a full-size score
    row per hypothesis -- the prefix scores on the pre-beam ids, <eos> always scored (whether or not the pre-beam
    kept it), logzero = -1e10 everywhere else -- which is added with its weight; ended hypotheses get no
    final_score.  post_process / end_detect / maxlen follow BeamSearch.forward.

    forward_batch runs U utterances in lockstep: every output step is ONE decoder step over the running rows
    of all utterances (TransformerDecoder.batch_score on a DecoderCache and the memory projected once), ONE LM step
    on a second DecoderCache when scorer "lm" is present (TransformerLM.batch_score), ONE
    esp_ctc_prefix_score_batch launch and ONE device->host copy (parent row, token and scores of the U x beam
    selected entries); the host keeps the token sequences and decides what ended.  Each utterance has its own
    maxlen and end_detect, finishes on its own, and its rows are then dropped.  Rows stay sorted by utterance.
    """

    LOGZERO = -10000000000.0

    def forward(self, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> List[Hypothesis]:
        return self.forward_batch(x.unsqueeze(0), [x.shape[0]], maxlenratio, minlenratio)[0]

    def _score_rows(self, i, ys, utt, utt_dev, dec, mem, cache, lm, lm_cache, ctc, lp, tlen, r, s_prev, score):
        """Output step i of the N running rows ys (host (N, i + 1); utt / utt_dev: their utterances): every scorer's
        scores and their weighted sum plus the rows' own scores.  -> (weighted (N, V), full {name: (N, V)},
        part (N, V) CTC score deltas, psi_full (N, V), r_new (N, C, Tmax, 2), cands (N, C), cache, lm_cache); the
        CTC entries are None without a CTC scorer."""
        N, V, dev = ys.shape[0], self.n_vocab, score.device
        # full scorers
        full = {}
        weighted = torch.zeros(N, V, dtype=torch.float32, device=dev)
        for k in self.full_scorers:
            if k == "decoder":
                full[k], cache = dec.batch_score(torch.from_numpy(ys), cache, (mem, utt))
            elif k == "lm":
                full[k], lm_cache = lm.batch_score(torch.from_numpy(ys), lm_cache, None)
            else:
                full[k] = torch.ones(N, V, dtype=torch.float32, device=dev)
            weighted += self.weights[k] * full[k]
        # partial scorer on the pre-beam ids (+ <eos>), as a full-size score row
        part = psi_full = r_new = cands = None
        if ctc is not None:
            if self.do_pre_beam:
                pre = weighted if self.pre_beam_score_key == "full" else full[self.pre_beam_score_key]
                cands = torch.cat([torch.topk(pre, self.pre_beam_size, dim=1)[1],
                                   torch.full((N, 1), self.eos, dtype=torch.int64, device=dev)], 1).contiguous()
            else:
                cands = torch.arange(V, device=dev).expand(N, V).contiguous()
            last = K.h2d(torch.from_numpy(np.ascontiguousarray(ys[:, -1])), dev)
            psi, r_new = K.ctc_prefix_score_batch(lp, tlen, utt_dev, r, last, i, cands, ctc.blank, ctc.eos)
            psi_full = torch.full((N, V), self.LOGZERO, dtype=torch.float32, device=dev).scatter_(1, cands, psi)
            part = psi_full - s_prev[:, None]
            weighted += self.weights["ctc"] * part
        weighted += score[:, None]
        return weighted, full, part, psi_full, r_new, cands, cache, lm_cache

    @staticmethod
    def _ctc_select(r_new, psi_full, cands, parent, tok):
        """The CTC states (r, s_prev) of the selected (parent row, token) entries: the candidate slot of the chosen
        token (a duplicate <eos> slot holds the same state; a token outside the candidates can only be chosen at
        logzero: slot 0, as the reference does)."""
        N, V = psi_full.shape
        slotmap = torch.full((N, V), -1, dtype=torch.int64, device=psi_full.device)
        slotmap.scatter_(1, cands, torch.arange(cands.shape[1], device=psi_full.device).expand_as(cands))
        return r_new[parent, slotmap[parent, tok].clamp_(min=0)].contiguous(), psi_full[parent, tok]

    def forward_batch(self, xs_pad: torch.Tensor, xlens, maxlenratio: float = 0.0,
                      minlenratio: float = 0.0) -> List[List[Hypothesis]]:
        """xs_pad (U, Tmax, D) encoder outputs, xlens (U,) their lengths -> one n-best list per utterance."""
        U, Tmax, _ = xs_pad.shape
        dev, V, beam = xs_pad.device, self.n_vocab, self.beam_size
        xlens = [int(t) for t in xlens]
        assert len(xlens) == U and all(1 <= t <= Tmax for t in xlens), (xlens, xs_pad.shape)
        maxlen = [t if maxlenratio == 0 else max(1, int(maxlenratio * t)) for t in xlens]
        dec = self.full_scorers["decoder"].decoder if "decoder" in self.full_scorers else None
        ctc = self.part_scorers.get("ctc")
        names = list(chain(self.full_scorers, self.part_scorers))
        ended: List[List[Hypothesis]] = [[] for _ in range(U)]
        self.finish_step = [-1] * U  # the output step at which each utterance's search ended
        self.steps = 0
        with torch.no_grad():
            xs_pad = xs_pad.to(torch.float32).contiguous()
            mem = dec.prepare_memory(xs_pad, xlens) if dec is not None else None
            cache = dec.init_cache(U) if dec is not None else None
            lm = self.full_scorers.get("lm")
            lm_cache = None  # the LM's own K/V cache, reordered and pruned with the decoder's
            lp = tlen = r = s_prev = None
            if ctc is not None:
                lp = ctc.ctc.log_softmax(xs_pad).contiguous()
                tlen = K.h2d(torch.tensor(xlens, dtype=torch.int32), dev)
                r = torch.stack([K.ctc_prefix_init(lp[u], ctc.blank) for u in range(U)])  # (N, Tmax, 2)
                s_prev = torch.zeros(U, dtype=torch.float32, device=dev)
            # running rows, sorted by utterance: host token sequences / utterance ids, device scores
            ys = np.full((U, 1), self.sos, dtype=np.int64)
            utt = np.arange(U, dtype=np.int32)
            score = torch.zeros(U, dtype=torch.float32, device=dev)
            scores = {k: torch.zeros(U, dtype=torch.float32, device=dev) for k in names}
            for i in range(max(maxlen)):
                N = ys.shape[0]
                active, counts = np.unique(utt, return_counts=True)  # ascending: the row order
                A = len(active)
                start = np.concatenate([[0], np.cumsum(counts)[:-1]])
                utt_dev = K.h2d(torch.from_numpy(utt), dev)
                weighted, full, part, psi_full, r_new, cands, cache, lm_cache = self._score_rows(
                    i, ys, utt, utt_dev, dec, mem, cache, lm, lm_cache, ctc, lp, tlen, r, s_prev, score)
                # top `beam` of every utterance over its flattened (row x vocabulary) scores
                slot = np.concatenate([a * beam + np.arange(c) for a, c in enumerate(counts)])
                padded = torch.full((A * beam, V), -float("inf"), dtype=torch.float32, device=dev)
                padded[K.h2d(torch.from_numpy(slot), dev)] = weighted
                vals, flat = padded.view(A, beam * V).topk(beam, dim=1)
                parent = (torch.div(flat, V, rounding_mode="floor")
                          + K.h2d(torch.from_numpy(start), dev)[:, None]).reshape(-1)
                tok = (flat % V).reshape(-1)
                new_scores = {k: scores[k][parent] + (part if k == "ctc" else full[k])[parent, tok] for k in names}
                # the one device->host copy of the step
                host = torch.stack([parent.double(), tok.double(), vals.reshape(-1).double()]
                                   + [new_scores[k].double() for k in names]).cpu().numpy()
                self.steps += 1
                h_parent, h_tok = host[0].astype(np.int64), host[1].astype(np.int64)
                keep = []
                for a, u in enumerate(active):
                    remained = 0
                    for e in range(a * beam, (a + 1) * beam):
                        y = list(ys[h_parent[e]]) + [int(h_tok[e])]
                        if i == maxlen[u] - 1:
                            y.append(self.eos)
                        if y[-1] == self.eos:
                            ended[u].append(Hypothesis(yseq=torch.tensor(y, dtype=torch.int64), score=float(host[2, e]),
                                                       scores={k: float(host[3 + j, e]) for j, k in enumerate(names)},
                                                       states={}))
                        else:
                            keep.append(e)
                            remained += 1
                    if (maxlenratio == 0.0 and end_detect([h.asdict() for h in ended[u]], i)) or remained == 0:
                        keep = keep[: len(keep) - remained]
                        self.finish_step[u] = i
                if not keep:
                    break
                keep = np.asarray(keep, dtype=np.int64)
                ys = np.concatenate([ys[h_parent[keep]], h_tok[keep, None]], 1)
                utt = np.ascontiguousarray(active[keep // beam].astype(np.int32))
                keep_dev = K.h2d(torch.from_numpy(keep), dev)
                parent, tok = parent[keep_dev], tok[keep_dev]
                score = vals.reshape(-1)[keep_dev]
                scores = {k: v[keep_dev] for k, v in new_scores.items()}
                if cache is not None:
                    cache.reorder(parent)
                if lm_cache is not None:
                    lm_cache.reorder(parent)
                if ctc is not None:
                    r, s_prev = self._ctc_select(r_new, psi_full, cands, parent, tok)
        return [sorted(e, key=lambda h: h.score, reverse=True) for e in ended]


def first_window(T: int, block_size, hop_size, look_ahead) -> int:
    """Frames the block-synchronous search sees at first: block_size - look_ahead, or all T when a size is unset or
    zero or that window already covers the utterance."""
    if block_size and hop_size and look_ahead:
        return min(int(block_size - look_ahead), T)
    return T


def next_window(cur: int, T: int, hop_size, look_ahead) -> int:
    """The window after `cur` frames: one hop further while a hop and the look-ahead still fit before T, else T."""
    if hop_size and cur + int(hop_size) + int(look_ahead) < T:
        return cur + int(hop_size)
    return T


class _Rows:
    """The token matrix of one search step's selected entries.  An ended hypothesis refers to its row as
    (offset, length) into the flattened matrix, as the reference's hypotheses hold views of the step's yseq tensor:
    when the last step appends <eos> to that tensor in place, the views made before then read shifted tokens, and so
    do these."""

    def __init__(self, mat: np.ndarray):
        self.mat = mat

    def view(self, b: int):
        L = self.mat.shape[1]
        return self, b * L, L

    def append_eos(self, eos: int):
        self.mat = np.concatenate([self.mat, np.full((self.mat.shape[0], 1), eos, dtype=self.mat.dtype)], 1)


class BatchBeamSearchOnlineSim(BatchBeamSearch):
    """The reference's BatchBeamSearchOnlineSim (espnet/nets/batch_beam_search_online_sim.py:96-270): the
    blockwise-synchronous beam search of Tsunoo et al. (arXiv:2006.14941), simulated on the encoder output of the
    whole utterance.  The decoder and the CTC scorer see the first `window` frames only; the search moves to the next
    block when a hypothesis of the new beam ends or starts repeating a token, discards that step, and (from the third
    output step on, never twice in a row) also takes back the step before it.  With a size unset the window is the
    whole utterance and the search is BatchBeamSearch with this class's ending rules.

    The CTC scorer grows with the window (CTCPrefixScoreTH.extend_prob / extend_state, which the reference's
    CTCPrefixScorer does not forward to as shipped).

    On the device machinery of forward_batch at U = 1.  The CTC log-softmax and the memory's K/V projection are
    computed once over all frames; the window is a length: the key length of the source attention
    (PreparedMemory.set_window) and tlen of the CTC kernel.  A new window grows the running CTC states in place
    (esp_ctc_prefix_extend).  The self-attention cache reorders into a second buffer (DecoderCache.reorder_keep), so
    the step before the last selection can be restored (rollback) together with the host's token matrix and the score
    and CTC state tensors of then, which are kept by reference; cached K/V of earlier positions stay as they were
    computed under the shorter window, like the reference's cached layer outputs.

    block_trace: one (frames in the window, running hypotheses, prefix length) per block; rollbacks: steps taken back.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if "lm" in self.full_scorers:
            raise ValueError("BatchBeamSearchOnlineSim: scorer 'lm' is not supported (the LM cache has no rollback)")
        self.block_size = self.hop_size = self.look_ahead = None
        self.block_trace: List[tuple] = []
        self.rollbacks = 0

    def set_block_size(self, block_size: int):
        self.block_size = block_size

    def set_hop_size(self, hop_size: int):
        self.hop_size = hop_size

    def set_look_ahead(self, look_ahead: int):
        self.look_ahead = look_ahead

    def forward_batch(self, *args, **kwargs):
        raise ValueError("BatchBeamSearchOnlineSim searches one utterance at a time (forward)")

    def forward(self, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> List[Hypothesis]:
        T, dev, V, beam = x.shape[0], x.device, self.n_vocab, self.beam_size
        cur_end = first_window(T, self.block_size, self.hop_size, self.look_ahead)
        maxlen = T if maxlenratio == 0 else max(1, int(maxlenratio * T))
        dec = self.full_scorers["decoder"].decoder if "decoder" in self.full_scorers else None
        ctc = self.part_scorers.get("ctc")
        names = list(chain(self.full_scorers, self.part_scorers))
        self.block_trace, self.rollbacks, self.steps = [], 0, 0
        ended = []  # (score, scores, rows view), in the reference's order of appending
        with torch.no_grad():
            xs = x.to(torch.float32).contiguous().unsqueeze(0)
            mem = dec.prepare_memory(xs, [T]) if dec is not None else None
            cache = dec.init_cache(1) if dec is not None else None
            lp = tlen = None
            # running rows: host token matrix, device scores, CTC states valid for the first `tv` frames
            run = dict(ys=np.full((1, 1), self.sos, dtype=np.int64), score=torch.zeros(1, dtype=torch.float32, device=dev),
                       scores={k: torch.zeros(1, dtype=torch.float32, device=dev) for k in names}, r=None, s_prev=None,
                       tv=T)
            if ctc is not None:
                lp = ctc.ctc.log_softmax(xs).contiguous()
                run["r"] = K.ctc_prefix_init(lp[0], ctc.blank).unsqueeze(0)  # the blank path over all frames
                run["s_prev"] = torch.zeros(1, dtype=torch.float32, device=dev)
            prev = None  # the running rows of one step ago (cache: DecoderCache's kept buffer)
            prev_repeat = False
            i = 0
            decoding = True
            while decoding and i < maxlen:
                move = False
                # extend: the scorers see `cur_end` frames from here on
                N = run["ys"].shape[0]
                self.block_trace.append((cur_end, N, run["ys"].shape[1]))
                utt = np.zeros(N, dtype=np.int32)
                utt_dev = torch.zeros(N, dtype=torch.int32, device=dev)
                if mem is not None:
                    mem.set_window(cur_end)
                if ctc is not None:
                    tlen = K.h2d(torch.tensor([cur_end], dtype=torch.int32), dev)
                    if run["tv"] < cur_end:
                        K.ctc_prefix_extend(lp, utt_dev, run["r"], run["tv"], cur_end, ctc.blank)
                    run["tv"] = cur_end
                while i < maxlen:
                    ys = run["ys"]
                    N = ys.shape[0]
                    if N != utt.shape[0]:
                        utt = np.zeros(N, dtype=np.int32)
                        utt_dev = torch.zeros(N, dtype=torch.int32, device=dev)
                    weighted, full, part, psi_full, r_new, cands, cache, _ = self._score_rows(
                        i, ys, utt, utt_dev, dec, mem, cache, None, None, ctc, lp, tlen, run["r"], run["s_prev"],
                        run["score"])
                    vals, flat = weighted.view(-1).topk(beam)
                    parent, tok = torch.div(flat, V, rounding_mode="floor"), flat % V
                    new_scores = {k: run["scores"][k][parent] + (part if k == "ctc" else full[k])[parent, tok]
                                  for k in names}
                    # the one device->host copy of the step
                    host = torch.stack([parent.double(), tok.double(), vals.double()]
                                       + [new_scores[k].double() for k in names]).cpu().numpy()
                    self.steps += 1
                    h_parent, h_tok = host[0].astype(np.int64), host[1].astype(np.int64)
                    rows = _Rows(np.concatenate([ys[h_parent], h_tok[:, None]], 1))

                    def entry(b):
                        return float(host[2, b]), {k: float(host[3 + j, b]) for j, k in enumerate(names)}, rows.view(b)

                    def post_process():
                        """Ended entries of the step join `ended`; -> the entries that go on."""
                        if i == maxlen - 1:
                            rows.append_eos(self.eos)
                        is_eos = rows.mat[:, -1] == self.eos
                        ended.extend(entry(b) for b in np.nonzero(is_eos)[0])
                        return np.nonzero(~is_eos)[0]

                    if i == maxlen - 1:
                        keep = post_process()
                    local_ended = []
                    for b in range(beam):
                        if rows.mat[b, -1] == self.eos:
                            local_ended.append(entry(b))
                        elif not prev_repeat and rows.mat[b, -1] in rows.mat[b, :-1] and cur_end < T:
                            move = True
                            prev_repeat = True
                    if maxlenratio == 0.0 and end_detect(
                            [dict(score=s, yseq=range(v[2])) for s, _, v in local_ended], i):
                        decoding = False
                        break
                    if local_ended and cur_end < T:
                        move = True
                    if move:
                        cur_end = next_window(cur_end, T, self.hop_size, self.look_ahead)
                        if i > 1 and prev is not None:  # take back the step before this one as well
                            run, prev = prev, None
                            i -= 1
                            self.rollbacks += 1
                            if cache is not None:
                                cache.rollback()
                        elif cache is not None:
                            cache.len -= 1  # this step's position is computed again under the new window
                        break
                    prev_repeat = False
                    prev = run
                    keep = post_process()
                    if cur_end >= T:
                        ended.extend(local_ended)
                    if keep.size == 0:
                        decoding = False
                        break
                    keep_dev = K.h2d(torch.from_numpy(keep), dev)
                    parent, tok = parent[keep_dev], tok[keep_dev]
                    run = dict(ys=np.ascontiguousarray(rows.mat[keep]), score=vals[keep_dev],
                               scores={k: v[keep_dev] for k, v in new_scores.items()}, r=None, s_prev=None, tv=cur_end)
                    if cache is not None:
                        cache.reorder_keep(parent)
                    if ctc is not None:
                        run["r"], run["s_prev"] = self._ctc_select(r_new, psi_full, cands, parent, tok)
                    i += 1
        nbest = []
        for s, sc, (rows, off, L) in sorted(ended, key=lambda e: e[0], reverse=True):
            nbest.append(Hypothesis(yseq=torch.from_numpy(rows.mat.reshape(-1)[off:off + L].copy()), score=s, scores=sc,
                                    states={}))
        if not nbest:
            return [] if minlenratio < 0.1 else self.forward(x, maxlenratio, max(0.0, minlenratio - 0.1))
        return nbest
