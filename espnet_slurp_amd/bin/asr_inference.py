"""Speech2Text (espnet2/bin/asr_inference.py:52-470, ASR attention/CTC path): speech -> n-best
(text, tokens, token ids, hypothesis).  Encoder in eval mode (BatchNorm running statistics,
no dropout / SpecAug) on the HIP kernels, then the joint CTC/attention BeamSearch of
asr/beam_search.py with the reference's weights: decoder 1 - ctc_weight, ctc ctc_weight,
length_bonus penalty; pre-beam on the "full" scores unless ctc_weight == 1.0.
Tokenizers: "bpe" (sentencepiece model file, as the SLURP recipes use) and "char";
ids2tokens by the model's token_list.  lm= (a TransformerLM, or an ESPnetLanguageModel whose .lm is used) adds
neural-LM shallow fusion: scorer "lm" with weight lm_weight in the same weighted sum (and so in the "full" pre-beam
key), as the reference's Speech2Text does with lm_train_config / lm_file / lm_weight (build the LM with
tasks/lm.build_model and load_state_dict).  Word LM / n-gram / chunk-by-chunk encoding (the encoders' forward_infer)
are out of scope.

A transducer model (asr_model.use_transducer_decoder) is searched by BeamSearchTransducer(decoder, joint_network,
beam_size, **transducer_conf) (asr/transducer/beam_search_transducer.py: greedy at beam_size <= 1, else `default`);
the results hold yseq[1:] (a transducer hypothesis has no trailing <eos>).  batch_search, streaming, an LM and
decode_batch raise ValueError with such a model.

batch_search=True runs the reference Speech2Text's own search instead, BatchBeamSearch (top `beam` over the
flattened hypothesis x vocabulary scores, <eos> always CTC-scored), on the cached one-step decoder: the
memory's source-attention K/V are projected once per utterance and every output step computes the newest
position only.  decode_batch(speeches) encodes several utterances as one padded batch and searches them in
lockstep (BatchBeamSearch.forward_batch).  The default stays the plain search.

streaming=True is the reference's `--streaming true`: the search is BatchBeamSearchOnlineSim, the block-synchronous
beam search simulated on the whole utterance's encoder output, with batch_search's scorers and weights.  Its block /
hop / look-ahead sizes are the encoder's (a contextual block Transformer encoder has all three; the reference reads
them from the training YAML); with any of them missing or zero they stay unset and the whole utterance is one window.
No LM and no decode_batch in this mode.
"""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ..asr.beam_search import (BatchBeamSearch, BatchBeamSearchOnlineSim, BeamSearch, CTCPrefixScorer, DecoderScorer,
                               Hypothesis, LengthBonus)


class CharTokenizer:
    def __init__(self, space_symbol: str = "<space>"):
        self.space_symbol = space_symbol

    def tokens2text(self, tokens):
        return "".join(tokens).replace(self.space_symbol, " ")


class SentencepiecesTokenizer:
    def __init__(self, model: str):
        import sentencepiece as spm
        self.sp = spm.SentencePieceProcessor()
        self.sp.load(str(model))

    def tokens2text(self, tokens):
        return self.sp.DecodePieces(list(tokens))


class Speech2Text:
    def __init__(self, asr_model, token_list: Optional[List[str]] = None, beam_size: int = 20,
                 ctc_weight: float = 0.5, penalty: float = 0.0, nbest: int = 1, maxlenratio: float = 0.0,
                 minlenratio: float = 0.0, token_type: Optional[str] = None, bpemodel: Optional[str] = None,
                 batch_search: bool = False, lm=None, lm_weight: float = 1.0, streaming: bool = False,
                 transducer_conf: Optional[dict] = None):
        self.transducer = bool(getattr(asr_model, "use_transducer_decoder", False))
        if self.transducer:
            for name, on in (("batch_search", batch_search), ("streaming", streaming), ("lm", lm is not None)):
                if on:
                    raise ValueError(f"Speech2Text: {name} is not served with a transducer model")
        elif transducer_conf is not None:
            raise ValueError("Speech2Text: transducer_conf needs a transducer model (joint_network)")
        if streaming and lm is not None:
            raise ValueError("Speech2Text: streaming=True does not take an LM (the streaming search has no LM rollback)")
        asr_model.eval()
        self.asr_model = asr_model
        self.device = asr_model.flat.flat.device
        self.token_list = list(token_list if token_list is not None else asr_model.token_list)
        self.maxlenratio, self.minlenratio, self.nbest = maxlenratio, minlenratio, nbest
        self.streaming = streaming
        self.tokenizer = (SentencepiecesTokenizer(bpemodel) if token_type == "bpe"
                          else CharTokenizer() if token_type == "char" else None)
        if self.transducer:
            from ..asr.transducer.beam_search_transducer import BeamSearchTransducer
            self.beam_search_transducer = BeamSearchTransducer(
                decoder=asr_model.decoder, joint_network=asr_model.joint_network, beam_size=beam_size,
                token_list=self.token_list, **(transducer_conf or {}))
            return
        decoder = asr_model.decoder
        scorers = dict(decoder=DecoderScorer(decoder) if decoder is not None else None,
                       ctc=CTCPrefixScorer(asr_model.ctc, eos=asr_model.eos, blank=asr_model.blank_id),
                       length_bonus=LengthBonus())
        weights = dict(decoder=1.0 - ctc_weight, ctc=ctc_weight, length_bonus=penalty)
        if lm is not None:
            scorers["lm"] = getattr(lm, "lm", lm).eval()
            weights["lm"] = lm_weight
        kw = dict(scorers=scorers, weights=weights, beam_size=beam_size, vocab_size=len(self.token_list),
                  sos=asr_model.sos, eos=asr_model.eos, token_list=self.token_list,
                  pre_beam_score_key=None if ctc_weight == 1.0 else "full")
        self.batch_search = batch_search
        self.batch_beam_search = BatchBeamSearch(**kw)  # decode_batch's search, and __call__'s with batch_search
        self.beam_search = self.batch_beam_search if batch_search else BeamSearch(**kw)
        if streaming:
            self.beam_search = BatchBeamSearchOnlineSim(**kw)
            sizes = [getattr(asr_model.encoder, k, None) for k in ("block_size", "hop_size", "look_ahead")]
            if all(sizes):
                self.beam_search.set_block_size(sizes[0])
                self.beam_search.set_hop_size(sizes[1])
                self.beam_search.set_look_ahead(sizes[2])

    @torch.no_grad()
    def encode(self, speech: Union[torch.Tensor, np.ndarray]) -> torch.Tensor:
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        speech = speech.unsqueeze(0).to(torch.float32).to(self.device)
        lengths = torch.tensor([speech.shape[1]], dtype=torch.int64)
        enc, _ = self.asr_model.encode(speech, lengths, sl_cpu=lengths)
        return enc[0]

    @torch.no_grad()
    def __call__(self, speech: Union[torch.Tensor, np.ndarray]) -> List[Tuple[Optional[str], List[str], List[int],
                                                                                Hypothesis]]:
        enc = self.encode(speech)
        if self.transducer:
            return self._results(self.beam_search_transducer(enc))
        return self._results(self.beam_search.forward(enc, self.maxlenratio, self.minlenratio))

    @torch.no_grad()
    def decode_batch(self, speeches: list) -> List[List[Tuple[Optional[str], List[str], List[int], Hypothesis]]]:
        """Several utterances at once: one padded-batch encode, one lockstep BatchBeamSearch.forward_batch (whatever
        batch_search says); one result list per utterance, each in __call__'s tuple form.

        The padded-batch encode follows the reference's batch behaviour at utterance ends (the encoder treats a
        shorter utterance's padding as it does in a training batch), so its encoder outputs, and with them the
        scores, are not bit-equal to single-utterance encodes."""
        if self.transducer:
            raise ValueError("Speech2Text.decode_batch: decode_batch is not served with a transducer model")
        if self.streaming:
            raise ValueError("Speech2Text.decode_batch: the streaming search takes one utterance at a time")
        sp = [torch.as_tensor(s).to(torch.float32) for s in speeches]
        lengths = torch.tensor([s.shape[0] for s in sp], dtype=torch.int64)
        pad = torch.zeros((len(sp), int(lengths.max())) + tuple(sp[0].shape[1:]), dtype=torch.float32)
        for i, s in enumerate(sp):
            pad[i, : s.shape[0]] = s
        enc, enc_lens = self.asr_model.encode(pad.to(self.device), lengths, sl_cpu=lengths)
        nbests = self.batch_beam_search.forward_batch(enc, [int(t) for t in enc_lens], self.maxlenratio, self.minlenratio)
        return [self._results(h) for h in nbests]

    def _results(self, hyps):
        hyps = hyps[: self.nbest]
        out = []
        for h in hyps:
            yseq = h.yseq[1:] if self.transducer else h.yseq[1:-1].tolist()
            token_int = [t for t in yseq if t != 0]
            token = [self.token_list[i] for i in token_int]
            text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
            out.append((text, token, token_int, h))
        return out
