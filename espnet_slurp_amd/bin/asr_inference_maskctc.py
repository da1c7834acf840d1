"""Speech2Text for Mask-CTC (espnet2/bin/asr_inference_maskctc.py:22-145): speech -> [(text, tokens, token ids,
hypothesis)], one entry.  Encoder in eval mode on the HIP kernels, then MaskCTCInference: greedy CTC, low-confidence
tokens masked, at most n_iterations whole-sequence passes of the MLM decoder, all on the device
(asr/maskctc_model.py).  __call__ takes one utterance; decode_batch takes several through one padded-batch encode and
MaskCTCInference.forward_batch.  An LM is out of scope.
"""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ..asr.beam_search import Hypothesis
from ..asr.maskctc_model import MaskCTCInference, MaskCTCModel
from .asr_inference import CharTokenizer, SentencepiecesTokenizer


class Speech2Text:
    def __init__(self, asr_model: MaskCTCModel, n_iterations: int = 10, threshold_probability: float = 0.99,
                 token_type: Optional[str] = None, bpemodel: Optional[str] = None):
        if not isinstance(asr_model, MaskCTCModel):
            raise TypeError(f"asr_inference_maskctc.Speech2Text needs a MaskCTCModel, got {type(asr_model).__name__}")
        asr_model.eval()
        self.asr_model = asr_model
        self.device = asr_model.flat.flat.device
        self.token_list = list(asr_model.token_list)
        self.s2t = MaskCTCInference(asr_model=asr_model, n_iterations=n_iterations,
                                    threshold_probability=threshold_probability)
        if token_type == "bpe":
            self.tokenizer = SentencepiecesTokenizer(bpemodel) if bpemodel is not None else None
        elif token_type == "char":
            self.tokenizer = CharTokenizer()
        else:
            self.tokenizer = None

    @torch.no_grad()
    def __call__(self, speech: Union[torch.Tensor, np.ndarray]) -> List[Tuple[Optional[str], List[str], List[int],
                                                                                Hypothesis]]:
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        speech = speech.unsqueeze(0).to(torch.float32).to(self.device)
        lengths = torch.tensor([speech.shape[1]], dtype=torch.int64)
        enc, _ = self.asr_model.encode(speech, lengths, sl_cpu=lengths)
        hyp = self.s2t(enc[0])
        token_int = [t for t in hyp.yseq[1:-1].tolist() if t != 0]  # without the <mask> ends and blanks (id 0)
        token = [self.token_list[i] for i in token_int]
        text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
        return [(text, token, token_int, hyp)]

    @torch.no_grad()
    def decode_batch(self, speeches: list) -> List[List[Tuple[Optional[str], List[str], List[int], Hypothesis]]]:
        """Several utterances at once: one padded-batch encode, one MaskCTCInference.forward_batch; one result list
        per utterance, each in __call__'s form.

        The padded-batch encode follows the reference's batch behaviour at utterance ends (the encoder treats a
        shorter utterance's padding as it does in a training batch), so its encoder outputs, and with them the
        token probabilities, are not bit-equal to single-utterance encodes."""
        if len(speeches) == 0:
            raise ValueError("Speech2Text.decode_batch: an empty list of utterances")
        sp = [torch.as_tensor(s).to(torch.float32) for s in speeches]
        lengths = torch.tensor([s.shape[0] for s in sp], dtype=torch.int64)
        pad = torch.zeros((len(sp), int(lengths.max())) + tuple(sp[0].shape[1:]), dtype=torch.float32)
        for i, s in enumerate(sp):
            pad[i, : s.shape[0]] = s
        enc, enc_lens = self.asr_model.encode(pad.to(self.device), lengths, sl_cpu=lengths)
        out = []
        for hyp in self.s2t.forward_batch(enc, [int(t) for t in enc_lens]):
            token_int = [t for t in hyp.yseq[1:-1].tolist() if t != 0]
            token = [self.token_list[i] for i in token_int]
            text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
            out.append([(text, token, token_int, hyp)])
        return out
