"""Speech2Text for Mask-CTC (espnet2/bin/asr_inference_maskctc.py:22-145): speech -> [(text, tokens, token ids,
hypothesis)], one entry.  Encoder in eval mode on the HIP kernels, then MaskCTCInference: greedy CTC, low-confidence
tokens masked, at most n_iterations whole-sequence passes of the MLM decoder, all on the device
(asr/maskctc_model.py).  One utterance at a time; batched Mask-CTC decoding and an LM are out of scope.
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
