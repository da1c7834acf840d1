"""ErrorCalculatorTransducer — espnet2/asr/transducer/error_calculator.py:11-170: eval-mode cer_transducer /
wer_transducer from a beam search (beam 2, `default`, no score normalisation) over every utterance of the batch."""
from __future__ import annotations

from typing import List

import torch

from ..error_calculator import edit_distance
from .beam_search_transducer import BeamSearchTransducer


class ErrorCalculatorTransducer:
    def __init__(self, decoder, joint_network, token_list: List[str], sym_space: str, sym_blank: str,
                 report_cer: bool = False, report_wer: bool = False):
        self.beam_search = BeamSearchTransducer(decoder=decoder, joint_network=joint_network, beam_size=2,
                                                search_type="default", score_norm=False)
        self.decoder = decoder
        self.token_list = token_list
        self.space = sym_space
        self.blank = sym_blank
        self.report_cer = report_cer
        self.report_wer = report_wer

    def __call__(self, encoder_out: torch.Tensor, target: torch.Tensor):
        """encoder_out (B, T, D_enc) on the device (every padded frame is searched, as the reference does); target
        (B, L) blank-padded label ids on the host."""
        pred = [self.beam_search(encoder_out[b].contiguous())[0].yseq[1:] for b in range(int(encoder_out.size(0)))]
        char_pred, char_target = self.convert_to_char(pred, target)
        cer = self.calculate_cer(char_pred, char_target) if self.report_cer else None
        wer = self.calculate_wer(char_pred, char_target) if self.report_wer else None
        return cer, wer

    def convert_to_char(self, pred, target):
        char_pred, char_target = [], []
        for i, pred_i in enumerate(pred):
            p = "".join(self.token_list[int(h)] for h in pred_i).replace(self.space, " ").replace(self.blank, "")
            t = "".join(self.token_list[int(r)] for r in target[i]).replace(self.space, " ").replace(self.blank, "")
            char_pred.append(p)
            char_target.append(t)
        return char_pred, char_target

    def calculate_cer(self, char_pred, char_target) -> float:
        d = [edit_distance(p.replace(" ", ""), t.replace(" ", "")) for p, t in zip(char_pred, char_target)]
        return float(sum(d)) / sum(len(t.replace(" ", "")) for t in char_target)

    def calculate_wer(self, char_pred, char_target) -> float:
        d = [edit_distance(p.split(), t.split()) for p, t in zip(char_pred, char_target)]
        return float(sum(d)) / sum(len(t.split()) for t in char_target)
