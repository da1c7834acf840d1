"""LMTask subset: the `lm` registry and build_model (espnet2/tasks/lm.py:33-46, 170-199), so the resolved LM
`config.yaml` of a recipe (`lm: transformer`, `lm_conf:`, `model_conf:`) drops in unchanged and a reference-saved
LM checkpoint loads with load_state_dict(strict=True)."""
from __future__ import annotations

import argparse

from ..lm.espnet_model import ESPnetLanguageModel
from ..lm.transformer_lm import AbsLM, TransformerLM
from ..torch_utils.initialize import initialize
from .asr import ClassChoices

lm_choices = ClassChoices("lm", dict(transformer=TransformerLM), type_check=AbsLM, default="seq_rnn")


def build_model(args: argparse.Namespace, device="cuda") -> ESPnetLanguageModel:
    """LMTask.build_model: args needs token_list (a list or a token file path), lm, lm_conf, model_conf, init."""
    if isinstance(args.token_list, str):
        with open(args.token_list, encoding="utf-8") as f:
            token_list = [line.rstrip() for line in f]
        args.token_list = list(token_list)  # "portable", as the reference does
    elif isinstance(args.token_list, (tuple, list)):
        token_list = list(args.token_list)
    else:
        raise RuntimeError("token_list must be str or list")
    vocab_size = len(token_list)
    lm_class = lm_choices.get_class(getattr(args, "lm", lm_choices.default))
    lm = lm_class(vocab_size=vocab_size, **(getattr(args, "lm_conf", None) or {}))
    model = ESPnetLanguageModel(lm=lm, vocab_size=vocab_size, **(getattr(args, "model_conf", None) or {}))
    if getattr(args, "init", None) is not None:
        initialize(model, args.init)
    model = model.to(device)
    model.flatten()
    return model
