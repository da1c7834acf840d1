"""The LM layer without a GPU: the `lm` registry, the reference's errors, and the state_dict layout of TransformerLM /
ESPnetLanguageModel against what the reference's classes produce (tests/golden/lm.npz keys_json, lm_small.pt)."""
import argparse
import os

import pytest
import torch

from tests.helpers import GOLDEN, token_list
from tests.lm_helpers import LM_CFGS, TRANSFORMER2, V, build_lm, golden_keys, golden_state


def test_lm_registry():
    from espnet_slurp_amd.lm import TransformerLM
    from espnet_slurp_amd.tasks.lm import lm_choices
    assert lm_choices.name == "lm" and lm_choices.get_class("transformer") is TransformerLM
    for name in ("seq_rnn", "nope"):
        with pytest.raises(ValueError, match="--lm must be one of"):
            lm_choices.get_class(name)


def test_unknown_pos_enc_raises():
    from espnet_slurp_amd.lm import TransformerLM
    with pytest.raises(ValueError, match="unknown pos-enc option: rel"):
        TransformerLM(V, pos_enc="rel")


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_small_state_dict_layout(tag):
    lm = build_lm(tag)  # strict load of the fixture's parameters
    got = [[k, list(v.shape)] for k, v in lm.state_dict().items()]
    assert got == golden_keys()[tag]
    for k, v in golden_state(tag).items():
        assert torch.equal(lm.state_dict()[k], v)


def test_transformer2_state_dict_layout_on_meta():
    from espnet_slurp_amd.lm import TransformerLM
    with torch.device("meta"):
        lm = TransformerLM(5000, **TRANSFORMER2)
    got = [[k, list(v.shape)] for k, v in lm.state_dict().items()]
    want = golden_keys()["transformer2"]
    assert len(want) == 1 + 4 + 16 * 16 + 2 + 2 and got == want


def test_strict_load_of_reference_checkpoint():
    from espnet_slurp_amd.lm import ESPnetLanguageModel, TransformerLM
    model = ESPnetLanguageModel(TransformerLM(V, **LM_CFGS["A"]), V)
    sd = torch.load(os.path.join(GOLDEN, "lm_small.pt"), map_location="cpu", weights_only=True)
    model.load_state_dict(sd, strict=True)
    assert model.sos == model.eos == V - 1 and model.ignore_id == 0
    for k, v in golden_state("A").items():
        assert torch.equal(model.state_dict()["lm." + k], v)


def test_build_model_args_without_device():
    """build_model's class resolution (the device part runs in tests/test_gpu_lm.py)."""
    from espnet_slurp_amd.tasks import lm as T
    args = argparse.Namespace(token_list=token_list(V), lm="seq_rnn", lm_conf={}, model_conf={})
    with pytest.raises(ValueError, match="--lm must be one of"):
        T.build_model(args, device="cpu")
    with pytest.raises(RuntimeError, match="token_list must be str or list"):
        T.build_model(argparse.Namespace(token_list=None, lm="transformer", lm_conf={}, model_conf={}), device="cpu")
