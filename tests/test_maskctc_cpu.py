"""Mask-CTC without a GPU: registries, the state_dict layout against the reference's recorded keys, mask_uniform
parity under NumPy seeds (fixtures: tests/golden/make_maskctc_golden.py), the stats keys and the unsupported
calls."""
import numpy as np
import pytest
import torch

from tests import maskctc_helpers as MH
from tests.helpers import golden, small_cfg


def _model(name="lsm", **kw):
    _, cfg = MH.case_cfg(name)
    return cfg, MH.build_maskctc(cfg, torch.device("cpu"), **kw)


def test_registry_resolves_maskctc_and_mlm():
    from espnet_slurp_amd.asr.decoder.mlm_decoder import MLMDecoder
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCModel
    from espnet_slurp_amd.tasks import asr
    assert asr.model_choices.get_class("maskctc") is MaskCTCModel
    assert asr.decoder_choices.get_class("mlm") is MLMDecoder
    assert asr.model_choices.get_class("espnet").__name__ == "ESPnetASRModel"
    with pytest.raises(ValueError):
        asr.decoder_choices.get_class("mlm2")


def test_state_dict_matches_reference_keys():
    g = golden("maskctc_meta")
    cfg, model = _model()
    want = {k: tuple(int(v) for v in s if v >= 0) for k, s in zip(g["model_keys"].tolist(), g["model_shapes"])}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    dec = {k: tuple(v.shape) for k, v in model.decoder.state_dict().items()}
    assert dec == {k[len("decoder."):]: s for k, s in want.items() if k.startswith("decoder.")}
    V1 = cfg.vocab_size + 1
    assert dec["embed.0.weight"] == (V1, 64) and dec["output_layer.weight"] == (V1, 64)
    assert dec["output_layer.bias"] == (V1,)
    assert {k.split(".")[0] for k in dec} == {"embed", "decoders", "after_norm", "output_layer"}
    assert model.vocab_size == int(g["vocab_size"]) and model.mask_token == int(g["mask_token"])
    assert model.eos == int(g["eos"]) and model.token_list[-1] == str(g["token_last"]) == "<mask>"
    assert model.ctc.ctc_lo.weight.shape[0] == cfg.vocab_size  # the CTC keeps the unextended vocabulary


def test_self_attention_causal_flags():
    from espnet_slurp_amd.asr.decoder.transformer_decoder import TransformerDecoder
    _, model = _model()
    assert [l.causal for l in model.decoder.decoders] == [False, False]
    plain = TransformerDecoder(vocab_size=32, encoder_output_size=64, linear_units=128, num_blocks=2)
    assert [l.causal for l in plain.decoders] == [True, True]


def test_unsupported_decoder_options_raise():
    from espnet_slurp_amd.asr.decoder.mlm_decoder import MLMDecoder
    for kw in (dict(input_layer="linear"), dict(normalize_before=False), dict(use_output_layer=False),
               dict(concat_after=True)):
        with pytest.raises(NotImplementedError):
            MLMDecoder(vocab_size=32, encoder_output_size=64, **kw)


@pytest.mark.parametrize("seed", [0, 5, 11])
def test_mask_uniform_matches_reference_under_numpy_seed(seed):
    from espnet_slurp_amd.asr.maskctc_model import mask_uniform
    g = golden("maskctc_meta")
    ys_pad = torch.from_numpy(g["mu_ys_pad"])
    assert (ys_pad[1] != -1).sum() == 1  # a single-token target is among them
    np.random.seed(seed)
    ys_in, ys_out = mask_uniform(ys_pad, 32, 31, -1)
    assert np.array_equal(ys_in.numpy(), g[f"mu_in_{seed}"]) and np.array_equal(ys_out.numpy(), g[f"mu_out_{seed}"])
    # the draws themselves give the same masks, and a wider (bucketed) target axis is padding only
    draws = MH.draws_from_targets(g[f"mu_out_{seed}"])
    a, b = mask_uniform(ys_pad, 32, 31, -1, draws=draws)
    assert np.array_equal(a.numpy(), g[f"mu_in_{seed}"]) and np.array_equal(b.numpy(), g[f"mu_out_{seed}"])
    a, b = mask_uniform(ys_pad, 32, 31, -1, draws=draws, width=9)
    assert a.shape == b.shape == (4, 9)
    assert np.array_equal(a[:, :6].numpy(), g[f"mu_in_{seed}"]) and np.array_equal(b[:, :6].numpy(), g[f"mu_out_{seed}"])
    assert (a[:, 6:] == 31).all() and (b[:, 6:] == -1).all()


def test_prepare_masks_seed_draws_and_bucket():
    cfg, model = _model()
    g = golden("maskctc_model_lsm")
    speech, slen, text, tlen = MH.batch(cfg, int(g["seed"]))
    np.random.seed(int(g["seed"]))  # the generator seeded the reference's step with the case's seed
    prep = model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2])
    assert np.array_equal(prep.host["ys_in"].numpy(), g["ys_in"]) and np.array_equal(prep.host["ys_out"].numpy(), g["ys_out"])
    assert prep.L == prep.Umax == max(MH.ULENS) and prep.host["ys_in_lens"].tolist() == MH.ULENS
    draws = MH.draws_from_targets(g["ys_out"])
    prep = model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2], mask_draws=draws)
    assert np.array_equal(prep.host["ys_in"].numpy(), g["ys_in"]) and np.array_equal(prep.host["ys_out"].numpy(), g["ys_out"])
    prep = model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2], u_bucket=12, mask_draws=draws)
    assert prep.L == prep.Umax == 12 and prep.host["ys_in"].shape == prep.host["ys_out"].shape == (3, 12)
    assert np.array_equal(prep.host["ys_in"][:, :9].numpy(), g["ys_in"])
    assert np.array_equal(prep.host["ys_out"][:, :9].numpy(), g["ys_out"])
    assert (prep.host["ys_in"][:, 9:] == model.eos).all() and (prep.host["ys_out"][:, 9:] == -1).all()
    assert prep.host["ys"].shape == (3, 12) and prep.host["ys_in_lens"].tolist() == MH.ULENS
    with pytest.raises(ValueError):
        model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2], mask_draws=[[0], [9], [1]])
    with pytest.raises(ValueError):
        model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2], mask_draws=draws[:2])


@pytest.mark.parametrize("name", ["lsm", "noctc", "interctc"])
def test_stats_keys_are_the_references(name):
    cfg, model = _model(name)
    g = golden("maskctc_model_" + name)
    z = torch.zeros(1)
    inter = None
    if name == "interctc":
        inter = dict(stats={f"loss_interctc_layer{i}": z for i in cfg.enc.interctc_layer_idx})
    stats = model._stats(z, torch.zeros(3), inter, detach=True)
    assert sorted(stats) == g["stat_keys"].tolist()
    assert not {"loss_att", "acc", "cer", "wer"} & set(stats)


def test_nll_not_implemented_and_decoder_type_checked():
    from espnet_slurp_amd.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCModel
    cfg, model = _model()
    z = torch.zeros(1)
    with pytest.raises(NotImplementedError):
        model.nll(z, z, z, z)
    with pytest.raises(NotImplementedError):
        model.batchify_nll(z, z, z, z)
    with pytest.raises(NotImplementedError):
        model.decoder.forward_one_step(torch.zeros(1, 1, dtype=torch.long), None, z)
    plain = TransformerDecoder(vocab_size=33, encoder_output_size=64, linear_units=128, num_blocks=1)
    with pytest.raises(TypeError):
        MaskCTCModel(vocab_size=32, token_list=model.token_list[:-1], frontend=None, specaug=None, normalize=None,
                     preencoder=None, encoder=model.encoder, postencoder=None, decoder=plain, ctc=model.ctc)
