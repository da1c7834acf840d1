"""TransformerLM / ESPnetLanguageModel on the GPU against the reference's own classes (tests/golden/lm.npz, written by
make_lm_golden.py in fp32 and in fp64).

Gate for logits and log-probabilities: the distance from the reference's fp64 result may be at most twice the
reference fp32's own distance from it, and never tighter than 1e-5 absolute (the gate of test_gpu_decoder_step.py);
both distances are printed.  LMs: A (pos_enc None, d_k 32), B (sinusoidal, d_k 16), C (d_k 64)."""
import argparse

import numpy as np
import pytest
import torch

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd.asr.decoder.transformer_decoder import DecoderCache, RowState
from tests.helpers import token_list
from tests.lm_helpers import CHECK, LM_CFGS, LMAX, PARENTS, REORDER_AFTER, V, build_lm, golden_state, history, lm_golden

pytestmark = pytest.mark.gpu


def _gate(got, g, key, what):
    want64, ref32 = g[key + "64"], g[key + "32"]
    e_ref = float(np.abs(ref32 - want64).max())
    e_got = float(np.abs(got - want64).max())
    gate = max(2 * e_ref, 1e-5)
    print(f"{what}: ours {e_got:.3e}, reference fp32 {e_ref:.3e}, gate {gate:.3e}")
    assert np.isfinite(got).all() and e_got <= gate, (what, e_got, gate)


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_forward_and_nll_match_reference(dev, tag):
    from espnet_slurp_amd.lm import ESPnetLanguageModel
    g = lm_golden()
    model = ESPnetLanguageModel(build_lm(tag, dev), V)
    text, lens = torch.tensor(g["fwd_text"]), torch.tensor(g["fwd_lens"])
    x = torch.nn.functional.pad(text, [1, 0], "constant", model.eos)
    for i, l in enumerate(lens):
        x[i, l + 1:] = 0
    logits, hidden = model.lm(x, None)
    assert hidden is None and logits.shape == (3, 8, V)
    valid = (torch.arange(8)[None, :] < (lens + 1)[:, None]).numpy()
    got = logits.cpu().numpy()
    # positions past a row's length are padding: the reference computes them too, nothing reads them
    _gate(np.where(valid[..., None], got, g[f"{tag}.fwd_logits64"]), g, f"{tag}.fwd_logits", f"{tag} forward logits")
    nll, xl = model.batchify_nll(text, lens)
    assert xl.tolist() == [8, 6, 3] and nll.shape == (3, 8)
    _gate(nll.cpu().numpy(), g, f"{tag}.nll", f"{tag} nll")
    assert float(nll.cpu()[~torch.tensor(valid)].abs().max()) == 0.0
    nll2, _ = model.batchify_nll(text, lens, batch_size=2)
    assert float((nll2 - nll).abs().max()) <= 1e-5
    with torch.no_grad():
        loss, stats, weight = model(text, lens)
    assert int(weight) == 17 and abs(float(loss) - float(g[f"{tag}.nll64"].sum()) / 17) <= 1e-4
    with pytest.raises(NotImplementedError, match="training"):
        model(text, lens)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_stepped_batch_score_matches_reference(dev, monkeypatch, tag, fused):
    """N = 5 prefixes stepped L = 1..66 on a cache of capacity 8 (it doubles to 128), rows reordered twice; rows carry
    token 0 inside (whole runs included), which every layer must hide as a key."""
    monkeypatch.setattr(K, "LM_STEP_FUSED", fused)
    g = lm_golden()
    lm, hist = build_lm(tag, dev), history()
    assert any((hist[LMAX][r, 1:-1] == 0).any() for r in range(5))
    cache, grown, got = lm.init_cache(5, capacity=8), set(), []
    for L in range(1, LMAX + 1):
        logp, cache = lm.batch_score(hist[L], cache, None)
        grown.add(cache.capacity)
        assert isinstance(cache, DecoderCache) and logp.shape == (5, V) and cache.len == L
        if L in CHECK:
            got.append(logp.cpu().numpy())
        if L in REORDER_AFTER:
            cache.reorder(PARENTS)
    assert grown == {8, 16, 32, 64, 128}, grown
    _gate(np.stack(got), g, f"{tag}.bs_logp", f"{tag} batch_score fused={fused}")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_score_on_a_prefix_with_zeros(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(K, "LM_STEP_FUSED", fused)
    lm = build_lm(tag, dev)
    prefix = torch.tensor([31, 4, 0, 7, 0])
    logp, state = lm.score(prefix, None, torch.zeros(3, 4))  # no state: the earlier positions are caught up
    assert logp.shape == (V,) and isinstance(state, DecoderCache) and state.len == 5
    _gate(logp.cpu().numpy(), lm_golden(), f"{tag}.score", f"{tag} score fused={fused}")
    st = None
    for L in range(1, 6):  # stepped: the same function of the prefix
        lp, st = lm.score(prefix[:L], st, None)
    assert float((lp - logp).abs().max()) <= 1e-5


def test_list_of_states_form_agrees_with_cache_form(dev):
    """The same kernels on the same rows, the cache only gathered another way: one fp32 rounding of a
    log-probability of magnitude < 8 (4.8e-7), as test_gpu_decoder_step.test_batch_score_forms_agree."""
    lm, hist = build_lm("A", dev), history()
    cache, states = None, [None] * 5
    for L in range(1, 9):
        logp, cache = lm.batch_score(hist[L], cache, None)
        got, states = lm.batch_score(hist[L], states, None)
        assert isinstance(states, list) and all(isinstance(s, RowState) for s in states)
        assert float((got - logp).abs().max()) <= 4.8e-7, L
        if L in REORDER_AFTER:
            cache.reorder(PARENTS)
            states = [states[p] for p in PARENTS]
    with pytest.raises(ValueError, match="mix"):
        lm.batch_score(hist[9], [None] + states[1:], None)


def test_interior_zero_raises_in_forward_and_scorer_is_eval_only(dev):
    lm = build_lm("A", dev)
    with pytest.raises(ValueError, match="token 0"):
        lm(torch.tensor([[31, 4, 0, 7, 0]]), None)
    with pytest.raises(ValueError, match="token 0"):
        lm(torch.tensor([[0, 4, 5]]), None)
    lm(torch.tensor([[31, 4, 7, 0, 0]]), None)
    lm.train()
    with pytest.raises(RuntimeError, match="inference only"):
        lm.batch_score(torch.tensor([[31]]), None, None)


def test_build_model_and_strict_load(dev):
    from espnet_slurp_amd.lm import ESPnetLanguageModel
    from espnet_slurp_amd.tasks.lm import build_model
    conf = dict(LM_CFGS["B"])
    model = build_model(argparse.Namespace(token_list=token_list(V), lm="transformer", lm_conf=conf, model_conf={},
                                           init=None), dev)
    assert isinstance(model, ESPnetLanguageModel) and model.lm.flat is not None
    assert next(model.parameters()).device.type == "cuda"
    model.load_state_dict({"lm." + k: v for k, v in golden_state("B").items()}, strict=True)
    model.eval()
    logp, _ = model.lm.score(torch.tensor([31, 4, 0, 7, 0]), None, None)
    _gate(logp.cpu().numpy(), lm_golden(), "B.score", "built + loaded B score")
