"""The RNN-Transducer model on the MI355X against the reference's own ESPnetASRModel with a joint network
(tests/golden/transducer_model_<case>.npz, written by make_transducer_golden.py in fp32 and in fp64).

Tiny models (D = 64, 2 blocks, V = 32; LSTM 1 and 2 layers of 48 units; joint space 40), Transformer and Conformer
encoders, ctc_weight 0.0 and 0.3, B = 3 with ragged lengths and a one-token target.  Gates: the losses by
tests.helpers.loss_gate's rule, |ours - ref64| <= max(1e-4, 2 |ref32 - ref64|); every parameter's whole gradient
(the encoder's included: the feature-side gradient reaches it through the joint network's lin_enc) against the fp64
restatement of tests/transducer_helpers.py, which the generator asserted equal to the reference's fp64 step: the L2
norm (relative, floor 1e-4) and the largest element error relative to the tensor's fp64 maximum (floor 1e-5), each
within 2 x the reference fp32 run's own figure from the fixture; a gradient whose fp64 maximum is below 1e-6 of the
model's largest counts as zero and must stay below 1e-5 of that scale.
"""
import functools

import numpy as np
import pytest
import torch

from tests import transducer_helpers as TH
from tests.helpers import golden, loss_gate

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _truth(name):
    return TH.restated_grads(name)


def _model(name, dev, **kw):
    seed, cfg, tc = TH.case_cfg(name)
    model = TH.build_transducer(cfg, tc, dev, **kw)
    TH.load_params(model, TH.transducer_params(cfg, tc, seed))
    return model.train(), cfg, seed


def _batch(cfg, seed, dev):
    speech, slen, text, tlen = TH.batch(cfg, seed)
    return speech.to(dev), slen, text.clone(), tlen


def _check_step(name, model, loss, stats):
    g = golden(f"transducer_model_{name}")
    ok, info = loss_gate(float(loss), g)
    assert ok, info
    assert list(stats) == g["stat_keys"].tolist()
    assert [stats[k] is None for k in stats] == g["stat_none"].tolist()
    for k in ("loss_transducer", "loss_ctc"):
        if k + "_f64" in g:
            ok, info = loss_gate(float(stats[k]), g, key=k)
            assert ok, info
    assert torch.equal(stats["loss"], loss.detach())
    _, _, G = _truth(name)
    names = [n for n, _ in model.named_parameters()]
    assert set(names) == set(G), set(names) ^ set(G)
    scale = max(float(g["gmax_f64/" + n]) for n in names)
    bad, worst = [], 0.0
    for n, p in model.named_parameters():
        got, r64 = p.grad.detach().double().cpu(), G[n]
        gm = float(g["gmax_f64/" + n])
        if gm < 1e-6 * scale:
            if float(got.abs().max()) > 1e-5 * scale:
                bad.append((n, "nonzero", float(got.abs().max())))
            continue
        e, r = float((got - r64).abs().max()) / gm, float(g["emax_f32/" + n]) / gm
        gn64 = float(g["gn_f64/" + n])
        en, rn = abs(float(got.norm()) - gn64) / gn64, abs(float(g["gn_f32/" + n]) - gn64) / gn64
        worst = max(worst, e)
        if e > max(2 * r, 1e-5):
            bad.append((n, "element", e, r))
        if en > max(2 * rn, 1e-4):
            bad.append((n, "norm", en, rn))
    print(f"{name}: worst element error / max {worst:.3e} over {len(names)} tensors")
    assert not bad, bad


@pytest.mark.parametrize("name", list(TH.CASES))
def test_training_step_against_the_reference(dev, name):
    model, cfg, seed = _model(name, dev)
    hooked = []
    model._grad_hook = hooked.append
    speech, slen, text, tlen = _batch(cfg, seed, dev)
    model.flat.zero_grad()
    loss, stats, weight = model(speech, slen, text, tlen)
    loss.backward()
    torch.cuda.synchronize()
    assert int(weight) == TH.B
    _check_step(name, model, loss, stats)
    # the module-done hook sees the decoder, the joint network and (when present) ctc
    assert any(m is model.decoder for m in hooked) and any(m is model.joint_network for m in hooked)
    assert any(m is model.ctc for m in hooked) == (model.ctc is not None)
    done = {id(p) for m in hooked for p in m.parameters()}  # (the encoder's modules report through its own hook)
    heads = [m for m in (model.decoder, model.joint_network, model.ctc) if m is not None]
    assert done == {id(p) for m in heads for p in m.parameters()}


@pytest.mark.parametrize("name", ["tf_l2_ctc", "cf_l2"])
def test_length_buckets_stay_within_the_gates(dev, name):
    model, cfg, seed = _model(name, dev)
    speech, slen, text, tlen = _batch(cfg, seed, dev)
    pad = torch.zeros(TH.B, 68, speech.shape[2], device=dev)
    pad[:, : speech.shape[1]] = speech
    model.flat.zero_grad()
    prep = model.prepare(slen, text, tlen, 68, speech.shape[2], t_bucket=68, u_bucket=9).to_device(dev)
    assert prep.U1 == 10 and prep.T == 68
    loss, stats, _ = model.forward_prepared(pad, prep)
    loss.backward()
    torch.cuda.synchronize()
    _check_step(name, model, loss, stats)


@pytest.mark.parametrize("name", list(TH.CASES))
def test_eval_stats_are_the_reference_s(dev, name):
    g = golden(f"transducer_model_{name}")
    model, cfg, seed = _model(name, dev)
    model.eval()
    speech, slen, text, tlen = _batch(cfg, seed, dev)
    with torch.no_grad():
        loss, stats, _ = model(speech, slen, text, tlen)
    assert list(stats) == g["eval.stat_keys"].tolist()
    assert [stats[k] is None for k in stats] == g["eval.stat_none"].tolist()
    assert 0.0 <= float(stats["cer_transducer"]) and 0.0 <= float(stats["wer_transducer"])
    ok, info = loss_gate(float(loss), dict(loss_f64=g["eval.loss_f64"], loss_f32=g["eval.loss_f32"]))
    assert ok, info


def test_eval_error_rates_equal_the_recorded_ones(dev):
    """cer_transducer / wer_transducer from the eval pass's own search (beam 2, `default`, no score normalisation) on
    the decoding models and batches of tests/golden/transducer_eval.npz.  The generator kept a batch only when the
    reference's fp32 and fp64 passes agreed and no decision of the search was within 100 x their distance (asserted
    again here); the batches have equal lengths, because the padded frames of a shorter utterance are identical rows
    on which the reference's own fp32 and fp64 searches part ways (exact ties decided by rounding)."""
    g = golden("transducer_eval")
    assert len(g["models"]) >= 2
    for mname in g["models"].tolist():
        assert float(g[f"{mname}/margin"]) >= 100.0 * float(g[f"{mname}/dist"])
        cfg, tc, seed = TH.search_model_of(mname)
        model = TH.build_transducer(cfg, tc, dev)
        TH.load_params(model, TH.search_params(cfg, tc, seed))
        model.eval()
        speech, slen, text, tlen = TH.O.synthetic_batch(3, TH.SEARCH_T, cfg.enc.input_size, cfg.vocab_size,
                                                        g["lens"].tolist(), g["ulens"].tolist(),
                                                        int(g[f"{mname}/batch_seed"]))
        with torch.no_grad():
            loss, stats, _ = model(speech.to(dev), slen, text, tlen)
        for k in ("cer_transducer", "wer_transducer"):
            assert float(stats[k]) == pytest.approx(float(g[f"{mname}/{k}"]), abs=1e-6), (mname, k)
        ok, info = loss_gate(float(loss), dict(loss_f64=g[f"{mname}/loss_f64"], loss_f32=g[f"{mname}/loss_f32"]))
        assert ok, info


def _trainer(name, dev, graph):
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    model, cfg, seed = _model(name, dev)
    opt = FusedAdam(model.parameters(), model.flat, lr=1e-3)
    return Trainer(model, opt, None, TrainerOptions(grad_clip=5.0), cuda_graph=graph), model, cfg, seed


def test_three_trainer_steps_follow_the_reference(dev):
    name = "tf_l2_ctc"
    g = golden(f"transducer_model_{name}")
    tr, model, cfg, seed = _trainer(name, dev, False)
    for i in range(3):
        speech, slen, text, tlen = _batch(cfg, seed, dev)
        stats = tr.train_one_step(dict(speech=speech, speech_lengths=slen, text=text, text_lengths=tlen))
        ok, info = loss_gate(float(stats["loss"]), dict(loss_f64=g["steps.loss_f64"][i], loss_f32=g["steps.loss_f32"][i]))
        assert ok, (i, info)
        assert bool(torch.isfinite(stats["grad_norm"]).all())


@pytest.mark.parametrize("name", ["tf_l2_ctc", "cf_l2"])
def test_graph_trainer_step_is_bit_equal_to_eager(dev, name):
    te, me, cfg, seed = _trainer(name, dev, False)
    tg, mg, _, _ = _trainer(name, dev, True)
    for _ in range(2):
        speech, slen, text, tlen = _batch(cfg, seed, dev)
        le = te.train_one_step(dict(speech=speech.clone(), speech_lengths=slen, text=text.clone(), text_lengths=tlen))
        lg = tg.train_one_step(dict(speech=speech.clone(), speech_lengths=slen, text=text.clone(), text_lengths=tlen))
        assert float(le["loss"]) == float(lg["loss"])
    te.resolve_pending()
    tg.sync_host_state()
    assert len(tg._graphs) == 1
    assert torch.equal(me.flat.flat, mg.flat.flat)


def test_explicit_forward_backward_equal_autograd(dev):
    name = "cf_l1_ctc"
    model, cfg, seed = _model(name, dev)
    speech, slen, text, tlen = _batch(cfg, seed, dev)
    model.flat.zero_grad()
    prep = model.prepare(slen, text, tlen, speech.shape[1], speech.shape[2]).to_device(dev)
    loss, _, _ = model.forward_prepared(speech.clone(), prep)
    loss.backward()
    want = model.flat.grad.clone()
    model.flat.zero_grad()
    hooked = []
    loss2, stats, _, ctx = model.forward_explicit(speech.clone(), prep)
    model.backward_explicit(ctx, torch.ones(1, device=dev), hooked.append)
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), loss2) and torch.equal(want, model.flat.grad)
    assert any(m is model.joint_network for m in hooked) and list(stats)[-1] == "loss"
