"""MaskCTCModel / MLMDecoder training on the MI355X against the reference's MaskCTCModel (fixtures:
tests/golden/make_maskctc_golden.py, fp32 and fp64 runs of the reference on the CPU).

Gates (the project's own): losses through tests.helpers.loss_gate; every parameter gradient as test_gpu_model.py
gates its small golden models -- relative to the fp64 gradient (tests/maskctc_helpers.restated_grads, asserted equal
to the reference's fp64 step when the fixture was written), at most max(1e-4, 2 e_ref) with e_ref the reference
fp32 run's own error; the decoder's logits at valid rows within max(2 e_ref, 1e-5) of the fp64 logits."""
import functools

import numpy as np
import pytest
import torch

from tests import maskctc_helpers as MH
from tests.helpers import golden, loss_gate, rel_err

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The fixture and the fp64 gradients of one case (computed once, shared, never modified)."""
    g = golden("maskctc_model_" + name)
    seed, cfg = MH.case_cfg(name)
    _, _, grads = MH.restated_grads(cfg, seed, g)
    return g, seed, cfg, {k: v.numpy() for k, v in grads.items()}


def _model(cfg, seed, dev, dropout=0.0):
    model = MH.build_maskctc(cfg, dev, dropout=dropout)
    MH.load_params(model, MH.maskctc_params(cfg, seed))
    return model


@pytest.mark.parametrize("name", list(MH.CASES))
def test_step_vs_reference(dev, name):
    g, seed, cfg, g64 = _reference(name)
    model = _model(cfg, seed, dev)
    model.train()
    speech, slen, text, tlen = MH.batch(cfg, seed)
    loss, stats, weight = model(speech.to(dev), slen, text, tlen, mask_draws=MH.draws_from_targets(g["ys_out"]))
    loss.backward()
    torch.cuda.synchronize()
    assert loss.shape == (1,) and weight.tolist() == [MH.B]
    assert sorted(stats) == g["stat_keys"].tolist()
    bad = []
    for key in ["loss"] + [k[:-4] for k in g if k.startswith("loss_") and k.endswith("_f64") and k != "loss_f64"]:
        ok, info = loss_gate(stats[key].item(), g, key=key)
        if not ok:
            bad.append(info)
    assert not bad, bad
    assert abs(stats["acc_mlm"].item() - float(g["acc_mlm_f64"])) < 1e-6
    scale = max(float(np.abs(v).max()) for v in g64.values())
    worst = (0.0, None)
    for n, p in model.named_parameters():
        r64, got = g64[n], p.grad.detach().cpu().numpy()
        if np.abs(r64).max() < 1e-6 * scale:  # exactly-zero gradients: fp32 noise on both sides
            assert np.abs(got).max() < 1e-5 * scale, n
            continue
        e_gpu, e_ref = rel_err(got, r64), float(g["eref/" + n])
        worst = max(worst, (e_gpu, n))
        if e_gpu > max(1e-4, 2 * e_ref):
            bad.append((n, e_gpu, e_ref))
    print(f"{name}: worst gradient error {worst}")
    assert not bad, bad


@pytest.mark.parametrize("name", ["lsm", "interctc"])
def test_decoder_logits_vs_reference(dev, name):
    g, seed, cfg, _ = _reference(name)
    model = _model(cfg, seed, dev)
    model.eval()
    logits, _ = model.decoder(torch.from_numpy(g["dec_hs"]).to(dev), torch.from_numpy(g["dec_hlens"]),
                              torch.from_numpy(g["ys_in"]), torch.tensor(MH.ULENS))
    valid = g["dec_valid"]
    err = float(np.abs(logits.cpu().double().numpy() - g["dec_logits_f64"])[valid].max())
    tol = max(2 * float(g["dec_eref"]), 1e-5)
    print(f"{name}: decoder logits err {err:.3e} e_ref {float(g['dec_eref']):.3e} tol {tol:.3e}")
    assert logits.shape == g["dec_logits_f64"].shape and err <= tol, (err, tol)


def test_eval_mode_reports_no_decoder_error_rates(dev):
    g, seed, cfg, _ = _reference("lsm")
    model = MH.build_maskctc(cfg, dev, dropout=0.0, report=True)
    MH.load_params(model, MH.maskctc_params(cfg, seed))
    model.eval()
    speech, slen, text, tlen = MH.batch(cfg, seed)
    with torch.no_grad():
        loss, stats, _ = model(speech.to(dev), slen, text, tlen, mask_draws=MH.draws_from_targets(g["ys_out"]))
    assert sorted(stats) == g["stat_keys"].tolist() and stats["cer_ctc"] is not None
    assert torch.isfinite(loss).all()


def test_dropout_is_seeded(dev):
    g, seed, cfg, _ = _reference("lsm")
    model = _model(cfg, seed, dev, dropout=0.1)
    model.train()
    speech, slen, text, tlen = MH.batch(cfg, seed)
    draws = MH.draws_from_targets(g["ys_out"])
    out = []
    for s in (5, 5, 6):
        torch.manual_seed(s)
        model.flat.grad.zero_()
        loss, _, _ = model(speech.to(dev), slen, text.clone(), tlen, mask_draws=draws)
        loss.backward()
        assert torch.isfinite(loss).all() and torch.isfinite(model.flat.grad).all()
        out.append(loss.item())
    assert out[0] == out[1] and out[0] != out[2], out
    assert abs(out[0] - float(g["loss_f64"])) > 1e-4  # the dropout is really on


def _trainer(cfg, seed, dev, graph, buckets=None):
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    model = _model(cfg, seed, dev)
    model.train()
    opt = FusedAdam(model.parameters(), model.flat, lr=1e-3)
    return Trainer(model, opt, WarmupLR(opt, warmup_steps=10), TrainerOptions(grad_clip=5.0, graph_buckets=buckets),
                   cuda_graph=graph), model


def test_trainer_eager_and_graph_replay_with_new_masks(dev):
    """Three steps: the first captures the bucket's graph, the others replay it with other utterances and other
    masks (NumPy's generator, seeded per step for both trainers).  Every replayed step's loss is the eager step's."""
    from oracle import espnet_cpu as O
    _, seed, cfg, _ = _reference("lsm")
    te, _ = _trainer(cfg, seed, dev, False)
    tg, mg = _trainer(cfg, seed, dev, True, buckets=(64, 8))
    specs = [(112, [112, 90, 71], [6, 5, 4], 21), (97, [97, 97, 97], [7, 3, 5], 22), (120, [100, 120, 77], [3, 8, 1], 23)]
    masks = []
    for i, (T, lens, ulens, s) in enumerate(specs):
        speech, slen, text, tlen = O.synthetic_batch(3, T, 80, 32, lens, ulens, s)
        losses = []
        for tr in (te, tg):
            np.random.seed(200 + i)
            b = dict(speech=speech.clone().to(dev), speech_lengths=slen, text=text.clone(), text_lengths=tlen)
            st = tr.train_one_step(b)
            losses.append(st["loss"].item())
            assert {"loss_mlm", "acc_mlm", "loss_ctc"} <= set(st) and "loss_att" not in st
        assert np.isfinite(losses).all() and abs(losses[0] - losses[1]) <= 1e-6 * max(1.0, abs(losses[0])), (i, losses)
        masks.append(losses[0])
    te.resolve_pending()
    tg.sync_host_state()
    assert len(tg._graphs) == 1 and len(set(masks)) == 3
