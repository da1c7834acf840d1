"""E-Branchformer encoder on the MI355X against the reference's own fp32 / fp64 runs (fixtures written by
tests/golden/make_ebranchformer_golden.py; parameters from branchformer_helpers.seeded_params).  Models are built
through tasks.asr.build_model with encoder="e_branchformer".  The gates are tests/test_gpu_branchformer.py's:
losses within 1e-4 of fp64, acc within 1e-6, every gradient within max(1e-4, 2 e_ref) (e_ref the reference's own
fp32 error; tensors that are zero in exact arithmetic below 1e-5 of the scale), eval encode within 1e-4 relative,
bucketed and HIP-graph steps equal to the plain ones to 1e-6."""
import numpy as np
import pytest
import torch

from oracle import espnet_cpu as O
from tests import ebranchformer_helpers as EH
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

MAC = "ebf_small_mac_k31"


def _model(dev, conf, seed, dropout=None):
    from espnet_slurp_amd.tasks.asr import build_model
    model = build_model(EH.args_from_conf(conf, dropout=dropout), device=dev)
    EH.load_seeded(model, seed)
    return model


def _train_step(model, g, dev):
    model.train()
    loss, stats, weight = model(torch.from_numpy(g["speech"]).to(dev), torch.from_numpy(g["speech_lengths"]),
                                torch.from_numpy(g["text"]), torch.from_numpy(g["text_lengths"]))
    loss.backward()
    torch.cuda.synchronize()
    return loss, stats, weight


def _loss_gates(loss, stats, g):
    for key, got in (("loss", loss.item()), ("loss_ctc", stats["loss_ctc"].item()),
                     ("loss_att", stats["loss_att"].item())):
        print(f"EBRANCHFORMER {key} got={got!r} f64={float(g[key + '_f64'])!r} f32={float(g[key + '_f32'])!r}")
        assert abs(got - float(g[key + "_f64"])) < 1e-4, (key, got, float(g[key + "_f64"]))
    assert abs(stats["acc"].item() - float(g["acc_f64"])) < 1e-6


def _gradient_gate(model, g):
    scale = max(float(np.abs(g["grad64/" + n]).max()) for n, _ in model.named_parameters())
    bad, small = [], []
    for n, p in model.named_parameters():
        r64 = g["grad64/" + n]
        got = p.grad.detach().cpu().numpy()
        if np.abs(r64).max() < 1e-6 * scale:  # zero in exact arithmetic: fp32 noise on both sides
            small.append(n)
            assert np.abs(got).max() < 1e-5 * scale, n
            continue
        e_gpu, e_ref = rel_err(got, r64), rel_err(g["grad/" + n], r64)
        if e_gpu > max(1e-4, 2 * e_ref):
            bad.append((n, e_gpu, e_ref))
    assert not bad, bad
    assert all(n.endswith("linear_k.bias") for n in small), small


def _vs_reference(dev, name):
    g = EH.load_fixture(name)
    conf = EH.FIXTURES[name][0]
    model = _model(dev, conf, int(g["seed"]))
    assert int(sum(p.numel() for p in model.parameters())) == int(g["num_params"])
    with EH.recorded_pos_table(g, conf, dev):  # the reference run's positional table (a host-built constant)
        loss, stats, weight = _train_step(model, g, dev)
    assert loss.shape == (1,) and weight.tolist() == [3]
    # the fixture cannot be met by a merge convolution that masks the padded frames
    assert abs(float(g["loss_masked_merge_f64"]) - float(g["loss_f64"])) > 10 * 1e-4
    _loss_gates(loss, stats, g)
    _gradient_gate(model, g)
    return model


@pytest.mark.parametrize("name", list(EH.FIXTURES))
def test_small_model_vs_reference(dev, name):
    from espnet_slurp_amd import kernels as K
    assert K.EBF_MERGE_FUSED is True
    model = _vs_reference(dev, name)
    layer = model.encoder.encoders[0]
    assert float(layer.depthwise_conv_fusion.weight.grad.abs().max()) > 0.0
    assert float(layer.depthwise_conv_fusion.bias.grad.abs().max()) > 0.0


def test_composed_merge_meets_the_same_gates(dev):
    from espnet_slurp_amd import kernels as K
    K.EBF_MERGE_FUSED = False
    try:
        _vs_reference(dev, MAC)
    finally:
        K.EBF_MERGE_FUSED = True


@pytest.mark.parametrize("name", [MAC, "ebf_small_ffn_k7_legacy"])
def test_eval_encode_and_decode(dev, name):
    g = EH.load_fixture(name)
    model = _model(dev, EH.FIXTURES[name][0], int(g["seed"]))
    model.eval()
    with torch.no_grad(), EH.recorded_pos_table(g, EH.FIXTURES[name][0], dev):
        enc, olens = model.encode(torch.from_numpy(g["speech"]).to(dev), torch.from_numpy(g["speech_lengths"]))
    assert olens.cpu().tolist() == g["enc_olens"].tolist()
    assert enc.shape == g["enc_out"].shape
    assert rel_err(enc.cpu().numpy(), g["enc_out"]) < 1e-4
    if name == MAC:  # plumbing: a hypothesis comes back
        from espnet_slurp_amd.bin.asr_inference import Speech2Text
        s2t = Speech2Text(model, beam_size=2)
        res = s2t(torch.from_numpy(g["speech"][1][: int(g["speech_lengths"][1])]))
        assert len(res) >= 1 and res[0][3].yseq[0].item() == 31 and isinstance(res[0][2], list)


def test_bucketed_gradients_equal_unpadded(dev):
    """One forward + backward on the mac_k31 batch padded to its bucket (64 frames, 8 tokens) against the batch
    itself: the loss and every parameter gradient agree to 1e-6 relative to the tensor's largest gradient
    (tests/test_gpu_buckets.py's tolerances).  T = 120 -> 128 frames: T' 29 -> 31, so tvalid cuts both windows."""
    g = EH.load_fixture(MAC)
    conf, B, T, lens, ulens, seed = EH.FIXTURES[MAC]
    grads, losses = [], []
    for buck in (None, (64, 8)):
        model = _model(dev, conf, seed)
        model.train()
        model.flat.grad.zero_()
        speech = torch.from_numpy(g["speech"]).to(dev)
        tb = ub = None
        if buck:
            tb = -(-max(lens) // buck[0]) * buck[0]
            ub = -(-max(ulens) // buck[1]) * buck[1]
            speech = torch.nn.functional.pad(speech, (0, 0, 0, tb - speech.shape[1]))
        prep = model.prepare(torch.from_numpy(g["speech_lengths"]), torch.from_numpy(g["text"]),
                             torch.from_numpy(g["text_lengths"]), speech.shape[1], 80, t_bucket=tb, u_bucket=ub)
        prep.to_device(dev)
        loss, _, _ = model.forward_prepared(speech, prep)
        loss.backward()
        losses.append(loss.item())
        grads.append({n: p.grad.clone() for n, p in model.named_parameters()})
    assert abs(losses[0] - losses[1]) <= 1e-6 * max(1.0, abs(losses[0])), losses
    assert abs(losses[0] - float(g["loss_f64"])) < 1e-4
    for n, g0 in grads[0].items():
        d = (g0 - grads[1][n]).abs().max().item()
        assert d <= 1e-6 * max(1.0, g0.abs().max().item()), (n, d)


def test_dropout_deterministic(dev):
    g = EH.load_fixture(MAC)
    conf, _, _, _, _, seed = EH.FIXTURES[MAC]
    runs = []
    for s in (7, 7, 8):
        model = _model(dev, conf, seed, dropout=0.1)
        torch.manual_seed(s)
        loss, _, _ = _train_step(model, g, dev)
        runs.append((loss.item(), model.flat.grad.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0] != runs[2][0]  # another seed: other masks
    assert abs(runs[0][0] - float(g["loss_f64"])) > 1e-3  # dropout is on
    assert bool(torch.isfinite(runs[0][1]).all())


def _trainer(dev, graph):
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    conf, _, _, _, _, seed = EH.FIXTURES[MAC]
    model = _model(dev, conf, seed)
    model.train()
    opt = FusedAdam(model.parameters(), model.flat, lr=1e-3)
    return Trainer(model, opt, WarmupLR(opt, warmup_steps=10), TrainerOptions(grad_clip=5.0), cuda_graph=graph), model


def test_graph_step_matches_eager(dev):
    """Steps captured and replayed as a HIP graph equal the eager steps (tests/test_gpu_graph.py's tolerances)."""
    te, me = _trainer(dev, False)
    tg, mg = _trainer(dev, True)

    def batch():
        speech, slen, text, tlen = O.synthetic_batch(3, 120, 80, 32, [120, 97, 64], [9, 5, 7], 12)
        return dict(speech=speech.to(dev), speech_lengths=slen, text=text, text_lengths=tlen)
    le, lg = [], []
    for _ in range(3):
        le.append(te.train_one_step(batch())["loss"].item())
        lg.append(tg.train_one_step(batch())["loss"].item())
    te.resolve_pending()
    tg.sync_host_state()
    assert len(tg._graphs) == 1
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (le, lg)
    assert torch.allclose(me.flat.flat, mg.flat.flat, rtol=0, atol=1e-6)
