"""Contextual block Transformer encoder on the MI355X against the reference's own fp32 / fp64 runs (fixtures written
by tests/golden/make_cbt_golden.py; parameters from branchformer_helpers.seeded_params, all dropouts 0).

Gates (those of test_gpu_branchformer.py): the encoder output within max(2 e_ref, 1e-5) absolute of the fp64 run,
e_ref the reference's own fp32 error; every gradient within max(1e-4, 2 e_ref) relative to the fp64 run's; tensors
that are zero in exact arithmetic (below 1e-6 of the largest gradient: linear_k.bias) below 1e-5 of it.
The fixtures hold the fp64 run's tensors rounded to float32 (6e-8 relative: inside both e_gpu and e_ref, two orders
below the gates' floors).

The input gradient is the feature gradient (B, T, F), which training never forms (the features are data): the tests
ask run_backward for it (dfeats=, esp_conv1_dgrad behind the subsampling's backward).  The gradient at the subsampling
output (B, T', D), the tensor the block layout is cut from, is gated the same way."""
import numpy as np
import pytest
import torch

from tests import branchformer_helpers as BH
from tests import cbt_helpers as CH
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[True, False], ids=["fused", "generic"])
def attn_fused(request, monkeypatch):
    from espnet_slurp_amd import kernels as K
    monkeypatch.setattr(K, "CBT_ATTN_FUSED", request.param)
    return request.param


def _encoder(dev, conf, seed, input_size=CH.INPUT_SIZE):
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder
    from espnet_slurp_amd.flat import FlatParams
    enc = ContextualBlockTransformerEncoder(input_size, **conf).to(dev)
    enc.attach_flat(FlatParams(enc, dev))
    BH.load_seeded(enc, seed)
    return enc


def _encoder_step(dev, enc, feats, lens, cot):
    """One explicit forward + backward; returns (output, olens, feature gradient, gradient at the subsampling
    output)."""
    from espnet_slurp_amd.blocks import Seeds
    enc.train()
    enc.flat.grad.zero_()
    hs, olens, saved = enc.run_forward(feats.to(dev), lens, Seeds(5), True)
    kept = {}
    orig = enc.embed.bwd

    def bwd(c, d, **kw):
        kept["d"] = d * c.xscale  # (the short path folds x*sqrt(D) into the subsampling's output linear)
        return orig(c, d, **kw)

    enc.embed.bwd = bwd
    try:
        dfeats = torch.full(feats.shape, float("nan"), device=dev)
        enc.run_backward(saved, cot.to(dev).contiguous(), dfeats=dfeats)
    finally:
        del enc.embed.bwd
    torch.cuda.synchronize()
    return hs.cpu(), olens, dfeats.cpu(), kept["d"].cpu().view(hs.shape)


def _grad_gate(named, g, what):
    scale = max(float(np.abs(g["grad64/" + n]).max()) for n, _ in named)
    bad, small = [], []
    for n, p in named:
        r64 = g["grad64/" + n]
        got = p.grad.detach().cpu().numpy()
        if np.abs(r64).max() < 1e-6 * scale:  # zero in exact arithmetic: fp32 noise on both sides
            small.append(n)
            assert np.abs(got).max() < 1e-5 * scale, n
            continue
        e_gpu, e_ref = rel_err(got, r64), float(g["eref/" + n])
        if e_gpu > max(1e-4, 2 * e_ref):
            bad.append((n, e_gpu, e_ref))
    worst = max((rel_err(p.grad.detach().cpu().numpy(), g["grad64/" + n]) for n, p in named if n not in small))
    print(f"{what}: worst gradient error {worst:.3e}; zero tensors {small}")
    assert not bad, bad
    assert all(n.endswith("linear_k.bias") for n in small), small


def _encoder_case(dev, name):
    conf, T2, lens, seed = CH.ENC_FIXTURES[name]
    g = CH.load(name)
    feats, lens_t, cot = CH.enc_inputs(4 * T2 + 3, lens, seed + 1, D=conf["output_size"])
    enc = _encoder(dev, conf, seed)
    hs, olens, dfeats, dembed = _encoder_step(dev, enc, feats, lens_t, cot)
    assert olens.tolist() == g["olens"].tolist()
    assert tuple(hs.shape) == g["out_f64"].shape
    e_gpu = float(np.abs(hs.numpy().astype(np.float64) - g["out_f64"]).max())
    e_ref = float(np.abs(g["out_f32"].astype(np.float64) - g["out_f64"]).max())
    print(f"{name}: output ours {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= max(2 * e_ref, 1e-5)
    e_gpu, e_ref = rel_err(dfeats.numpy(), g["dfeats_f64"]), rel_err(g["dfeats_f32"], g["dfeats_f64"])
    print(f"{name}: input gradient ours {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= max(1e-4, 2 * e_ref)
    e_gpu, e_ref = rel_err(dembed.numpy(), g["dembed_f64"]), rel_err(g["dembed_f32"], g["dembed_f64"])
    print(f"{name}: gradient at the subsampling output ours {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= max(1e-4, 2 * e_ref)
    _grad_gate(list(enc.named_parameters()), g, name)
    return enc


@pytest.mark.parametrize("name", ["cbt_enc_t9", "cbt_enc_t11", "cbt_enc_t12", "cbt_enc_t13"])
def test_encoder_forward_and_gradients(dev, attn_fused, name):
    enc = _encoder_case(dev, name)
    assert enc.layout(CH.ENC_FIXTURES[name][1]) is not None


def test_encoder_without_ctx_pos_enc(dev, attn_fused):
    _encoder_case(dev, "cbt_enc_t13_noctxpe")


def test_short_path_honours_the_pad_mask(dev, attn_fused):
    """T' = 8 <= block_size: the plain stack with key lengths; unequal lengths, so ignoring the pad mask (as block
    mode does) would miss the gates."""
    enc = _encoder_case(dev, "cbt_enc_t8_short")
    assert enc.layout(8) is None


def test_block_size_above_the_fused_limit_runs_generic(dev, attn_fused, monkeypatch):
    """block_size 64 is S = 66 slots, above esp_block_attn's 64: the layout kernels take any block size and block mode
    runs on the generic attention kernels whatever the switch says; same gates against the reference."""
    from espnet_slurp_amd import kernels as K
    assert not K.block_attn_ok(66, 16)

    def no_fused(*a, **k):
        raise AssertionError("fused block attention launched at S = 66")

    monkeypatch.setattr(K, "block_attn_fwd", no_fused)
    enc = _encoder_case(dev, "cbt_enc_bs64")
    L = enc.layout(70)
    assert (L.S, L.nblk) == (66, 2)


def test_recipe_block_shape_s42_dk64(dev, attn_fused):
    """D = 128, 2 heads (d_k 64), block 40 / 16 / 16 (S = 42), T' = 75: gradient norms and a 16-element slice per
    tensor against the fp64 run."""
    c = CH.S42
    conf, T2, lens, seed = c["conf"], c["T2"], c["lens"], c["seed"]
    g = CH.load(c["name"])
    feats, lens_t, cot = CH.enc_inputs(4 * T2 + 3, lens, seed + 1, D=conf["output_size"])
    enc = _encoder(dev, conf, seed)
    hs, olens, _, dembed = _encoder_step(dev, enc, feats, lens_t, cot)
    assert olens.tolist() == g["olens"].tolist()
    e_gpu = float(np.abs(hs.numpy().astype(np.float64) - g["out_f64"]).max())
    e_ref = float(np.abs(g["out_f32"].astype(np.float64) - g["out_f64"]).max())
    print(f"s42: output ours {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= max(2 * e_ref, 1e-5)
    assert rel_err(dembed.numpy(), g["dembed_f64"]) <= max(1e-4, 2 * rel_err(g["dembed_f32"], g["dembed_f64"]))
    scale = max(float(g["gn_f64/" + n]) for n, _ in enc.named_parameters())
    bad = []
    for n, p in enc.named_parameters():
        n64, n32 = float(g["gn_f64/" + n]), float(g["gn_f32/" + n])
        got = p.grad.double()
        if n64 < 1e-6 * scale:
            assert n.endswith("linear_k.bias") and float(got.norm()) <= 1e-5 * scale, n
            continue
        e_n, e_nref = abs(float(got.norm()) - n64) / n64, abs(n32 - n64) / n64
        gmax = float(g["gmax_f64/" + n])
        s64 = g["slice_f64/" + n]
        e_s = float(np.abs(got.flatten()[:16].cpu().numpy() - s64).max()) / gmax
        e_sref = float(np.abs(g["slice_f32/" + n] - s64).max()) / gmax
        if e_n > max(1e-4, 2 * e_nref) or e_s > max(1e-4, 2 * e_sref):
            bad.append((n, e_n, e_nref, e_s, e_sref))
    assert not bad, bad


def _model(dev, dropout=None):
    from espnet_slurp_amd.tasks.asr import build_model
    name, conf, B, T, lens, ulens, seed = CH.MODEL_FIXTURE
    model = build_model(BH.args_from_conf(conf, dropout=dropout), device=dev)
    BH.load_seeded(model, seed)
    return model, CH.load(name)


def test_small_model_training_step(dev, attn_fused):
    model, g = _model(dev)
    assert int(sum(p.numel() for p in model.parameters())) == int(g["num_params"])
    model.train()
    loss, stats, weight = model(torch.from_numpy(g["speech"]).to(dev), torch.from_numpy(g["speech_lengths"]),
                                torch.from_numpy(g["text"]), torch.from_numpy(g["text_lengths"]))
    loss.backward()
    torch.cuda.synchronize()
    assert loss.shape == (1,) and weight.tolist() == [3]
    for key, got in (("loss", loss.item()), ("loss_ctc", stats["loss_ctc"].item()),
                     ("loss_att", stats["loss_att"].item())):
        print(f"CBT {key} got={got!r} f64={float(g[key + '_f64'])!r} f32={float(g[key + '_f32'])!r}")
        assert abs(got - float(g[key + "_f64"])) < 1e-4, (key, got, float(g[key + "_f64"]))
    assert abs(stats["acc"].item() - float(g["acc_f64"])) < 1e-6
    _grad_gate(list(model.named_parameters()), g, "cbt_model_small")


def test_eval_forward_and_speech2text(dev, attn_fused):
    model, g = _model(dev)
    model.eval()
    with torch.no_grad():
        enc, olens = model.encode(torch.from_numpy(g["speech"]).to(dev), torch.from_numpy(g["speech_lengths"]))
    assert olens.cpu().tolist() == g["enc_olens"].tolist()
    assert enc.shape == g["enc_out"].shape
    e_gpu = float(np.abs(enc.cpu().numpy().astype(np.float64) - g["enc_out_f64"]).max())
    e_ref = float(np.abs(g["enc_out"].astype(np.float64) - g["enc_out_f64"]).max())
    print(f"eval forward: ours {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= max(2 * e_ref, 1e-5)
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    s2t = Speech2Text(model)  # the default search
    res = s2t(torch.from_numpy(g["speech"][1][: int(g["speech_lengths"][1])]))
    assert len(res) >= 1 and res[0][3].yseq[0].item() == 31 and isinstance(res[0][2], list)


def test_dropout_deterministic_and_on(dev):
    """Dropouts on (0.1): the same seed repeats loss and gradients bit for bit, another seed does not."""
    g = None
    runs = []
    for s in (7, 7, 8):
        model, g = _model(dev, dropout=0.1)
        torch.manual_seed(s)
        model.train()
        loss, _, _ = model(torch.from_numpy(g["speech"]).to(dev), torch.from_numpy(g["speech_lengths"]),
                           torch.from_numpy(g["text"]), torch.from_numpy(g["text_lengths"]))
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.item(), model.flat.grad.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0] != runs[2][0]
    assert abs(runs[0][0] - float(g["loss_f64"])) > 1e-3
    assert bool(torch.isfinite(runs[0][1]).all())


def test_head_width_outside_the_fused_kernel_runs_generic(dev, monkeypatch):
    """d_k = 8 is outside esp_block_attn's shapes: block mode then takes the generic attention kernels whatever the
    switch says (no error, the same bits), and the fused kernel is never launched."""
    from espnet_slurp_amd import kernels as K
    conf, T2, lens, seed = CH.ENC_FIXTURES["cbt_enc_t13"]
    conf = {**conf, "attention_heads": 4}
    feats, lens_t, cot = CH.enc_inputs(4 * T2 + 3, lens, seed + 1, D=conf["output_size"])
    assert not K.block_attn_ok(conf["block_size"] + 2, conf["output_size"] // 4)

    def no_fused(*a, **k):
        raise AssertionError("fused block attention launched at d_k = 8")

    monkeypatch.setattr(K, "block_attn_fwd", no_fused)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(K, "CBT_ATTN_FUSED", fused)
        enc = _encoder(dev, conf, seed)
        hs, _, dfeats, _ = _encoder_step(dev, enc, feats, lens_t, cot)
        outs.append((hs, dfeats, enc.flat.grad.clone().cpu()))
    assert bool(torch.isfinite(outs[0][0]).all())
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
