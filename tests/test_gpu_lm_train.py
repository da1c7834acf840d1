"""Transformer LM training on the MI355X against the reference's own TransformerLM / ESPnetLanguageModel in .train()
mode (tests/golden/lm_train*.npz, written by make_lm_train_golden.py in fp32 and in fp64).

Gates: the loss by tests.helpers.loss_gate's rule, |ours - ref64| <= max(1e-4, 2 |ref32 - ref64|); every parameter's
gradient by grad_gate's rule on the whole tensor: the L2 norm (relative) and the largest element error (relative to
the tensor's fp64 maximum) within max(1e-4, 2 e_ref), e_ref the reference fp32 run's own figure; a gradient whose fp64
maximum is below 1e-6 of the model's largest counts as zero and must stay below 1e-5 of that scale.
LMs: A (pos_enc None, d_k 32), B (sinusoidal, d_k 16), C (d_k 64); batches b1 (lengths 7, 5, 2), b2 (12, 1, 9, 12).

Directional derivative under dropout (test_dropout_directional_derivative, eps 1e-2, batch b2, model A), relative
error of (loss(theta + eps d) - loss(theta - eps d)) / (2 eps) against g . d, first measured on an MI355X:
see DESIGN.md 3.6e."""
import numpy as np
import pytest
import torch

from espnet_slurp_amd import kernels as K
from tests.helpers import golden, loss_gate
from tests.lm_helpers import LM_CFGS, V, golden_state, lm_golden

pytestmark = pytest.mark.gpu


def _batches():
    g, t = lm_golden(), golden("lm_train")
    return {"b1": (torch.tensor(g["fwd_text"]), torch.tensor(g["fwd_lens"])),
            "b2": (torch.tensor(t["b2_text"]), torch.tensor(t["b2_lens"]))}


def _model(tag, dev, dropout=0.0):
    from espnet_slurp_amd.lm import ESPnetLanguageModel, TransformerLM
    lm = TransformerLM(V, **dict(LM_CFGS[tag], dropout_rate=dropout))
    lm.load_state_dict(golden_state(tag), strict=True)
    lm.positional_dropout_rate = dropout  # (the fixture runs PositionalEncoding's own dropout at 0 as well)
    model = ESPnetLanguageModel(lm.to(dev), V)
    model.flatten()
    return model.train()


def _step(model, text, lens, seed=0):
    """One training forward + backward from zeroed gradients -> (loss tensor on the host, ntokens)."""
    torch.manual_seed(seed)
    model.flat.zero_grad()
    loss, stats, weight = model(text, lens)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(stats["loss"], loss.detach())
    return loss.detach().cpu(), int(weight)


def _grads(model):
    return {n: p.grad.detach().double().cpu() for n, p in model.lm.named_parameters()}


def _grad_failures(grads, tag, b):
    g, part = golden("lm_train"), golden(f"lm_train.{tag}")
    key = f"{tag}.{b}."
    scale = max(float(g[key + "gmax_f64/" + n]) for n in grads)
    bad, worst = [], 0.0
    for n, got in grads.items():
        assert bool(torch.isfinite(got).all()), n
        gm = float(g[key + "gmax_f64/" + n])
        if gm < 1e-6 * scale:
            if float(got.abs().max()) > 1e-5 * scale:
                bad.append((n, "nonzero", float(got.abs().max())))
            continue
        gn64, gn32 = float(g[key + "gn_f64/" + n]), float(g[key + "gn_f32/" + n])
        e_norm, r_norm = abs(float(got.norm()) - gn64) / gn64, abs(gn32 - gn64) / gn64
        if e_norm > max(1e-4, 2 * r_norm):
            bad.append((n, "norm", e_norm, r_norm))
        want = torch.from_numpy(part[f"{b}.g/{n}"]).double()
        e_max, r_max = float((got - want).abs().max()) / gm, float(g[key + "emax_f32/" + n]) / gm
        worst = max(worst, e_max)
        if e_max > max(1e-4, 2 * r_max):
            bad.append((n, "max", e_max, r_max))
    print(f"GRAD_GATE {tag} {b}: worst whole-tensor error {worst:.3e} of the tensor maximum; failures {bad}")
    return bad, scale


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_loss_and_gradients_match_reference(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(K, "LM_ATTN_FUSED", fused)
    g = golden("lm_train")
    model = _model(tag, dev)
    for b, (text, lens) in _batches().items():
        loss, ntokens = _step(model, text, lens)
        assert ntokens == int(g[f"{tag}.{b}.ntokens"])
        ok, info = loss_gate(float(loss), g, key=f"{tag}.{b}.loss")
        assert ok, info
        grads = _grads(model)
        bad, scale = _grad_failures(grads, tag, b)
        assert not bad, bad
        # token 0 is padding only: the reference's embedding row 0 gets no gradient
        assert float(grads["embed.weight"][0].abs().max()) <= 1e-5 * scale


def test_eval_mode_still_raises_and_no_grad_forward_is_unchanged(dev):
    model = _model("A", dev)
    text, lens = _batches()["b1"]
    model.eval()
    with torch.no_grad():
        before, _, w = model(text, lens)
    assert int(w) == 17
    with pytest.raises(NotImplementedError, match="training"):
        model(text, lens)
    model.train()
    _step(model, text, lens)
    model.eval()
    with torch.no_grad():
        after, _, _ = model(text, lens)
    assert torch.equal(before, after)


def test_three_trainer_steps_follow_the_reference(dev):
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    g = golden("lm_train")
    model = _model("A", dev)
    opt = FusedAdam(model.parameters(), model.flat, lr=1e-3)
    tr = Trainer(model, opt, None, TrainerOptions(grad_clip=5.0), cuda_graph=False)
    batches = _batches()
    for i, b in enumerate(("b1", "b2", "b1")):
        text, lens = batches[b]
        stats = tr.train_one_step(dict(text=text, text_lengths=lens))
        ok, info = loss_gate(float(stats["loss"]), dict(loss_f64=g["A.steps.loss_f64"][i],
                                                         loss_f32=g["A.steps.loss_f32"][i]))
        assert ok, (i, info)
        assert bool(torch.isfinite(stats["grad_norm"]).all())
    assert float(model.flat.grad.abs().max()) == 0.0  # zero_grad after the update


def _directional_error(model, text, lens, dev, eps=1e-2):
    """Relative error of the central difference along d = g / |g| against g . d, the dropout seeds held fixed."""
    model.flat.zero_grad()
    prep = model.prepare(text, lens).to_device(dev)
    loss, _, _ = model.forward_prepared(prep)
    loss.backward()
    gvec = model.flat.grad.clone()
    gd = float(gvec.double().norm())
    d = (gvec.double() / gd).float()
    vals = []
    with torch.no_grad():
        for sign in (1.0, -1.0):
            model.flat.flat.add_(d, alpha=sign * eps)
            vals.append(float(model.forward_prepared(prep)[0]))
            model.flat.flat.add_(d, alpha=-sign * eps)
    fd = (vals[0] - vals[1]) / (2 * eps)
    return abs(fd - gd) / gd, fd, gd


def test_dropout_is_seeded_and_its_gradient_is_the_derivative(dev):
    text, lens = _batches()["b2"]
    model = _model("A", dev, dropout=0.1)
    l1, _ = _step(model, text, lens, seed=7)
    g1 = model.flat.grad.clone()
    l2, _ = _step(model, text, lens, seed=7)
    assert torch.equal(l1, l2) and torch.equal(g1, model.flat.grad)  # same seeds: bit-equal
    l3, _ = _step(model, text, lens, seed=8)
    assert not torch.equal(l1, l3) and not torch.equal(g1, model.flat.grad)
    clean, _ = _step(_model("A", dev), text, lens)
    assert not torch.equal(l1, clean)
    torch.manual_seed(11)
    e_drop, fd, gd = _directional_error(model, text, lens, dev)
    e_ref, fd0, gd0 = _directional_error(_model("A", dev), text, lens, dev)
    print(f"DIRECTIONAL dropout 0.1: fd {fd:.6f} g.d {gd:.6f} rel {e_drop:.3e}; dropout 0: fd {fd0:.6f} g.d {gd0:.6f} "
          f"rel {e_ref:.3e}; allowed {3 * e_ref:.3e}")
    assert e_drop <= 3 * e_ref, (e_drop, e_ref)


def _eager(model, text, lens, dev, l_bucket=None):
    model.flat.zero_grad()
    prep = model.prepare(text, lens, l_bucket=l_bucket).to_device(dev)
    loss, _, _ = model.forward_prepared(prep)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), model.flat.grad.clone()


def test_graph_capture_replays_another_batch(dev):
    model = _model("A", dev)
    text, lens = _batches()["b2"]
    prep = model.prepare(text, lens).to_device(dev)

    def body():
        model.flat.grad.zero_()
        loss, _, _ = model.forward_prepared(prep)
        loss.backward()
        return loss

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up: workspaces and the kernels' LDS grants
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = body()
    # another batch of the same shape (4 x 13), other lengths (so another ntokens) and tokens
    lens2 = torch.tensor([9, 12, 12, 3])
    text2 = torch.zeros_like(text)
    for i, n in enumerate(lens2):
        text2[i, :n] = (text[(i + 1) % 4, :12].repeat(2)[3:3 + int(n)] + 5) % (V - 2) + 1
    for t, l in ((text2, lens2), (text, lens)):
        model.prepare(t, l).copy_into(prep)
        graph.replay()
        torch.cuda.synchronize()
        got_loss, got_grad = loss_g.detach().clone(), model.flat.grad.clone()
        want_loss, want_grad = _eager(model, t, l, dev)
        assert torch.equal(got_loss, want_loss) and torch.equal(got_grad, want_grad)
        assert bool(torch.isfinite(got_grad).all()) and float(got_grad.abs().max()) > 0.0


def test_longer_than_lmax_takes_the_generic_path(dev, monkeypatch):
    """L = 70 (above the fused kernel's 64): model C on a batch of 63 tokens at most, run at L = 64 on the generic
    kernels, against the same batch padded to L = 70 with the fused path switched on -- the padding is invisible, so
    loss and gradients must agree within the gradient gate's floor (1e-4 of each tensor's maximum and norm)."""
    g = torch.Generator().manual_seed(70)
    lens = torch.tensor([63, 40, 1])
    text = torch.zeros(3, 63, dtype=torch.int64)
    for i, n in enumerate(lens):
        text[i, :n] = torch.randint(1, V - 1, (int(n),), generator=g)
    model = _model("C", dev)
    monkeypatch.setattr(K, "LM_ATTN_FUSED", False)
    want_loss, want_grad = _eager(model, text, lens, dev)
    monkeypatch.setattr(K, "LM_ATTN_FUSED", True)
    assert not K.causal_attn_ok(70, 64)
    got_loss, got_grad = _eager(model, text, lens, dev, l_bucket=70)
    fused_loss, fused_grad = _eager(model, text, lens, dev)  # L = 64: the fused kernel at its limit
    for what, l, gr in (("L=70 generic", got_loss, got_grad), ("L=64 fused", fused_loss, fused_grad)):
        assert bool(torch.isfinite(l).all()) and bool(torch.isfinite(gr).all())
        assert abs(float(l) - float(want_loss)) <= 1e-4, what
        for n, p in model.lm.named_parameters():
            o, k = model.flat.slots[id(p)]
            a, b = gr[o:o + k].double(), want_grad[o:o + k].double()
            gm = float(b.abs().max())
            if gm < 1e-6 * float(want_grad.abs().max()):
                assert float(a.abs().max()) <= 1e-5 * float(want_grad.abs().max()), (what, n)
                continue
            assert float((a - b).abs().max()) <= 1e-4 * gm, (what, n)
            assert abs(float(a.norm()) - float(b.norm())) <= 1e-4 * float(b.norm()), (what, n)
