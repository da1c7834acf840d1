"""The LSTM predictor's kernels (csrc/lstm.hip through asr/decoder/transducer_decoder.py) against torch.nn.LSTM on the
CPU in fp64, with torch's own fp32 run as the yardstick: err(ours vs fp64) <= max(2 * err(fp32 torch vs fp64), floor),
floors 1e-5 of the tensor's fp64 maximum element-wise and 1e-4 on relative norms.

Two stacked layers at H = 40, 320 x B = 1, 3, 70 x U1 = 1, 2, 9: the outputs, the final (h, c), and the whole
gradients of the input, the weights and the biases.  The decode surface: rnn_forward from a carried state equals
position u of the sequence run.  Dropout: p = 0 is bit-equal to no dropout, a seed fixes the masks, and the gradient
is the derivative of the loss the forward computed (directional derivative, eps 1e-2, relative error against g . d,
gated at 3 x the same figure without dropout as tests/test_gpu_lm_train.py does; the measured figures: DESIGN.md 3.6f).
"""
import pytest
import torch
from torch import nn

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd.blocks import Seeds
from espnet_slurp_amd.flat import FlatParams

pytestmark = pytest.mark.gpu

ELEM_FLOOR, NORM_FLOOR = 1e-5, 1e-4


def _stack(H, dev, seed):
    from espnet_slurp_amd.asr.decoder.transducer_decoder import LSTMLayer
    torch.manual_seed(seed)
    ref = nn.LSTM(H, H, 2, batch_first=True)
    ours = nn.ModuleList([LSTMLayer(H, H), LSTMLayer(H, H)])
    with torch.no_grad():
        for l in range(2):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(ours[l], n + "_l0").copy_(getattr(ref, f"{n}_l{l}"))
    ours = ours.to(dev)
    flat = FlatParams(ours, dev)
    return ref, ours, flat


def _reference(ref, x, dout, dtype):
    m = nn.LSTM(ref.input_size, ref.hidden_size, 2, batch_first=True).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in ref.state_dict().items()})
    xx = x.to(dtype).requires_grad_(True)
    out, (h, c) = m(xx)
    (out * dout.to(dtype)).sum().backward()
    grads = {f"{l}.{n}_l0": getattr(m, f"{n}_l{l}").grad for l in range(2)
             for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    return out.detach(), h.detach(), c.detach(), xx.grad, grads


def _gate(what, got, r64, r32):
    gm = float(r64.abs().max())
    if gm == 0.0:  # U1 = 1: the recurrent weights see a zero state, their gradient is exactly zero
        assert float(got.abs().max()) == 0.0 and float(r32.abs().max()) == 0.0, what
        return
    e, r = float((got.double() - r64).abs().max()) / gm, float((r32.double() - r64).abs().max()) / gm
    n64 = float(r64.norm())
    en, rn = abs(float(got.double().norm()) - n64) / n64, abs(float(r32.double().norm()) - n64) / n64
    print(f"{what}: elem/max ours {e:.3e} torch fp32 {r:.3e}; norm ours {en:.3e} torch fp32 {rn:.3e}")
    assert not torch.isnan(got).any(), what
    assert e <= max(2 * r, ELEM_FLOOR), (what, "element", e, r)
    assert en <= max(2 * rn, NORM_FLOOR), (what, "norm", en, rn)


@pytest.mark.parametrize("U1", [1, 2, 9])
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("H", [40, 320])
def test_two_layers_against_torch(dev, H, B, U1):
    ref, ours, flat = _stack(H, dev, 7 * H + B + U1)
    g = torch.Generator().manual_seed(H + 10 * B + U1)
    x, dout = torch.randn(B, U1, H, generator=g), torch.randn(B, U1, H, generator=g)
    r64, r32 = _reference(ref, x, dout, torch.float64), _reference(ref, x, dout, torch.float32)
    flat.zero_grad()
    y0, c0 = ours[0].fwd(x.reshape(B * U1, H).to(dev), B, U1)
    y1, c1 = ours[1].fwd(y0, B, U1)
    d1 = ours[1].bwd(c1, dout.reshape(B * U1, H).to(dev))
    dx = ours[0].bwd(c0, d1)
    torch.cuda.synchronize()
    what = f"H={H} B={B} U1={U1}"
    _gate(what + " out", y1.cpu().view(B, U1, H), r64[0], r32[0])
    h = torch.stack([y0.view(B, U1, H)[:, -1], y1.view(B, U1, H)[:, -1]]).cpu()
    c = torch.stack([c0.cs[:, -1], c1.cs[:, -1]]).cpu()
    _gate(what + " h_n", h, r64[1], r32[1])
    _gate(what + " c_n", c, r64[2], r32[2])
    _gate(what + " dx", dx.cpu().view(B, U1, H), r64[3], r32[3])
    for n, p in ours.named_parameters():
        _gate(f"{what} d{n}", p.grad.cpu(), r64[4][n], r32[4][n])


def _decoder(dev, p=0.0, layers=2, H=40, V=11, seed=3):
    from espnet_slurp_amd.asr.decoder.transducer_decoder import TransducerDecoder
    torch.manual_seed(seed)
    dec = TransducerDecoder(V, num_layers=layers, hidden_size=H, dropout=p, dropout_embed=p).to(dev)
    flat = FlatParams(dec, dev)
    return dec, flat


def _dec_in(dev, B=3, U1=6, V=11):
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(1, V, (B, U1), generator=g)
    tok[:, 0] = 0
    tok[1, 3:] = 0  # blank padding
    grad_tok = tok.clone()
    grad_tok[tok == 0] = -1
    return tok.to(dev), grad_tok.to(dev)


def test_step_from_a_carried_state_is_the_sequence_position(dev):
    dec, _ = _decoder(dev)
    tok, _ = _dec_in(dev)
    B, U1 = tok.shape
    seq = dec(tok)  # (B, U1, H)
    state = dec.init_state(B)
    for u in range(U1):
        with torch.no_grad():
            emb = dec._embed(tok[:, u].contiguous(), B).view(B, 1, -1)
        out, state = dec.rnn_forward(emb, state)
        gm = float(seq[:, u].abs().max())
        assert float((out[:, 0] - seq[:, u]).abs().max()) <= ELEM_FLOOR * gm, u
    # the reference's cache semantics: one entry per label sequence, reused
    from espnet_slurp_amd.asr.transducer.beam_search_transducer import Hypothesis
    cache = {}
    hyp = Hypothesis(score=0.0, yseq=[0, 4], dec_state=dec.init_state(1))
    o1, s1, lab = dec.score(hyp, cache)
    o2, s2, _ = dec.score(hyp, cache)
    assert list(cache) == ["0_4"] and o1.data_ptr() == o2.data_ptr() and int(lab) == 4 and o1.shape == (dec.dunits,)
    cache2 = {}
    bo, bs, _ = dec.batch_score([hyp, Hypothesis(0.0, [0, 7], dec.init_state(1))], dec.init_state(2), cache2, False)
    assert bo.shape == (2, dec.dunits) and bs[0].shape == (2, 2, dec.dunits)
    assert float((bo[0] - o1).abs().max()) <= ELEM_FLOOR * float(o1.abs().max())
    assert sorted(cache2) == ["0_4", "0_7"]
    sel = dec.select_state(bs, 1)
    assert sel[0].shape == (2, 1, dec.dunits) and torch.equal(sel[0][:, 0], bs[0][:, 1])


def _run(dec, flat, tok, gtok, R, seed, training=True):
    flat.zero_grad()
    out, saved = dec.run_forward(tok, gtok, Seeds(seed), training)
    loss = (out * R).sum()
    dec.run_backward(saved, R.clone())
    torch.cuda.synchronize()
    return out.clone(), loss, flat.grad.clone()


def _directional_error(dec, flat, tok, gtok, R, seed, eps=1e-2):
    _, _, gvec = _run(dec, flat, tok, gtok, R, seed)
    gd = float(gvec.double().norm())
    d = (gvec.double() / gd).float()
    vals = []
    with torch.no_grad():
        for sign in (1.0, -1.0):
            flat.flat.add_(d, alpha=sign * eps)
            out, _ = dec.run_forward(tok, gtok, Seeds(seed), True, keep=False)
            vals.append(float((out.double() * R.double()).sum()))
            flat.flat.add_(d, alpha=-sign * eps)
    fd = (vals[0] - vals[1]) / (2 * eps)
    return abs(fd - gd) / gd, fd, gd


def test_dropout_is_seeded_and_its_gradient_is_the_derivative(dev):
    tok, gtok = _dec_in(dev)
    B, U1 = tok.shape
    clean, flat0 = _decoder(dev, 0.0)
    R = torch.randn(B * U1, clean.dunits, generator=torch.Generator().manual_seed(9)).to(dev)
    o_eval, _, g_eval = _run(clean, flat0, tok, gtok, R, 1, training=False)
    o_p0, _, g_p0 = _run(clean, flat0, tok, gtok, R, 2, training=True)
    assert torch.equal(o_eval, o_p0) and torch.equal(g_eval, g_p0)  # p = 0: bit-equal to no dropout, any seed
    assert float(flat0.gview(clean.embed.weight)[0].abs().max()) == 0.0  # the padding row gets no gradient
    assert float(flat0.gview(clean.embed.weight)[1:].abs().max()) > 0.0
    dec, flat = _decoder(dev, 0.2)
    o1, _, g1 = _run(dec, flat, tok, gtok, R, 7)
    o2, _, g2 = _run(dec, flat, tok, gtok, R, 7)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)  # same seed: bit-equal
    o3, _, g3 = _run(dec, flat, tok, gtok, R, 8)
    assert not torch.equal(o1, o3) and not torch.equal(g1, g3) and not torch.equal(o1, o_p0)
    e_drop, fd, gd = _directional_error(dec, flat, tok, gtok, R, 7)
    e_ref, fd0, gd0 = _directional_error(clean, flat0, tok, gtok, R, 7)
    print(f"DIRECTIONAL lstm dropout 0.2: fd {fd:.6f} g.d {gd:.6f} rel {e_drop:.3e}; dropout 0: fd {fd0:.6f} g.d "
          f"{gd0:.6f} rel {e_ref:.3e}; allowed {3 * e_ref:.3e}")
    assert e_drop <= 3 * e_ref, (e_drop, e_ref)


def test_gru_raises_by_name():
    from espnet_slurp_amd.asr.decoder.transducer_decoder import TransducerDecoder
    with pytest.raises(NotImplementedError, match="gru"):
        TransducerDecoder(11, rnn_type="gru")
    with pytest.raises(ValueError, match="rnn_type=rnn"):
        TransducerDecoder(11, rnn_type="rnn")
    assert K.RNNT_ACT == {"tanh": 0, "relu": 1}
