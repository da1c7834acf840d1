"""MaskCTCInference.forward_batch / MLMDecoder.forward_masked_batch / asr_inference_maskctc.Speech2Text.decode_batch
against the reference's MaskCTCInference.forward, one reference run per utterance, on recorded encoder outputs of the
small decoding model (maskctc_decode_batch.npz, tests/golden/make_maskctc_batch_golden.py).

For every utterance of a batch the token row after every pass and the final yseq must be exactly the reference's.
That is fair for the reason test_gpu_maskctc_decode.py gives: the generator kept an utterance only when each decision's
margin is at least 100 x the reference's own fp32-vs-fp64 deviation of that quantity; margins and deviations are in
the fixture and re-checked here."""
import numpy as np
import pytest
import torch

from tests import maskctc_helpers as MH
from tests.helpers import golden
from tests.test_gpu_maskctc_decode import _case as _single_case
from tests.test_gpu_maskctc_decode import _model

pytestmark = pytest.mark.gpu


def _batch(name):
    """(case-level entries, one dict per utterance) of a batch case."""
    g = golden("maskctc_decode_batch")
    top = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/") and k.count("/") == 1}
    utts = [{k.split("/", 2)[2]: v for k, v in g.items() if k.startswith(f"{name}/{u}/")} for u in range(int(top["U"]))]
    return top, utts


def _padded(utts, dev, extra=()):
    encs = [c["enc"] for c in utts] + list(extra)
    lens = [e.shape[0] for e in encs]
    # the padding is garbage on purpose: no frame beyond an utterance's length may matter
    pad = np.full((len(encs), max(lens), encs[0].shape[1]), 1e3, dtype=np.float32)
    for u, e in enumerate(encs):
        pad[u, :e.shape[0]] = e
    return torch.from_numpy(pad).to(dev), lens


def _check_against_reference(utts, hyps, trace, last_batch, mask):
    got = [t.cpu().numpy() for t in trace]
    assert len(got) == 1 + max(int(c["passes"]) for c in utts)
    for u, c in enumerate(utts):
        L, mask_num, passes = int(c["L"]), int(c["mask_num"]), int(c["passes"])
        assert (last_batch[u]["L"], last_batch[u]["mask_num"], last_batch[u]["num_iter"]) == (L, mask_num, passes), u
        for t, arr in enumerate(got):  # after its last pass an utterance idles: its final row stays
            want = c["rows"][min(t, passes)] if L else np.zeros(0, dtype=np.int64)
            assert np.array_equal(arr[u, :L], want), (u, t, arr[u, :L], want)
        assert np.array_equal(hyps[u].yseq.numpy(), c["yseq"]), u
        assert hyps[u].yseq[0] == hyps[u].yseq[-1] == mask
        if L == 0:
            assert hyps[u].yseq.tolist() == [mask, mask]


def _assert_margins(c):
    for m, d in (("argmax", "argmax"), ("prob", "prob"), ("top1", "logit"), ("topk", "logit")):
        assert float(c["margin_" + m]) >= 100.0 * float(c["dev_" + d]), (m, float(c["margin_" + m]), float(c["dev_" + d]))


@pytest.mark.parametrize("name", ["mixed", "blank"])
def test_forward_batch_matches_reference_pass_by_pass(dev, name):
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    top, utts = _batch(name)
    for c in utts:
        _assert_margins(c)
    _, model = _model(dev, int(top["blank"]))
    inf = MaskCTCInference(model, n_iterations=int(top["n_iterations"]), threshold_probability=float(top["thr"]))
    enc_pad, lens = _padded(utts, dev)
    trace = []
    hyps = inf.forward_batch(enc_pad, lens, trace=trace)
    assert len(hyps) == len(utts) == int(top["U"])
    _check_against_reference(utts, hyps, trace, inf.last_batch, model.mask_token)
    # the batch agrees with the single-utterance path on every utterance
    for u, c in enumerate(utts):
        one = inf(torch.from_numpy(c["enc"]).to(dev))
        assert torch.equal(one.yseq, hyps[u].yseq), u


def test_forward_batch_on_run_forward(dev):
    """The path of a head size esp_decode_attn does not serve: every pass through MLMDecoder.run_forward on the
    active utterances' padded memory.  The same rows as the reference's."""
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    top, utts = _batch("mixed")
    _, model = _model(dev, 0)
    inf = MaskCTCInference(model, n_iterations=int(top["n_iterations"]), threshold_probability=float(top["thr"]))
    assert inf.prepared_memory
    inf.prepared_memory = False
    enc_pad, lens = _padded(utts, dev)
    trace = []
    hyps = inf.forward_batch(enc_pad, lens, trace=trace)
    _check_against_reference(utts, hyps, trace, inf.last_batch, model.mask_token)


def test_forward_batch_with_an_all_blank_utterance(dev):
    """The mixed batch plus a sixth utterance of three copies of a recorded blank frame: that one returns the
    two-<mask> hypothesis without reaching the decoder, the other five are unchanged."""
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    top, utts = _batch("mixed")
    bu, bt = (int(v) for v in top["blank_frame"])
    assert utts[bu]["lp"][bt].argmax() == 0
    frame = utts[bu]["enc"][bt]
    _, model = _model(dev, 0)
    inf = MaskCTCInference(model, n_iterations=int(top["n_iterations"]), threshold_probability=float(top["thr"]))
    enc_pad, lens = _padded(utts, dev, extra=[np.stack([frame] * 3)])
    trace = []
    hyps = inf.forward_batch(enc_pad, lens, trace=trace)
    assert len(hyps) == 6 and lens[5] == 3
    assert hyps[5].yseq.tolist() == [model.mask_token] * 2
    assert inf.last_batch[5] == dict(L=0, mask_num=0, num_iter=0)
    _check_against_reference(utts, hyps[:5], trace, inf.last_batch[:5], model.mask_token)


def test_forward_masked_batch_pass0_logits(dev):
    """Pass 0 of the active utterances of `mixed` in one forward_masked_batch: each utterance's valid rows against
    the reference's fp64 logits of that pass, within max(2 e_ref, 1e-5) (test_prepared_memory_pass_equals_run_forward's
    gate)."""
    top, utts = _batch("mixed")
    _, model = _model(dev, 0)
    enc_pad, lens = _padded(utts, dev)
    mem = model.decoder.prepare_memory(enc_pad, lens)
    rows = np.array([u for u, c in enumerate(utts) if int(c["passes"]) > 0], dtype=np.int32)
    assert len(rows) >= 3
    ylens = np.array([int(utts[u]["L"]) for u in rows], dtype=np.int32)
    Lmax = int(ylens.max())
    assert len(set(ylens.tolist())) > 1  # ragged
    y = np.zeros((len(rows), Lmax), dtype=np.int64)
    for a, u in enumerate(rows):
        y[a, :ylens[a]] = utts[u]["rows"][0]
    V1 = model.vocab_size
    logits = model.decoder.forward_masked_batch(torch.from_numpy(y).to(dev), ylens, mem, rows)
    assert logits.shape == (len(rows) * Lmax, V1)
    logits = logits.view(len(rows), Lmax, V1).cpu().double().numpy()
    again = model.decoder.forward_masked_batch(torch.from_numpy(y).to(dev), ylens, mem, rows)  # cached indices
    assert np.array_equal(again.view(len(rows), Lmax, V1).cpu().double().numpy(), logits)
    for a, u in enumerate(rows):
        c = utts[u]
        tol = max(2 * float(c["pred0_eref"]), 1e-5)
        err = np.abs(logits[a, :ylens[a]] - c["pred0_f64"]).max()
        print(f"utterance {u}: L {ylens[a]} of {Lmax}, pass-0 logits error {err:.3e} e_ref "
              f"{float(c['pred0_eref']):.3e} tol {tol:.3e}")
        assert c["pred0_f64"].shape == (ylens[a], V1) and err <= tol, (u, err, tol)


def test_forward_masked_batch_refuses_an_empty_sequence(dev):
    top, utts = _batch("mixed")
    _, model = _model(dev, 0)
    enc_pad, lens = _padded(utts[:2], dev)
    mem = model.decoder.prepare_memory(enc_pad, lens)
    y = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="forward_masked_batch"):
        model.decoder.forward_masked_batch(y, [4, 0], mem, [0, 1])


def test_decode_batch_of_one_equals_call(dev):
    from espnet_slurp_amd.bin.asr_inference_maskctc import Speech2Text
    c = _single_case("many")
    cfg, model = _model(dev, int(c["blank"]))
    s2t = Speech2Text(model, n_iterations=int(c["n_iterations"]), threshold_probability=float(c["thr"]))
    speech = MH.decode_speech(cfg, int(c["seed"]))
    out = s2t.decode_batch([speech])
    one = s2t(speech)
    assert len(out) == 1 and len(out[0]) == 1
    assert out[0][0][:3] == one[0][:3] and torch.equal(out[0][0][3].yseq, one[0][3].yseq)
    assert np.array_equal(out[0][0][3].yseq.numpy(), c["yseq"])


def test_decode_batch_ragged_equals_forward_batch_on_its_encode(dev):
    from espnet_slurp_amd.bin.asr_inference_maskctc import Speech2Text
    from oracle import espnet_cpu as O
    top, _ = _batch("mixed")
    cfg, model = _model(dev, 0)
    s2t = Speech2Text(model, n_iterations=int(top["n_iterations"]), threshold_probability=float(top["thr"]))
    frames = [96, 120, 72]
    speeches = [O.synthetic_batch(1, T, cfg.enc.input_size, cfg.vocab_size, [T], [3], 600 + i)[0][0]
                for i, T in enumerate(frames)]
    out = s2t.decode_batch([speeches[0].numpy(), speeches[1], speeches[2]])
    lengths = torch.tensor(frames, dtype=torch.int64)
    pad = torch.zeros(3, 120, speeches[0].shape[1])
    for i, s in enumerate(speeches):
        pad[i, :frames[i]] = s
    enc, enc_lens = model.encode(pad.to(dev), lengths, sl_cpu=lengths)
    hyps = s2t.s2t.forward_batch(enc, [int(t) for t in enc_lens])
    lens = [int(t) for t in enc_lens]  # a padded batch's lengths (not the single-utterance encodes' at the ends)
    assert lens[1] == enc.shape[1] == 29 and lens[2] < lens[0] < lens[1] and len(out) == 3
    for res, hyp in zip(out, hyps):
        assert len(res) == 1
        text, token, token_int, h = res[0]
        want = [t for t in hyp.yseq[1:-1].tolist() if t != 0]
        assert text is None and token_int == want and token == [model.token_list[i] for i in want]
        assert torch.equal(h.yseq, hyp.yseq)
