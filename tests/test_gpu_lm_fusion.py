"""LM shallow fusion in the joint search: Speech2Text(model, lm=..., lm_weight=...) with the plain and the batch search
against the reference's n-best lists with its TransformerLM as scorer "lm" (tests/golden/lm.npz fuse_*, written by
make_lm_golden.py on the model and utterance of tests/golden/inference.npz; the generator asserts that ranks 0, 1, 2
of every list are order-pinned and that the LM changes the best hypothesis).  Lists are compared by the rule of
tests/test_gpu_batch_beam.py (check_nbest, REL 1e-3).

The plain search's lists end in hypotheses that were cut at maxlen on a label the CTC prefix scorer gives logzero
(-1e10 * ctc_weight = -3e9 or -5e9).  One fp32 ulp at 3e9 is 256, more than any real score difference, so these
entries tie exactly in the reference as well, and which of them a beam keeps and in what order is its tie-breaking,
not a property of the scores.  They are compared as a group: the same number of entries, each at its logzero score
within REL; the rule above covers every entry in front of them (all pinned ranks lie there)."""
LOGZERO_TAIL = -1e9
import numpy as np
import pytest
import torch

from espnet_slurp_amd import _native
from espnet_slurp_amd import kernels as K
from tests.lm_helpers import V, build_lm, lm_golden
from tests.test_gpu_batch_beam import _model, check_nbest, pinned_ranks

pytestmark = pytest.mark.gpu

CONFIGS = {"a_lm": "A", "b_lm": "B"}


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("tag", ["a_lm", "b_lm"])
def test_fused_search_matches_reference(dev, tag, batch):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from espnet_slurp_amd.lm import ESPnetLanguageModel
    model, g = _model(dev)
    lg = lm_golden()
    ctc_w, beam, penalty, lm_w = lg[f"fuse_{tag}_cfg"]
    lm = build_lm(CONFIGS[tag], dev)
    s2t = Speech2Text(model, beam_size=int(beam), ctc_weight=float(ctc_w), penalty=float(penalty), nbest=100,
                      batch_search=batch, lm=ESPnetLanguageModel(lm, V) if batch else lm, lm_weight=float(lm_w))
    assert "lm" in s2t.beam_search.full_scorers and s2t.beam_search.weights["lm"] == float(lm_w)
    res = s2t(torch.tensor(g["speech"][0]))
    kind = "batch" if batch else "plain"
    want_y = [y[y >= 0].tolist() for y in lg[f"fuse_{tag}_{kind}_yseq"]]
    want_s = lg[f"fuse_{tag}_{kind}_score"]
    assert pinned_ranks(want_s)[:3] == [0, 1, 2]
    base = g[f"bs_{tag[0]}_{kind}_yseq"][0]
    assert want_y[0] != base[base >= 0].tolist(), "the fixture's LM must change the best hypothesis"
    got = [(r[3].yseq.tolist(), r[3].score) for r in res]
    for i, (y, s) in enumerate(got[:len(want_s)]):
        print(f"{tag} {kind} rank {i + 1}: score {s:.5f} want {want_s[i]:.5f} same tokens {y == want_y[i]}")
    n = int((want_s > LOGZERO_TAIL).sum())
    assert n > max(pinned_ranks(want_s)[:3]) and all(s <= LOGZERO_TAIL for s in want_s[n:])
    check_nbest(got[:n], want_y[:n], want_s[:n], f"{tag} {kind}")
    assert len(got) == len(want_s) and sum(s > LOGZERO_TAIL for _, s in got) == n
    for (_, s), w in zip(got[n:], want_s[n:]):
        assert abs(s - w) <= 1e-3 * abs(w)
    assert res[0][2] == [t for t in want_y[0][1:-1] if t != 0]
    assert "lm" in res[0][3].scores
    h = res[0][3]
    total = sum(s2t.beam_search.weights[k] * v for k, v in h.scores.items())
    assert abs(total - h.score) <= 1e-3 * abs(h.score), "the per-scorer scores must add up to the hypothesis score"


def test_forward_batch_with_lm_matches_single_utterance_search(dev):
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearch, CTCPrefixScorer, DecoderScorer, LengthBonus
    model, _ = _model(dev)
    lens = [59, 41, 23]
    xs = torch.randn(3, max(lens), 64, generator=torch.Generator().manual_seed(8)).to(dev)
    bs = BatchBeamSearch(scorers=dict(decoder=DecoderScorer(model.decoder),
                                      ctc=CTCPrefixScorer(model.ctc, eos=model.eos, blank=model.blank_id),
                                      length_bonus=LengthBonus(), lm=build_lm("A", dev)),
                         weights=dict(decoder=0.7, ctc=0.3, length_bonus=0.0, lm=0.6), beam_size=4, vocab_size=V,
                         sos=model.sos, eos=model.eos, pre_beam_score_key="full")
    nbests = bs.forward_batch(xs, lens)
    assert len(nbests) == 3 and all(len(n) >= 1 for n in nbests)
    for u, T in enumerate(lens):
        single = bs.forward(xs[u, :T])
        check_nbest([(h.yseq.tolist(), h.score) for h in nbests[u]], [h.yseq.tolist() for h in single],
                    np.array([h.score for h in single]), f"utt{u}")


@pytest.mark.parametrize("batch", [False, True])
def test_no_lm_and_zero_weight_are_todays_search(dev, batch):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model, g = _model(dev)
    speech = torch.tensor(g["speech"][0])
    kw = dict(beam_size=4, ctc_weight=0.3, penalty=0.0, nbest=100, batch_search=batch)
    today = Speech2Text(model, **kw)(speech)
    for extra in (dict(lm=None), dict(lm=build_lm("A", dev), lm_weight=0.0), dict(lm=None, lm_weight=0.6)):
        s2t = Speech2Text(model, **kw, **extra)
        assert "lm" not in s2t.beam_search.full_scorers
        res = s2t(speech)
        assert len(res) == len(today)
        for a, b in zip(res, today):
            assert a[3].yseq.tolist() == b[3].yseq.tolist() and a[3].score == b[3].score and a[3].scores == b[3].scores


def test_decode_batch_with_lm(dev):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model, _ = _model(dev)
    rng = np.random.RandomState(4)
    speeches = [rng.randn(n, 80).astype(np.float32) for n in (240, 160)]
    out = Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=2, lm=build_lm("A", dev), lm_weight=0.6).decode_batch(speeches)
    assert len(out) == 2
    for res in out:
        assert 1 <= len(res) <= 2 and all("lm" in r[3].scores and r[3].yseq[-1] == model.eos for r in res)


def test_fused_step_is_five_launches_per_layer(dev, monkeypatch):
    """Native launches of one LM step, counted through _native.call (no profiler): per layer LN + qkv + cache write,
    masked attention, out-proj + residual, LN + w_1 + ReLU, w_2 + residual; around the layers the embedding gather,
    the input Linear, its LayerNorm + ReLU + positional step, after_norm + decoder, and the log-softmax."""
    lm = build_lm("A", dev)
    ys = torch.tensor([[31, 4, 0, 7, 9]] * 6)
    _, cache = lm.batch_score(ys[:, :4], None, None)
    calls = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    assert K.LM_STEP_FUSED and ys.shape[0] <= K.LM_STEP_MAX_ROWS
    lm.batch_score(ys, cache, None)
    layers = len(lm.encoder.encoders)
    per_layer = [c for c in calls if c in ("esp_step_linear", "esp_decode_attn_masked")]
    print(f"one fused LM step, {layers} layers: {len(calls)} launches: {calls}")
    assert len(per_layer) - 2 <= 5 * layers and len(calls) <= 5 * layers + 5, calls
    assert calls.count("esp_decode_attn_masked") == layers and calls.count("esp_step_linear") == 4 * layers + 2
    del calls[:]
    monkeypatch.setattr(K, "LM_STEP_FUSED", False)
    lm.batch_score(torch.cat([ys, ys[:, :1]], 1), cache, None)
    print(f"one generic LM step: {len(calls)} launches")
    assert "esp_step_linear" not in calls and len(calls) > 5 * layers + 5
