"""BatchBeamSearch on the cached one-step decoder.

Reference part: Speech2Text(..., batch_search=True) on the model and utterance of tests/test_gpu_inference.py
against the reference BatchBeamSearch's n-best lists (tests/golden/inference.npz, bs_{a,b,c}_batch_*).
Multi-utterance part: forward_batch over U=3 encoder outputs of lengths 59, 41, 23 against three forward calls of
the same class on the same rows.

Rule for comparing an n-best list with the wanted one (allowance = 1e-3 relative, the plain search's gate): rank i
is order-pinned when the wanted score gaps to both neighbours exceed twice the allowance; at a pinned rank the
token sequence must be the wanted one, at any other rank it must be one of the wanted entries whose score is
within twice the allowance of rank i's; the score must be within the allowance of the matched entry's."""
import numpy as np
import pytest
import torch

from tests.helpers import build_model, golden, load_seeded, small_cfg

pytestmark = pytest.mark.gpu

REL = 1e-3


def _model(dev):
    g = golden("inference")
    cfg = small_cfg("latest", D=64, blocks=2, V=32)
    model = build_model(cfg, dev, dropout=0.0)
    load_seeded(model, cfg, 21)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if "bn." + name in g:
                buf.copy_(torch.tensor(g["bn." + name]))
    model.eval()
    return model, g


def pinned_ranks(want_s):
    out = []
    for i, s in enumerate(want_s):
        a = 2 * REL * abs(s)
        if all(abs(s - want_s[j]) > a for j in (i - 1, i + 1) if 0 <= j < len(want_s)):
            out.append(i)
    return out


def check_nbest(got, want_y, want_s, tag=""):
    """got: [(token list, score)], want_y: [token list], want_s: scores; both best first."""
    pinned = pinned_ranks(want_s)
    assert len(got) >= min(len(want_s), 1 + max(pinned, default=0)), (tag, len(got), len(want_s))
    for i in range(min(len(got), len(want_s))):
        y, s = got[i]
        allow = REL * abs(want_s[i])
        if i in pinned:
            assert y == want_y[i], (tag, i, y, want_y[i])
            j = i
        else:
            near = [j for j in range(len(want_s)) if abs(want_s[j] - want_s[i]) <= 2 * allow and want_y[j] == y]
            assert near, (tag, i, y)
            j = near[0]
        assert abs(s - want_s[j]) <= REL * abs(want_s[j]), (tag, i, j, s, want_s[j])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_batch_search_matches_reference(dev, tag):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model, g = _model(dev)
    ctc_w, beam, penalty = g[f"bs_{tag}_cfg"]
    s2t = Speech2Text(model, beam_size=int(beam), ctc_weight=float(ctc_w), penalty=float(penalty), nbest=100,
                      batch_search=True)
    res = s2t(torch.tensor(g["speech"][0]))
    want_y = [y[y >= 0].tolist() for y in g[f"bs_{tag}_batch_yseq"]]
    want_s = g[f"bs_{tag}_batch_score"]
    if tag == "a":
        assert pinned_ranks(want_s)[:6] == [0, 1, 2, 3, 4, 5]
    got = [(r[3].yseq.tolist(), r[3].score) for r in res]
    for i, (y, s) in enumerate(got[:len(want_s)]):
        print(f"{tag} rank {i + 1}: score {s:.5f} want {want_s[i]:.5f} same tokens {y == want_y[i]}")
    check_nbest(got, want_y, want_s, tag)
    best = res[0]
    assert best[2] == [t for t in want_y[0][1:-1] if t != 0]


@pytest.mark.parametrize("ctc_w", [0.3, 1.0, 0.0])
def test_forward_batch_matches_single_utterance_search(dev, ctc_w):
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearch, CTCPrefixScorer, DecoderScorer, LengthBonus
    model, _ = _model(dev)
    V, lens = 32, [59, 41, 23]
    xs = torch.randn(3, max(lens), 64, generator=torch.Generator().manual_seed(8)).to(dev)
    bs = BatchBeamSearch(scorers=dict(decoder=DecoderScorer(model.decoder),
                                      ctc=CTCPrefixScorer(model.ctc, eos=model.eos, blank=model.blank_id),
                                      length_bonus=LengthBonus()),
                         weights=dict(decoder=1.0 - ctc_w, ctc=ctc_w, length_bonus=0.0), beam_size=4, vocab_size=V,
                         sos=model.sos, eos=model.eos, pre_beam_score_key=None if ctc_w == 1.0 else "full")
    assert ("decoder" in bs.full_scorers) == (ctc_w != 1.0) and ("ctc" in bs.part_scorers) == (ctc_w != 0.0)
    nbests = bs.forward_batch(xs, lens)
    finish = list(bs.finish_step)
    print(f"ctc_weight {ctc_w}: finish steps {finish}, n-best sizes {[len(n) for n in nbests]}")
    assert len(nbests) == 3 and all(len(n) >= 1 for n in nbests)
    assert finish[2] < finish[0] and finish[2] < finish[1], finish
    for u, T in enumerate(lens):
        single = bs.forward(xs[u, :T])
        want_y = [h.yseq.tolist() for h in single]
        want_s = np.array([h.score for h in single])
        for h in nbests[u]:
            assert h.yseq[0] == model.sos and h.yseq[-1] == model.eos
        check_nbest([(h.yseq.tolist(), h.score) for h in nbests[u]], want_y, want_s, f"utt{u}")


def test_decode_batch_returns_one_result_list_per_utterance(dev):
    from espnet_slurp_amd.asr.beam_search import Hypothesis
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model, _ = _model(dev)
    rng = np.random.RandomState(4)
    speeches = [rng.randn(n, 80).astype(np.float32) for n in (240, 200, 160)]
    s2t = Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=2)
    out = s2t.decode_batch(speeches)
    assert len(out) == 3
    for res in out:
        assert 1 <= len(res) <= 2
        for text, token, token_int, hyp in res:
            assert text is None and isinstance(hyp, Hypothesis)
            assert all(isinstance(t, str) for t in token) and all(isinstance(t, int) for t in token_int)
            assert len(token) == len(token_int)
            assert hyp.yseq[0] == model.sos and hyp.yseq[-1] == model.eos
            assert token_int == [t for t in hyp.yseq[1:-1].tolist() if t != 0]
