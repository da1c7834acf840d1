"""BeamSearchTransducer on the MI355X against the reference's own search on recorded encoder outputs
(tests/golden/transducer_search.npz): greedy, and `default` at beams 2 and 5 with nbest 3, on two models x two
utterances.  The n-best token lists are the reference's entry by entry, duplicates included; the scores are within
the loss gate, |ours - ref64| <= max(1e-4, 2 |ref32 - ref64|).  Every committed case is compared: the generator kept
a case only when the reference's fp32 and fp64 n-best lists were identical, its smallest decision margin (fp64) was at
least 100 x the largest fp32-vs-fp64 score distance, and the best hypothesis was non-empty -- asserted again here from
the recorded margin and distance.  Speech2Text must return the same tokens."""
import pytest
import torch

from tests import transducer_helpers as TH
from tests.helpers import golden

pytestmark = pytest.mark.gpu


def _cases():
    g = golden("transducer_search")
    return g, g["cases"].tolist(), list(zip(g["searches"].tolist(), g["search_beam"].tolist(),
                                            g["search_nbest"].tolist()))


def _model(mname, dev):
    cfg, tc, seed = TH.search_model_of(mname)
    model = TH.build_transducer(cfg, tc, dev)
    TH.load_params(model, TH.search_params(cfg, tc, seed))
    return model.eval()


def test_every_committed_case(dev):
    from espnet_slurp_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    g, cases, searches = _cases()
    assert len(cases) >= 4 and len({c.split(".")[0] for c in cases}) >= 2
    models = {}
    for case in cases:
        mname = case.split(".")[0]
        model = models.setdefault(mname, _model(mname, dev))
        enc = torch.from_numpy(g[f"{case}/enc"]).to(dev)
        for sname, beam, nbest in searches:
            pre = f"{case}/{sname}/"
            margin, dist = float(g[pre + "margin"]), float(g[pre + "dist"])
            assert margin >= 100.0 * dist and g[pre + "yseq"][0, 1] >= 0, (case, sname, margin, dist)
            bs = BeamSearchTransducer(model.decoder, model.joint_network, beam, search_type="default",
                                      score_norm=False, nbest=nbest)
            hyps = bs(enc)
            want = [[int(t) for t in r if t >= 0] for r in g[pre + "yseq"]]
            assert [h.yseq for h in hyps] == want, (case, sname)
            for h, s64, s32 in zip(hyps, g[pre + "score_f64"], g[pre + "score_f32"]):
                tol = max(1e-4, 2 * abs(float(s32) - float(s64)))
                print(f"{case} {sname}: score err {abs(h.score - float(s64)):.3e} tol {tol:.3e} margin {margin:.3e}")
                assert abs(h.score - float(s64)) <= tol, (case, sname, h.score, float(s64))


def test_speech2text_returns_the_same_tokens(dev, monkeypatch):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    g, cases, searches = _cases()
    case = cases[0]
    model = _model(case.split(".")[0], dev)
    enc = torch.from_numpy(g[f"{case}/enc"]).to(dev)
    for sname, beam, nbest in searches:
        s2t = Speech2Text(model, beam_size=beam, nbest=nbest, transducer_conf=dict(score_norm=False, nbest=nbest))
        monkeypatch.setattr(s2t, "encode", lambda speech: enc)  # the recorded encoder output
        res = s2t(torch.zeros(TH.SEARCH_T, 80))
        want = [[int(t) for t in r[1:] if t >= 0] for r in g[f"{case}/{sname}/yseq"]]
        assert [r[2] for r in res] == [[t for t in w if t != 0] for w in want]
        assert all(r[1] == [model.token_list[t] for t in r[2]] and r[0] is None for r in res)
    # and end to end from features: the encoder runs in front of the search, the hypothesis has no <sos> / <eos> frame
    speech = TH.search_speech(TH.search_model_of(case)[0], int(g[f"{case}/utt_seed"]))
    res = Speech2Text(model, beam_size=2, transducer_conf=dict(score_norm=False))(speech)
    assert len(res) == 1 and len(res[0][2]) >= 1 and all(0 < t < TH.V for t in res[0][2])
    assert res[0][3].yseq[0] == 0 and res[0][3].yseq[1:] == res[0][2]
