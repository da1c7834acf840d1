"""MaskCTCInference / asr_inference_maskctc.Speech2Text end to end against the reference's MaskCTCInference.forward
on recorded encoder outputs of the small model (maskctc_decode.npz, tests/golden/make_maskctc_golden.py).

The token row after every pass and the final yseq must be exactly the reference's.  That is fair because the
generator asserted, for every case, that each decision's margin (per-frame CTC argmax, token probability against the
threshold, top-1 against top-2 logit at every filled position, k-th against (k+1)-th score of every top-k) is at
least 100 x the reference's own fp32-vs-fp64 deviation of that quantity; margins and deviations are in the fixture
and re-checked here."""
import numpy as np
import pytest
import torch

from tests import maskctc_helpers as MH
from tests.helpers import golden, small_cfg

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(dev, blank):
    """The decoding model (ctc_lo scaled so the posteriors are peaky; `blank`: a bias that makes every frame blank)."""
    key = (str(dev), bool(blank))
    if key not in _MODELS:
        cfg = small_cfg("latest")
        model = MH.build_maskctc(cfg, dev, dropout=0.0)
        MH.load_params(model, MH.decode_params(cfg, blank=blank))
        _MODELS[key] = (cfg, model.eval())
    return _MODELS[key]


def _case(name):
    g = golden("maskctc_decode")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}


@pytest.mark.parametrize("name", list(MH.DECODE_CASES))
def test_decode_matches_reference_pass_by_pass(dev, name):
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    c = _case(name)
    spec = MH.DECODE_CASES[name]
    L, mask_num, passes = int(c["L"]), int(c["mask_num"]), int(c["passes"])
    # the case is what its name says, and its margins hold
    n_it = int(c["n_iterations"])
    assert n_it == spec["n_iterations"]
    assert {"ge": mask_num >= n_it, "lt": 0 < mask_num < n_it, "zero": mask_num == 0 and L > 0,
            "blank": L == 0}[spec["want"]]
    for m, d in (("argmax", "argmax"), ("prob", "prob"), ("top1", "logit"), ("topk", "logit")):
        assert float(c["margin_" + m]) >= 100.0 * float(c["dev_" + d]), (m, float(c["margin_" + m]), float(c["dev_" + d]))
    _, model = _model(dev, int(c["blank"]))
    inf = MaskCTCInference(model, n_iterations=n_it, threshold_probability=float(c["thr"]))
    trace = []
    hyp = inf(torch.from_numpy(c["enc"]).to(dev), trace=trace)
    assert (inf.last["L"], inf.last["mask_num"], inf.last["num_iter"]) == (L, mask_num, passes)
    got = [t.cpu().numpy() for t in trace]
    assert len(got) == (passes + 1 if L else 0)
    for t, row in enumerate(got):
        assert np.array_equal(row, c["rows"][t]), (t, row, c["rows"][t])
    assert np.array_equal(hyp.yseq.numpy(), c["yseq"])
    assert hyp.yseq[0] == hyp.yseq[-1] == model.mask_token


def test_prepared_memory_pass_equals_run_forward(dev):
    """One pass over the prepared memory (forward_masked) against MLMDecoder.run_forward on the same row, and both
    against the reference's fp64 logits of that pass: within max(2 e_ref, 1e-5)."""
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    c = _case("many")
    _, model = _model(dev, False)
    inf = MaskCTCInference(model, n_iterations=3, threshold_probability=float(c["thr"]))
    enc = torch.from_numpy(c["enc"]).to(dev)
    y = torch.from_numpy(c["rows"][0]).to(dev)
    mem = model.decoder.prepare_memory(enc.unsqueeze(0), [enc.shape[0]])
    a = inf._logits(y, enc, mem).cpu().double().numpy()
    b = inf._logits(y, enc, None).cpu().double().numpy()
    tol = max(2 * float(c["pred0_eref"]), 1e-5)
    ea, eb, d = np.abs(a - c["pred0_f64"]).max(), np.abs(b - c["pred0_f64"]).max(), np.abs(a - b).max()
    print(f"prepared {ea:.3e} run_forward {eb:.3e} between {d:.3e} e_ref {float(c['pred0_eref']):.3e} tol {tol:.3e}")
    assert a.shape == c["pred0_f64"].shape and ea <= tol and eb <= tol and d <= tol, (ea, eb, d, tol)


@pytest.mark.parametrize("name", ["many", "blank"])
def test_speech2text_returns_the_same_ids(dev, name):
    from espnet_slurp_amd.bin.asr_inference_maskctc import Speech2Text
    c = _case(name)
    cfg, model = _model(dev, int(c["blank"]))
    s2t = Speech2Text(model, n_iterations=int(c["n_iterations"]), threshold_probability=float(c["thr"]))
    out = s2t(MH.decode_speech(cfg, int(c["seed"])))
    assert len(out) == 1
    text, token, token_int, hyp = out[0]
    want = [int(t) for t in c["yseq"][1:-1] if t != 0]
    assert text is None and token_int == want and token == [model.token_list[i] for i in want]
    assert np.array_equal(hyp.yseq.numpy(), c["yseq"])
