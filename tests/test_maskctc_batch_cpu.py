"""Batched Mask-CTC decoding, the parts that need no GPU: the fixture maskctc_decode_batch.npz is what its cases are
for (variety, margins), the pass plan restated in NumPy gives every utterance's recorded pass count, and the public
entry point exists."""
import numpy as np
import pytest

from tests.helpers import golden


def _batch(name):
    g = golden("maskctc_decode_batch")
    top = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/") and k.count("/") == 1}
    utts = [{k.split("/", 2)[2]: v for k, v in g.items() if k.startswith(f"{name}/{u}/")} for u in range(int(top["U"]))]
    return top, utts


def plan(mask_num, n_iterations):
    """maskctc_model.py:319-323: (num_iter, positions filled per pass but the last)."""
    num_iter = n_iterations if mask_num >= n_iterations and n_iterations > 0 else mask_num
    return num_iter, (mask_num // num_iter if num_iter else 0)


def test_mixed_case_has_the_variety_it_is_for():
    top, utts = _batch("mixed")
    n_it = int(top["n_iterations"])
    assert n_it == 3 and int(top["U"]) == len(utts) == 5 and int(top["blank"]) == 0
    assert top["frames"].tolist() == [96, 120, 72, 72, 120]
    T = [c["enc"].shape[0] for c in utts]
    assert sorted(set(T)) == [17, 23, 29] and T[0] != max(T)  # all three lengths, the longest not in first place
    nums = [int(c["mask_num"]) for c in utts]
    assert any(n >= 4 and plan(n, n_it) == (3, n // 3) and n // 3 >= 1 for n in nums)
    assert any(0 < n < 3 for n in nums) and any(n == 0 and int(c["L"]) > 0 for n, c in zip(nums, utts))
    assert all(int(c["L"]) > 0 for c in utts)
    assert len({(int(f), int(c["seed"])) for f, c in zip(top["frames"], utts)}) == 5  # five different inputs
    bu, bt = (int(v) for v in top["blank_frame"])
    lp = utts[bu]["lp"][bt]
    assert lp.argmax() == 0
    gap = np.sort(lp)[-1] - np.sort(lp)[-2]
    for c in utts:  # no recorded blank frame has a larger top-2 gap
        s = np.sort(c["lp"][c["lp"].argmax(-1) == 0], axis=-1)
        assert (s[:, -1] - s[:, -2] <= gap).all()
    assert gap >= 100.0 * max(float(c["dev_argmax"]) for c in utts)


def test_blank_case_is_all_blank_at_two_lengths():
    top, utts = _batch("blank")
    assert int(top["U"]) == len(utts) == 2 and int(top["blank"]) == 1
    assert len({c["enc"].shape[0] for c in utts}) == 2
    for c in utts:
        assert int(c["L"]) == int(c["mask_num"]) == int(c["passes"]) == 0
        assert c["rows"].shape == (1, 0) and c["yseq"].tolist() == [32, 32]
        assert (c["lp"].argmax(-1) == 0).all()


@pytest.mark.parametrize("name", ["mixed", "blank"])
def test_margins_hold_and_the_plan_gives_the_recorded_passes(name):
    top, utts = _batch(name)
    n_it, thr, mask = int(top["n_iterations"]), float(top["thr"]), 32
    for u, c in enumerate(utts):
        for m, d in (("argmax", "argmax"), ("prob", "prob"), ("top1", "logit"), ("topk", "logit")):
            assert float(c["margin_" + m]) >= 100.0 * float(c["dev_" + d]), (u, m)
        L, mask_num, passes = int(c["L"]), int(c["mask_num"]), int(c["passes"])
        assert c["tok_prob"].shape == (L,) and c["tokens"].shape == (L,)
        masked = c["tok_prob"].astype(np.float64) < thr
        assert int(masked.sum()) == mask_num
        assert plan(mask_num, n_it)[0] == passes
        assert c["rows"].shape == (passes + 1, L)
        assert np.array_equal(c["yseq"], np.concatenate([[mask], c["rows"][-1], [mask]]))
        if L:
            assert np.array_equal(c["rows"][0], np.where(masked, mask, c["tokens"]))
        k = plan(mask_num, n_it)[1]
        for t in range(passes):  # every pass but the last fills k positions; the last one every position left
            left = int((c["rows"][t + 1] == mask).sum())
            assert left == (mask_num - (t + 1) * k if t < passes - 1 else 0), (u, t, left)
        assert ("pred0_f64" in c) == (passes > 0)
        if passes:
            assert c["pred0_f64"].shape == (L, mask + 1)


@pytest.mark.parametrize("mask_num,n_it,want", [(0, 3, (0, 0)), (1, 3, (1, 1)), (2, 3, (2, 1)), (3, 3, (3, 1)),
                                                (4, 3, (3, 1)), (7, 3, (3, 2)), (5, 0, (5, 1)), (5, 1, (1, 5)),
                                                (0, 0, (0, 0))])
def test_plan_arithmetic(mask_num, n_it, want):
    assert plan(mask_num, n_it) == want


def test_speech2text_has_decode_batch_and_refuses_an_empty_list():
    from espnet_slurp_amd.asr.decoder.mlm_decoder import MLMDecoder
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    from espnet_slurp_amd.bin.asr_inference_maskctc import Speech2Text
    assert callable(getattr(Speech2Text, "decode_batch", None))
    assert callable(getattr(MaskCTCInference, "forward_batch", None))
    assert callable(getattr(MLMDecoder, "forward_masked_batch", None))
    s2t = Speech2Text.__new__(Speech2Text)  # the check comes before anything that needs a model or a device
    with pytest.raises(ValueError, match="empty"):
        s2t.decode_batch([])
