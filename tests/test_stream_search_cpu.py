"""The block-synchronous search's host side: the window schedule, the setters and Speech2Text's signature.  (The
search itself runs on the GPU: tests/test_gpu_stream_search.py.)"""
import inspect

import pytest

from tests.helpers import golden

# T', (block, hop, look-ahead) -> every window the schedule can reach, by hand
SCHEDULES = [
    (99, (40, 16, 16), [24, 40, 56, 72, 99]),   # 72 + 16 + 16 = 104 >= 99: the jump to T
    (81, (40, 16, 16), [24, 40, 56, 81]),
    (49, (16, 4, 4), [12, 16, 20, 24, 28, 32, 36, 40, 44, 49]),  # 40 + 8 = 48 < 49, 44 + 8 >= 49
    (24, (40, 16, 16), [24]),                   # the first window covers the utterance
    (25, (40, 16, 16), [24, 25]),
    (57, (40, 16, 16), [24, 40, 57]),           # 24 + 32 = 56 < 57; 40 + 32 >= 57
    (99, (40, 0, 16), [99]),                    # a size of zero: one window
    (99, (None, 16, 16), [99]),
    (13, (8, 3, 3), [5, 8, 13]),
]


def _windows(T, sizes):
    from espnet_slurp_amd.asr.beam_search import first_window, next_window
    out = [first_window(T, *sizes)]
    while out[-1] < T:
        out.append(next_window(out[-1], T, sizes[1], sizes[2]))
        assert out[-1] > out[-2]
    return out


@pytest.mark.parametrize("T,sizes,want", SCHEDULES)
def test_window_schedule(T, sizes, want):
    assert _windows(T, sizes) == want


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f", "g"])
def test_window_schedule_against_the_recorded_traces(tag):
    g = golden("stream_search")
    sizes = tuple(int(v) for v in g[f"{tag}_cfg"][4:7])
    T = g[f"{tag}_enc"].shape[0]
    trace = g[f"{tag}_trace"]
    # the reference moved at every boundary in these cases, so its trace walks the whole schedule
    assert trace[:, 0].tolist() == _windows(T, sizes)
    assert trace[0, 1:].tolist() == [1, 1]


def test_setters_and_restrictions():
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearch, BatchBeamSearchOnlineSim, LengthBonus
    kw = dict(scorers=dict(length_bonus=LengthBonus()), weights=dict(length_bonus=1.0), beam_size=2, vocab_size=8,
              sos=7, eos=7)
    bs = BatchBeamSearchOnlineSim(**kw)
    assert isinstance(bs, BatchBeamSearch)
    assert (bs.block_size, bs.hop_size, bs.look_ahead) == (None, None, None) and bs.block_trace == []
    bs.set_block_size(40)
    bs.set_hop_size(16)
    bs.set_look_ahead(8)
    assert (bs.block_size, bs.hop_size, bs.look_ahead) == (40, 16, 8)
    with pytest.raises(ValueError):
        bs.forward_batch(None, [1])
    with pytest.raises(ValueError):
        BatchBeamSearchOnlineSim(**dict(kw, scorers=dict(lm=object()), weights=dict(lm=1.0)))


def test_speech2text_signature():
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    p = inspect.signature(Speech2Text.__init__).parameters
    assert p["streaming"].default is False and p["batch_search"].default is False


def test_fixture_covers_what_it_claims():
    g = golden("stream_search")
    moves = {t: len(g[f"{t}_trace"]) - 1 for t in "abcdefg"}
    assert max(moves.values()) >= 3 and moves["g"] == 0
    assert sum(int(g[f"{t}_rollbacks"]) for t in "abcdefg") >= 1
    assert max(int(g[f"{t}_trace"][1, 2]) for t in "abcdef") >= 8
    assert g["ext_r_prev"].shape == (3, 24, 2) and g["ext_r_new"].shape == (3, 40, 2)
