"""Block-synchronous beam search (BatchBeamSearchOnlineSim), its two kernels and Speech2Text(streaming=True).

Reference part: tests/golden/stream_search.npz (tests/golden/make_stream_search_golden.py): the reference's
BatchBeamSearchOnlineSim, its CTC scorer given the extend_prob / extend_state delegation it lacks as shipped, on the
reference encoder's output of seeded noise, cases a-g.  Per case the search here runs on the recorded encoder output
and must give the recorded block trace, an n-best list that passes check_nbest of tests/test_gpu_batch_beam.py
(allowance 1e-3, the fp32 search's gate; the reference's own fp32 and fp64 runs agree to 6e-7) and the recorded best
tokens.

What the random-weight fixtures reach: a randomly initialised model repeats a token at once, so between the first
move and the last block each block advances one step and takes it back; deep decoding (up to maxlen in cases d and
e) happens in the last block, on CTC states and a K/V cache that went through every extension and rollback.  They do
not show a search that advances several steps in a middle block.

Kernel parts: esp_ctc_prefix_extend against CTCPrefixScoreTH.extend_state's recorded states (same inputs, same
order of fp32 adds: exact) and against the rule restated in numpy; DecoderCache.reorder_keep / rollback against
torch indexing (copies: exact)."""
import numpy as np
import pytest
import torch

from tests.helpers import build_model, golden, load_seeded, small_cfg
from tests.test_gpu_batch_beam import check_nbest

pytestmark = pytest.mark.gpu

CASES = ["a", "b", "c", "d", "e", "f", "g"]
LOGZERO = np.float32(-10000000000.0)
_models = {}


def _model(dev, V):
    if V not in _models:
        cfg = small_cfg("latest", D=64, blocks=2, V=V)
        model = build_model(cfg, dev, dropout=0.0)
        load_seeded(model, cfg, 21)
        model.eval()
        _models[V] = model
    return _models[V]


def _search(model, ctc_w, beam, penalty, V, sizes):
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearchOnlineSim, CTCPrefixScorer, DecoderScorer, LengthBonus
    bs = BatchBeamSearchOnlineSim(
        scorers=dict(decoder=DecoderScorer(model.decoder),
                     ctc=CTCPrefixScorer(model.ctc, eos=model.eos, blank=model.blank_id), length_bonus=LengthBonus()),
        weights=dict(decoder=1.0 - ctc_w, ctc=ctc_w, length_bonus=penalty), beam_size=beam, vocab_size=V,
        sos=model.sos, eos=model.eos, pre_beam_score_key=None if ctc_w == 1.0 else "full")
    if sizes is not None:
        bs.set_block_size(sizes[0])
        bs.set_hop_size(sizes[1])
        bs.set_look_ahead(sizes[2])
    return bs


# ------------------------------------------------------------------------------------------------ extend kernel
def _extend_np(lp, r, t_old, t_new, blank):
    r = r.copy()
    for t in range(max(t_old, 1), t_new):
        r[:, t, 0] = LOGZERO
        r[:, t, 1] = r[:, t - 1, 1] + lp[t, blank]  # fp32 adds, frame order
    return r


def test_ctc_prefix_extend_equals_the_reference_states(dev):
    from espnet_slurp_amd import kernels as K
    g = golden("stream_search")
    lp, r_prev, want = g["ext_lp"], g["ext_r_prev"], g["ext_r_new"]
    assert lp.shape == (40, 12) and r_prev.shape == (3, 24, 2) and want.shape == (3, 40, 2)
    r = torch.full((3, 40, 2), 7.0, dtype=torch.float32)
    r[:, :24] = torch.from_numpy(r_prev)
    r = r.to(dev)
    K.ctc_prefix_extend(torch.from_numpy(lp).unsqueeze(0).to(dev), torch.zeros(3, dtype=torch.int32, device=dev), r,
                        24, 40, 0)
    assert np.array_equal(r.cpu().numpy(), want)


@pytest.mark.parametrize("t_old,t_new", [(24, 40), (24, 24), (1, 40), (0, 5), (39, 40), (7, 23)])
def test_ctc_prefix_extend_sweep(dev, t_old, t_new):
    """NH=3 states of Tmax=40 frames, V=12, two utterances; rows outside [max(t_old, 1), t_new) keep their bits."""
    from espnet_slurp_amd import kernels as K
    rng = np.random.RandomState(11)
    lp = np.log(rng.dirichlet(np.ones(12), size=(2, 40))).astype(np.float32)
    r0 = (rng.randn(3, 40, 2) * 5 - 20).astype(np.float32)
    utt = np.array([1, 0, 1], dtype=np.int32)
    blank = 2
    want = r0.copy()
    for h in range(3):
        want[h:h + 1] = _extend_np(lp[utt[h]], r0[h:h + 1], t_old, t_new, blank)
    r = torch.from_numpy(r0).to(dev)
    K.ctc_prefix_extend(torch.from_numpy(lp).to(dev), torch.from_numpy(utt).to(dev), r, t_old, t_new, blank)
    got = r.cpu().numpy()
    lo = max(t_old, 1)
    assert np.array_equal(got[:, :lo].view(np.uint32), r0[:, :lo].view(np.uint32))
    assert np.array_equal(got[:, t_new:].view(np.uint32), r0[:, t_new:].view(np.uint32))
    assert np.array_equal(got, want)
    if t_old == t_new:
        assert np.array_equal(got.view(np.uint32), r0.view(np.uint32))


# -------------------------------------------------------------------------------------------------- cache gather
def _filled_cache(dev, seed, rows=5, capacity=8, length=7):
    from espnet_slurp_amd.asr.decoder.transformer_decoder import DecoderCache
    c = DecoderCache(2, 16, dev, rows=rows, capacity=capacity)
    g = torch.Generator().manual_seed(seed)
    c.buf.copy_(torch.randn(c.buf.shape, generator=g))
    c.len = length
    return c


def _append(c, n, g):
    """What a decoder step does to the cache: room for one more position, write it, count it."""
    c.ensure(n, c.len + 1)
    new = torch.randn(2, n, 32, generator=g)
    c.buf[:, :n, c.len] = new.to(c.buf.device)
    c.len += 1
    return new


def test_cache_reorder_keep_and_rollback(dev):
    index = [3, 3, 0, 4, 1, 1]  # repeats, and longer than the 5 rows in use
    c = _filled_cache(dev, 1)
    before = c.buf.clone()
    old_buf = c.buf
    c.reorder_keep(index)
    assert (c.n, c.len) == (6, 7) and c.row_capacity >= 6
    assert torch.equal(c.buf[:, :6, :7], before[:, index, :7])
    assert torch.equal(old_buf, before)  # the source rows survive
    c.rollback()
    assert c.buf is old_buf and (c.n, c.len) == (5, 6) and torch.equal(c.buf, before)
    with pytest.raises(RuntimeError):
        c.rollback()  # one step of history only


def test_cache_growth_keeps_the_history_and_steps_do_not_allocate(dev):
    index = [3, 3, 0, 4, 1, 1]
    c = _filled_cache(dev, 2)
    before = c.buf.clone()
    g = torch.Generator().manual_seed(3)
    c.reorder_keep(index)
    p7 = _append(c, 6, g)  # len 7 -> 8: fits
    assert c.capacity == 8
    p8 = _append(c, 6, g)  # len 8 -> 9: the live buffer grows, the kept one stays
    assert c.capacity == 16 and c.len == 9
    assert torch.equal(c.buf[:, :6, :7], before[:, index, :7])
    assert torch.equal(c.buf[:, :6, 7].cpu(), p7) and torch.equal(c.buf[:, :6, 8].cpu(), p8)
    live = c.buf.clone()
    c.reorder_keep([5, 0, 0, 2])
    assert (c.n, c.len) == (4, 9) and torch.equal(c.buf[:, :4, :9], live[:, [5, 0, 0, 2], :9])
    bufs = {c.buf.data_ptr(), c.alt.data_ptr()}
    for step in range(4):  # capacity reached: the two buffers only swap
        _append(c, 4, g)
        c.reorder_keep([1, 0, 3, 2])
        assert {c.buf.data_ptr(), c.alt.data_ptr()} == bufs
    c.rollback()
    assert (c.n, c.len) == (4, 12)
    # history across growth: back to the rows of before the first reorder_keep of a fresh cache
    c = _filled_cache(dev, 2)
    c.reorder_keep(index)
    _append(c, 6, g)
    _append(c, 6, g)
    c.rollback()
    assert (c.n, c.len) == (5, 6) and torch.equal(c.buf, before)


def test_reorder_is_unaffected(dev):
    index = [3, 3, 0, 4, 1, 1]
    a, b = _filled_cache(dev, 4), _filled_cache(dev, 4)
    before = a.buf.clone()
    a.reorder(index)
    b.reorder_keep(index)
    assert a.alt is None and a.hist is None and (a.n, a.len) == (6, 7)
    assert torch.equal(a.buf[:, :6, :7], before[:, index, :7]) and torch.equal(a.buf[:, :6, :7], b.buf[:, :6, :7])


def test_prepared_memory_window(dev):
    model = _model(dev, 32)
    xs = torch.randn(1, 30, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    mem = model.decoder.prepare_memory(xs, [30])
    rows = np.zeros(3, dtype=np.int32)
    assert mem.index(rows).host[1].tolist() == [30, 30, 30]
    mem.set_window(12)
    assert mem.index(rows).host[1].tolist() == [12, 12, 12]
    with pytest.raises(ValueError):
        mem.set_window(31)


# -------------------------------------------------------------------------------------------------------- search
@pytest.mark.parametrize("tag", CASES)
def test_search_matches_reference(dev, tag):
    g = golden("stream_search")
    ctc_w, beam, penalty, V, block, hop, la = g[f"{tag}_cfg"]
    V, beam = int(V), int(beam)
    model = _model(dev, V)
    bs = _search(model, float(ctc_w), beam, float(penalty), V, (int(block), int(hop), int(la)))
    assert ("decoder" in bs.full_scorers) == (ctc_w != 1.0) and ("ctc" in bs.part_scorers) == (ctc_w != 0.0)
    nbest = bs.forward(torch.from_numpy(g[f"{tag}_enc"]).to(dev))
    want_trace = [tuple(int(v) for v in row) for row in g[f"{tag}_trace"]]
    want_y = [y[y >= 0].tolist() for y in g[f"{tag}_yseq"]]
    want_s = g[f"{tag}_score"]
    got = [(h.yseq.tolist(), h.score) for h in nbest]
    print(f"{tag}: trace {bs.block_trace} rollbacks {bs.rollbacks} steps {bs.steps} n-best {len(got)} "
          f"(want {len(want_s)})")
    for i, (y, s) in enumerate(got[:len(want_s)]):
        print(f"{tag} rank {i + 1}: score {s:.5f} want {want_s[i]:.5f} same tokens {y == want_y[i]}")
    assert bs.block_trace == want_trace
    assert bs.rollbacks == int(g[f"{tag}_rollbacks"])
    check_nbest(got, want_y, want_s, tag)
    assert got[0][0] == want_y[0]
    assert len(got) == len(want_y)


def test_restrictions(dev):
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearchOnlineSim, LengthBonus
    model = _model(dev, 32)
    bs = _search(model, 0.3, 4, 0.0, 32, None)
    with pytest.raises(ValueError):
        bs.forward_batch(torch.zeros(1, 8, 64, device=dev), [8])
    with pytest.raises(ValueError):
        BatchBeamSearchOnlineSim(scorers=dict(lm=object(), length_bonus=LengthBonus()),
                                 weights=dict(lm=0.5, length_bonus=0.0), beam_size=2, vocab_size=32, sos=31, eos=31)


# --------------------------------------------------------------------------------------------------- Speech2Text
def _same(res_a, res_b):
    assert len(res_a) == len(res_b) >= 1
    for a, b in zip(res_a, res_b):
        assert a[2] == b[2] and a[3].yseq.tolist() == b[3].yseq.tolist() and a[3].score == b[3].score


def test_speech2text_streaming_on_the_block_encoder(dev):
    from espnet_slurp_amd.asr.beam_search import BatchBeamSearchOnlineSim
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from tests.test_gpu_cbt import _model as cbt_model
    model, g = cbt_model(dev)
    speech = torch.from_numpy(g["speech"][0][: int(g["speech_lengths"][0])])
    s2t = Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=100, streaming=True)
    assert isinstance(s2t.beam_search, BatchBeamSearchOnlineSim)
    enc = model.encoder
    assert (s2t.beam_search.block_size, s2t.beam_search.hop_size, s2t.beam_search.look_ahead) == \
        (enc.block_size, enc.hop_size, enc.look_ahead) == (8, 3, 3)
    res = s2t(speech)
    trace = list(s2t.beam_search.block_trace)
    print(f"block encoder: trace {trace}")
    assert trace[0][0] == 5 and trace[-1][0] == 13 and len(trace) >= 2
    direct = _search(model, 0.3, 4, 0.0, len(s2t.token_list), (8, 3, 3))
    hyps = direct.forward(s2t.encode(speech))
    assert direct.block_trace == trace
    assert [(h.yseq.tolist(), h.score) for h in hyps] == [(r[3].yseq.tolist(), r[3].score) for r in res]
    with pytest.raises(ValueError):
        s2t.decode_batch([speech.numpy()])


def test_speech2text_streaming_on_the_conformer_is_one_window(dev):
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model = _model(dev, 32)
    speech = torch.randn(100, 80, generator=torch.Generator().manual_seed(5))
    s2t = Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=3, streaming=True)
    assert s2t.beam_search.block_size is None
    res = s2t(speech)
    assert len(res) >= 1 and s2t.beam_search.block_trace == [(24, 1, 1)]
    with pytest.raises(ValueError):
        Speech2Text(model, beam_size=4, ctc_weight=0.3, lm=object(), streaming=True)
    # streaming=False is today's behaviour, for the plain and the batch search
    for kw in (dict(), dict(batch_search=True)):
        _same(Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=3, streaming=False, **kw)(speech),
              Speech2Text(model, beam_size=4, ctc_weight=0.3, nbest=3, **kw)(speech))
