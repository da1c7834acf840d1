"""Golden vectors for the block-synchronous beam search (simulated streaming decoding), generated in THIS container
with the reference's own BatchBeamSearchOnlineSim (espnet/nets/batch_beam_search_online_sim.py, imported through
refshim) on the reference encoder's output.  Writes tests/golden/stream_search.npz (data only).
Run:  python tests/golden/make_stream_search_golden.py

As shipped, the reference's CTCPrefixScorer has no extend_prob / extend_state, so its search never grows the CTC
scorer past the first window (it raises, or ends early).  The methods that do the work are in the reference
(CTCPrefixScoreTH.extend_prob / extend_state); ExtCTC below gives the scorer two delegating methods, which is what
the search's extend() looks for.  That is the behaviour recorded here.

Every case runs in fp32 and in fp64; the generator asserts that both give the same block trace and n-best lists
that agree under the n-best rule of tests/test_gpu_batch_beam.py.  The fp32 run (on the recorded fp32 encoder
output) is what is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import refshim  # noqa: E402

refshim.install()
from tests.golden.make_golden import build_reference, load_params, small_cfg  # noqa: E402
from tests.test_gpu_batch_beam import check_nbest  # noqa: E402

# tag: (speech seed, T, V, ctc_weight, beam, penalty, (block, hop, look-ahead))
CASES = {
    "a": (5, 400, 32, 0.3, 4, 0.0, (40, 16, 16)),
    "b": (7, 330, 32, 0.5, 6, 0.2, (40, 16, 16)),
    "c": (5, 400, 32, 1.0, 3, 0.0, (40, 16, 16)),
    "d": (9, 400, 32, 0.0, 4, 0.0, (40, 16, 16)),
    "e": (11, 400, 160, 0.3, 3, 0.0, (40, 16, 16)),
    "f": (13, 200, 32, 0.3, 4, 0.0, (16, 4, 4)),
    "g": (5, 100, 32, 0.3, 4, 0.0, (40, 16, 16)),
}


def run_case(tag, dtype):
    from espnet.nets.batch_beam_search_online_sim import BatchBeamSearchOnlineSim
    from espnet.nets.scorers.ctc import CTCPrefixScorer
    from espnet.nets.scorers.length_bonus import LengthBonus

    class ExtCTC(CTCPrefixScorer):
        def extend_prob(self, x):
            self.impl.extend_prob(self.ctc.log_softmax(x.unsqueeze(0)))

        def extend_state(self, state):
            return [self.impl.extend_state(s) for s in state]

    seed, T, V, ctc_w, beam, penalty, (bs, hop, la) = CASES[tag]
    cfg = small_cfg("latest", D=64, blocks=2, V=V)
    model = build_reference(cfg).to(dtype)
    load_params(model, cfg, 21, dtype)
    model.eval()
    speech = torch.randn(1, T, 80, generator=torch.Generator().manual_seed(seed)).to(dtype)
    with torch.no_grad():
        enc, _ = model.encode(speech, torch.tensor([T]))
    search = BatchBeamSearchOnlineSim(
        scorers=dict(decoder=model.decoder, ctc=ExtCTC(ctc=model.ctc, eos=model.eos), length_bonus=LengthBonus(V)),
        weights=dict(decoder=1.0 - ctc_w, ctc=ctc_w, length_bonus=penalty), beam_size=beam, vocab_size=V,
        sos=model.sos, eos=model.eos, token_list=None, pre_beam_score_key=None if ctc_w == 1.0 else "full")
    search.set_block_size(bs)
    search.set_hop_size(hop)
    search.set_look_ahead(la)
    trace, lens = [], []
    extend, step = search.extend, search.search

    def traced_extend(x, hyps):
        trace.append((int(x.shape[0]), len(hyps), int(hyps.yseq.shape[1])))
        return extend(x, hyps)

    def traced_search(hyps, x):
        lens.append(int(hyps.yseq.shape[1]))
        return step(hyps, x)

    search.extend, search.search = traced_extend, traced_search
    with torch.no_grad():
        hyps = search(x=enc[0], maxlenratio=0.0, minlenratio=0.0)
    # a rollback: the next search starts from a shorter prefix than the one before it
    rollbacks = sum(1 for a, b in zip(lens, lens[1:]) if b < a)
    return enc[0], hyps, trace, rollbacks


def extend_triple():
    """(lp, r_prev, r_new) of CTCPrefixScoreTH.extend_state: 3 hypotheses' states, grown from 24 to 40 frames."""
    from espnet.nets.ctc_prefix_score import CTCPrefixScoreTH
    rng = np.random.RandomState(3)
    T0, T1, V = 24, 40, 12
    lp = torch.log_softmax(torch.tensor(rng.randn(1, T1, V) * 2, dtype=torch.float32), -1)
    impl = CTCPrefixScoreTH(lp[:, :T0].clone(), torch.tensor([T0]), 0, V - 1)
    y = [torch.tensor([V - 1])]
    _, (r, log_psi, f_min, f_max, _) = impl(y, None, None)
    states = [(r[:, :, 0, c].clone(), log_psi[0, c].expand(V), f_min, f_max) for c in (3, 5, 7)]
    impl.extend_prob(lp.clone())
    grown = [impl.extend_state(s) for s in states]
    r_prev, r_new = torch.stack([s[0] for s in states]), torch.stack([s[0] for s in grown])
    assert r_prev.shape == (3, T0, 2) and r_new.shape == (3, T1, 2) and torch.equal(r_new[:, :T0], r_prev)
    return lp[0].numpy(), r_prev.numpy(), r_new.numpy()


def main():
    out = {}
    out["ext_lp"], out["ext_r_prev"], out["ext_r_new"] = extend_triple()
    moves, rolled, first_move = {}, 0, {}
    for tag in CASES:
        res = {}
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            res[name] = run_case(tag, dtype)
        enc, hyps, trace, rollbacks = res["f32"]
        _, hyps64, trace64, rollbacks64 = res["f64"]
        assert trace == trace64 and rollbacks == rollbacks64, (tag, trace, trace64)
        ys = [h.yseq.tolist() for h in hyps]
        ss = np.array([float(h.score) for h in hyps])
        ys64 = [h.yseq.tolist() for h in hyps64]
        ss64 = np.array([float(h.score) for h in hyps64])
        assert len(ys) == len(ys64) and len(ys) >= 1, (tag, len(ys), len(ys64))
        check_nbest(list(zip(ys, ss)), ys64, ss64, tag + " f32 vs f64")
        check_nbest(list(zip(ys64, ss64)), ys, ss, tag + " f64 vs f32")
        mat = np.full((len(ys), max(len(y) for y in ys)), -1, dtype=np.int64)
        for i, y in enumerate(ys):
            mat[i, : len(y)] = y
        seed, T, V, ctc_w, beam, penalty, sizes = CASES[tag]
        out[f"{tag}_enc"], out[f"{tag}_yseq"], out[f"{tag}_score"] = enc.numpy(), mat, ss
        out[f"{tag}_trace"] = np.array(trace, dtype=np.int64).reshape(-1, 3)
        out[f"{tag}_rollbacks"] = np.array(rollbacks)
        out[f"{tag}_cfg"] = np.array([ctc_w, beam, penalty, V, *sizes])
        moves[tag], rolled = len(trace) - 1, rolled + rollbacks
        first_move[tag] = trace[1][2] if len(trace) > 1 else 0
        print(tag, "trace", trace, "rollbacks", rollbacks, "n-best", len(ys), "best", len(ys[0]), "tokens, score",
              ss[0], "max rel f32/f64 score diff", float(np.max(np.abs(ss - ss64) / np.abs(ss64))))
    assert max(moves.values()) >= 3 and rolled >= 1 and max(first_move.values()) >= 8, (moves, rolled, first_move)
    assert moves["g"] == 0, moves
    np.savez_compressed(os.path.join(HERE, "stream_search.npz"), **out)
    print("wrote stream_search.npz")


if __name__ == "__main__":
    main()
