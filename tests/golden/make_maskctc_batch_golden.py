"""Batched Mask-CTC decoding fixture from the REFERENCE's own MaskCTCInference (needs the reference's sources, CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_maskctc_batch_golden.py [--check]

maskctc_decode_batch.npz   the reference decodes one utterance at a time, so a batch case is U reference runs, in
                     fp32 and fp64, under ONE (n_iterations, threshold), on recorded encoder outputs of the small
                     decoding model (maskctc_helpers.decode_params).  Per utterance <case>/<u>/...: what
                     maskctc_decode.npz records per case (encoder output, the token row after every pass, yseq, the
                     counts, the margins and the reference's own fp32-vs-fp64 deviations, pass 0's fp64 logits).

An utterance is kept under make_maskctc_golden.py's rule: the fp32 and fp64 rows are identical after every pass and
every decision margin is >= 100 x the reference's own fp32-vs-fp64 deviation of that quantity.

  mixed   n_iterations = 3, U = 5, inputs of 120 / 96 / 72 frames (29 / 23 / 17 encoder frames): utterances that need
          three, two, one and no pass, the longest not in first place.  mixed/blank_frame = (utterance, frame): the
          recorded frame whose greedy id is blank with the largest top-2 gap (a test builds an all-blank utterance
          from copies of it).
  blank   the blank-biased model, U = 2, two lengths, every L == 0.

--check: compare what this run computes with the committed file instead of writing it.

The fixture is data; nothing of the reference's code travels with it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_maskctc_golden as G  # noqa: E402  (installs the reference shim, sets the thread count)

from oracle import espnet_cpu as O  # noqa: E402
from tests import maskctc_helpers as MH  # noqa: E402
from tests.helpers import small_cfg  # noqa: E402

MARGIN = G.MARGIN
THRESHOLD = 0.65576
SEEDS = range(500, 516)
# case -> n_iterations, the model, and per slot (input frames, the pass plan wanted there)
BATCH_CASES = {
    "mixed": dict(n_iterations=3, blank=False,
                  slots=[(96, "lt"), (120, "ge4"), (72, "lt"), (72, "zero"), (120, "ge")]),
    "blank": dict(n_iterations=3, blank=True, slots=[(72, "blank"), (120, "blank")]),
}


def speech_of(cfg, frames, seed):
    """maskctc_helpers.decode_speech with another number of frames."""
    return O.synthetic_batch(1, frames, cfg.enc.input_size, cfg.vocab_size, [frames], [3], seed)[0][0]


def wanted(want, L, mask_num, passes, n_it):
    return {"ge4": mask_num >= max(4, n_it) and passes == n_it, "ge": mask_num >= n_it and passes == n_it,
            "lt": 0 < mask_num < n_it and passes == mask_num, "zero": L > 0 and mask_num == 0 and passes == 0,
            "blank": L == 0 and passes == 0}[want]


def decode_utterance(m32, m64, enc, n_it, thr):
    """One utterance through the reference in both precisions -> (its record, margins hold).  The margins are
    make_maskctc_golden.decode_case's."""
    mask = m64.mask_token
    lp32 = m32.ctc.log_softmax(enc.unsqueeze(0))[0].detach().numpy()
    lp64 = m64.ctc.log_softmax(enc.double().unsqueeze(0))[0].detach().numpy()
    toks, p64 = G.token_probs(lp64)
    toks32, p32 = G.token_probs(lp32.astype(np.float64))
    L = len(toks)
    if not np.array_equal(toks, toks32):
        return None, False
    y32, rows32, preds32, _ = G.run_reference_decode(m32, enc, n_it, thr)
    y64, rows64, preds64, _ = G.run_reference_decode(m64, enc.double(), n_it, thr)
    if not torch.equal(y32, y64) or len(rows32) != len(rows64) or any(
            not torch.equal(a, b) for a, b in zip(rows32, rows64)):
        return None, False
    dev = dict(argmax=float(np.abs(lp32 - lp64).max()), prob=0.0, logit=0.0)
    mar = dict(argmax=float(G.top2_gap(lp64).min()), prob=np.inf, top1=np.inf, topk=np.inf)
    if L:
        dev["prob"] = float(np.abs(p32 - p64).max())
        mar["prob"] = float(np.abs(p64 - thr).min())
    mask_num = int((rows64[0] == mask).sum()) if L and preds64 else 0
    num_iter = len(preds64)
    for t, (a, b) in enumerate(zip(preds32, preds64)):
        a, b = a.double().numpy(), b.numpy()
        midx = np.nonzero(rows64[t].numpy() == mask)[0]
        dev["logit"] = max(dev["logit"], float(np.abs(a - b)[midx].max()))
        sc = b[midx].max(-1)
        if t < num_iter - 1:  # a top-k pass: the chosen positions' top-1 gaps, and the k-th against the (k+1)-th
            k = mask_num // num_iter
            order = np.argsort(-sc)
            mar["top1"] = min(mar["top1"], float(G.top2_gap(b[midx[order[:k]]]).min()))
            if len(order) > k:
                mar["topk"] = min(mar["topk"], float(sc[order[k - 1]] - sc[order[k]]))
        else:
            mar["top1"] = min(mar["top1"], float(G.top2_gap(b[midx]).min()))
    ok = (mar["argmax"] >= MARGIN * dev["argmax"] and mar["prob"] >= MARGIN * dev["prob"]
          and mar["top1"] >= MARGIN * dev["logit"] and mar["topk"] >= MARGIN * dev["logit"])
    rec = {"enc": enc.numpy(), "yseq": y64.numpy(), "L": np.int64(L), "mask_num": np.int64(mask_num),
           "passes": np.int64(num_iter),
           "rows": (np.stack([r.numpy() for r in rows64]) if L else np.zeros((1, 0), dtype=np.int64)),
           "tok_prob": p32.astype(np.float32), "lp": lp32, "tokens": toks}
    for k, v in dev.items():
        rec[f"dev_{k}"] = np.float64(v)
    for k, v in mar.items():
        rec[f"margin_{k}"] = np.float64(v)
    if preds64:
        rec["pred0_f64"] = preds64[0].numpy()
        rec["pred0_eref"] = np.float64(np.abs(preds32[0].double().numpy() - preds64[0].numpy()).max())
    return rec, ok


def batch_case(name, spec, cfg, models):
    m32, m64 = models[spec["blank"]]
    n_it, thr = spec["n_iterations"], THRESHOLD
    out = {f"{name}/U": np.int64(len(spec["slots"])), f"{name}/thr": np.float64(thr),
           f"{name}/n_iterations": np.int64(n_it), f"{name}/blank": np.int64(spec["blank"]),
           f"{name}/frames": np.array([f for f, _ in spec["slots"]], dtype=np.int64)}
    used, recs, cache = set(), [], {}
    for u, (frames, want) in enumerate(spec["slots"]):
        for seed in SEEDS:
            if (frames, seed) in used:
                continue
            if (frames, seed) not in cache:
                speech = speech_of(cfg, frames, seed)
                with torch.no_grad():
                    enc64 = m64.encode(speech.double().unsqueeze(0), torch.tensor([frames]))[0][0]
                # the recorded encoder output: both precisions decode this
                cache[frames, seed] = decode_utterance(m32, m64, enc64.float(), n_it, thr)
            rec, ok = cache[frames, seed]
            if rec is None:
                continue
            L, mask_num, passes = int(rec["L"]), int(rec["mask_num"]), int(rec["passes"])
            hit = ok and wanted(want, L, mask_num, passes, n_it)
            print(f"{name}[{u}] {frames} frames seed {seed}: L {L} mask_num {mask_num} passes {passes} margins "
                  f"{'ok' if ok else 'short'} -> {'taken' if hit else 'no ' + want}", flush=True)
            if hit:
                used.add((frames, seed))
                out[f"{name}/{u}/seed"] = np.int64(seed)
                out.update({f"{name}/{u}/{k}": v for k, v in rec.items()})
                recs.append(rec)
                break
        else:
            raise RuntimeError(f"{name}[{u}]: no seed in {SEEDS} gives '{want}' at {frames} frames within the margins")
    if name == "mixed":  # the variety the case is for
        T = [r["enc"].shape[0] for r in recs]
        assert len(set(T)) == 3 and T[0] != max(T), T
        # a recorded frame whose greedy id is blank, the one with the largest top-2 gap
        best = max((float(G.top2_gap(r["lp"][t])), -u, -t) for u, r in enumerate(recs)
                   for t in range(r["lp"].shape[0]) if r["lp"][t].argmax() == 0)
        out[f"{name}/blank_frame"] = np.array([-best[1], -best[2]], dtype=np.int64)
        print(f"{name}: blank frame (utterance, frame) {out[name + '/blank_frame'].tolist()} top-2 gap {best[0]:.3f}")
    return out


def main():
    cfg = small_cfg("latest")
    models = {}
    for blank in (False, True):
        pair = []
        for dt in (torch.float32, torch.float64):
            m = G.build_reference(cfg).to(dt)
            G.load(m, MH.decode_params(cfg, dt, blank=blank))
            pair.append(m.eval())
        models[blank] = pair
    out = {}
    for name, spec in BATCH_CASES.items():
        out.update(batch_case(name, spec, cfg, models))
    path = os.path.join(HERE, "maskctc_decode_batch.npz")
    if "--check" in sys.argv[1:]:
        with np.load(path) as old:
            assert sorted(old.files) == sorted(out), sorted(set(old.files) ^ set(out))
            for k in out:
                a, b = np.asarray(out[k]), old[k]
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        print(f"{path}: reproduced, {len(out)} arrays")
    else:
        np.savez_compressed(path, **out)
        print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
