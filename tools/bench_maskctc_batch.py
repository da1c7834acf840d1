"""Decode timing: batched Mask-CTC mask-predict (MaskCTCInference.forward_batch, the search part of
asr_inference_maskctc.Speech2Text.decode_batch) against U sequential MaskCTCInference.forward calls on the same
encoder outputs.

The C2 decode shape of tools/bench_maskctc_decode.py (80 x 1500 input -> encoder output T' = 374, D = 256; 6 decoder
layers; V = 600) with seeded random weights, and its token and mask counts: the CTC's blank bias is raised so that
greedy CTC leaves about TOKENS tokens per utterance, and the threshold is placed so that about a third of all tokens
are masked; n_iterations = 10.  32 seeded inputs go through one padded-batch encode; a batch of U takes the first U.

    python tools/bench_maskctc_batch.py [--repeat 5] [--out profiles/<tag>_maskctc_batch.json]

For each U in {1, 8, 32} the two sides are timed alternately, --repeat times each (wall time, synchronised on both
sides); the record holds every repeat, the median and the spread (max - min), utterances per second, and whether
both sides returned the same hypotheses.  ms per pass is the difference between the n_iterations = 10 and the
n_iterations = 1 decode of the same utterances over the passes that differ: the batch runs max(num_iter) passes, the
sequential loop sum(num_iter).  launcher calls per pass counts the native launcher calls of one batched pass.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FRAMES, TOKENS, N_ITER, U_MAX, BATCHES = 1500, 24, 10, 32, (1, 8, 32)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _summary(ms):
    return {"runs_ms": [round(v, 3) for v in ms], "median_ms": round(statistics.median(ms), 3),
            "spread_ms": round(max(ms) - min(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from espnet_slurp_amd import _native
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCInference
    from tests.helpers import c2_cfg
    from tests.maskctc_helpers import build_maskctc

    if not torch.cuda.is_available():
        raise SystemExit("bench_maskctc_batch.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc = build_maskctc(c2_cfg(), dev, dropout=0.0).eval()
    speech = torch.from_numpy(np.random.RandomState(1).randn(U_MAX, T_FRAMES, 80).astype(np.float32)).to(dev)
    lengths = torch.full((U_MAX,), T_FRAMES, dtype=torch.int64)
    with torch.no_grad():
        enc, enc_lens = mc.encode(speech, lengths, sl_cpu=lengths)
        enc = enc.contiguous()
        lens = [int(t) for t in enc_lens]
        # blank bias: all but about TOKENS frames per utterance become blank
        logits = mc.ctc.logits(enc.reshape(-1, enc.shape[-1]))
        lead = (logits[:, 1:].max(-1).values - logits[:, 0]).sort().values
        n = TOKENS * U_MAX
        mc.ctc.ctc_lo.bias.data[0] += float(0.5 * (lead[-n - 1] + lead[-n]))
        tl = K.h2d(torch.tensor(lens, dtype=torch.int32), dev)
        _, _, tok_prob, counts = K.maskctc_init_batch(mc.ctc.log_softmax(enc), tl, mc.mask_token, 0.0, N_ITER)
        Ls = counts[:, 0].cpu().tolist()
        p = torch.cat([tok_prob[u, :L] for u, L in enumerate(Ls)]).sort().values
        thr = float(0.5 * (p[len(p) // 3 - 1] + p[len(p) // 3]))  # a third of the tokens below it
    inf10 = MaskCTCInference(mc, n_iterations=N_ITER, threshold_probability=thr)
    inf1 = MaskCTCInference(mc, n_iterations=1, threshold_probability=thr)
    record = {"tool": "tools/bench_maskctc_batch.py",
              "shape": {"T_enc": int(enc.shape[1]), "D": int(enc.shape[2]), "decoder_layers": 6, "V": 600},
              "threshold_probability": thr, "n_iterations": N_ITER, "repeat": args.repeat, "batches": {}}
    for U in BATCHES:
        e, el = enc[:U].contiguous(), lens[:U]
        rows = [e[u, :el[u]].contiguous() for u in range(U)]
        sides = {"batch_n10": lambda: inf10.forward_batch(e, el), "sequential_n10": lambda: [inf10(r) for r in rows],
                 "batch_n1": lambda: inf1.forward_batch(e, el), "sequential_n1": lambda: [inf1(r) for r in rows]}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        ms = {k: [] for k in sides}
        outs = {}
        for _ in range(args.repeat):  # alternated
            for k, fn in sides.items():
                t, outs[k] = _timed(fn)
                ms[k].append(t)
        same = all(torch.equal(a.yseq, b.yseq) for a, b in zip(outs["batch_n10"], outs["sequential_n10"]))
        plan10, plan1 = list(inf10.last_batch), list(inf1.last_batch)  # the batched runs' plans
        passes10, passes1 = [d["num_iter"] for d in plan10], [d["num_iter"] for d in plan1]
        calls = {"n": 0}
        orig = _native.call

        def counting(name, *a):
            calls["n"] += 1
            return orig(name, *a)
        _native.call = counting
        try:
            inf10.forward_batch(e, el)
            c10 = calls["n"]
            calls["n"] = 0
            inf1.forward_batch(e, el)
            c1 = calls["n"]
        finally:
            _native.call = orig
        med = {k: statistics.median(v) for k, v in ms.items()}
        dpass_b = max(1, max(passes10) - max(passes1))
        dpass_s = max(1, sum(passes10) - sum(passes1))
        record["batches"][str(U)] = {
            "tokens": [d["L"] for d in plan10], "mask_num": [d["mask_num"] for d in plan10], "passes": passes10,
            "batch_passes": max(passes10), "sequential_passes": sum(passes10),
            **{k: _summary(v) for k, v in ms.items()},
            "batch_utt_per_s": round(U * 1e3 / med["batch_n10"], 1),
            "sequential_utt_per_s": round(U * 1e3 / med["sequential_n10"], 1),
            "batch_ms_per_pass": round((med["batch_n10"] - med["batch_n1"]) / dpass_b, 3),
            "sequential_ms_per_pass": round((med["sequential_n10"] - med["sequential_n1"]) / dpass_s, 3),
            "batch_launcher_calls_per_decode": c10, "batch_launcher_calls_per_pass": (c10 - c1) // dpass_b,
            "sequential_over_batch": round(med["sequential_n10"] / med["batch_n10"], 2),
            "same_hypotheses": bool(same),
        }
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
