"""Decode timing: Mask-CTC mask-predict (MaskCTCInference) against the batch beam search, one utterance.

The C2 decode shape of tools/bench_decode.py (80 x 1500 input -> encoder output T' = 374, D = 256; 6 decoder layers;
V = 600) with seeded random weights.  One encoder output serves both sides: the Mask-CTC model's (its CTC's blank bias
is raised so that greedy CTC leaves about TOKENS tokens, as a trained model would; random posteriors change symbol
every frame).  The threshold is placed so that about a third of the tokens are masked; n_iterations = 10.  The
other side is Speech2Text(batch_search=True)'s BatchBeamSearch (beam 20, ctc_weight 0.1, 29 output steps) of a
CTC/attention model of the same shape on that encoder output.

    python tools/bench_maskctc_decode.py [--repeat 5] [--out profiles/r17a_maskctc_decode.json]

The two decoders are timed alternately, --repeat times each (wall time, synchronised on both sides); the record
holds every repeat, the median and the spread (max - min).  ms per refinement pass is the difference between the
n_iterations = 10 and the n_iterations = 1 decode of the same utterance over the passes that differ.  launcher calls
per pass counts the native launcher calls of one pass (a launcher may enqueue more than one kernel, e.g. a split GEMM).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FRAMES, T_ENC, BEAM, CTC_WEIGHT, MAXLENRATIO, TOKENS, N_ITER = 1500, 374, 20, 0.1, 0.08, 24, 10


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
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from tests.helpers import build_model, c2_cfg
    from tests.maskctc_helpers import build_maskctc

    if not torch.cuda.is_available():
        raise SystemExit("bench_maskctc_decode.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc = build_maskctc(c2_cfg(), dev, dropout=0.0).eval()
    torch.manual_seed(1)
    ar = build_model(c2_cfg(), dev, dropout=0.0).eval()
    speech = torch.from_numpy(np.random.RandomState(1).randn(1, T_FRAMES, 80).astype(np.float32)).to(dev)
    lengths = torch.tensor([T_FRAMES])
    with torch.no_grad():
        enc = mc.encode(speech, lengths, sl_cpu=lengths)[0][0].contiguous()
        # blank bias: all but about TOKENS frames become blank
        logits = mc.ctc.logits(enc)
        lead = (logits[:, 1:].max(-1).values - logits[:, 0]).sort().values
        mc.ctc.ctc_lo.bias.data[0] += float(0.5 * (lead[-TOKENS - 1] + lead[-TOKENS]))
        _, _, tok_prob, counts = K.maskctc_init(mc.ctc.log_softmax(enc.unsqueeze(0))[0], mc.mask_token, 0.0)
        L = int(counts[0])
        p = tok_prob[:L].sort().values
        thr = float(0.5 * (p[L // 3 - 1] + p[L // 3]))  # a third of the tokens below it
    inf10 = MaskCTCInference(mc, n_iterations=N_ITER, threshold_probability=thr)
    inf1 = MaskCTCInference(mc, n_iterations=1, threshold_probability=thr)
    search = Speech2Text(ar, beam_size=BEAM, ctc_weight=CTC_WEIGHT, nbest=1, maxlenratio=MAXLENRATIO,
                         batch_search=True).beam_search
    sides = {"maskctc_n10": lambda: inf10(enc), "maskctc_n1": lambda: inf1(enc),
             "batch_search": lambda: search.forward(enc, MAXLENRATIO, 0.0)}
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    ms = {k: [] for k in sides}
    for _ in range(args.repeat):  # alternated
        for k, fn in sides.items():
            ms[k].append(_timed(fn)[0])
    passes10, passes1, mask_num = inf10.last["num_iter"], inf1.last["num_iter"], inf10.last["mask_num"]
    # native launcher calls of one decode, and of one pass
    calls = {"n": 0}
    orig = _native.call

    def counting(name, *a):
        calls["n"] += 1
        return orig(name, *a)
    _native.call = counting
    try:
        inf10(enc)
        c10 = calls["n"]
        calls["n"] = 0
        inf1(enc)
        c1 = calls["n"]
    finally:
        _native.call = orig
    steps = getattr(search, "steps", None) or int(MAXLENRATIO * T_ENC)
    med = {k: statistics.median(v) for k, v in ms.items()}
    record = {
        "tool": "tools/bench_maskctc_decode.py", "shape": {"T_enc": int(enc.shape[0]), "D": int(enc.shape[1]),
                                                            "decoder_layers": 6, "V": 600},
        "tokens": L, "mask_num": mask_num, "threshold_probability": thr, "n_iterations": N_ITER, "passes": passes10,
        "repeat": args.repeat, "maskctc_n10": _summary(ms["maskctc_n10"]), "maskctc_n1": _summary(ms["maskctc_n1"]),
        "batch_search": dict(_summary(ms["batch_search"]), beam=BEAM, steps=steps,
                             ms_per_step=round(med["batch_search"] / steps, 3)),
        "maskctc_ms_per_utt": round(med["maskctc_n10"], 3),
        "maskctc_ms_per_pass": round((med["maskctc_n10"] - med["maskctc_n1"]) / max(1, passes10 - passes1), 3),
        "launcher_calls_per_decode": c10, "launcher_calls_per_pass": (c10 - c1) // max(1, passes10 - passes1),
        "batch_search_over_maskctc": round(med["batch_search"] / med["maskctc_n10"], 2),
    }
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
