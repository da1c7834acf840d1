"""Decode timing: the plain Speech2Text search against the batch search on the cached one-step decoder.

The C2 model shape (80 x 1500 input -> encoder output T'=374, D=256; 6 decoder layers; V=600) with seeded weights,
beam 20, ctc_weight 0.1, nbest 1 and a fixed maxlenratio, so that every path takes the same number of output steps
(int(maxlenratio * 374); end_detect is off when maxlenratio is not 0).

    python tools/bench_decode.py [--maxlenratio 0.08] [--repeat 3] [--out FILE]
        three timed runs, each in a process of its own with its own time limit:
          plain    the existing search, Speech2Text(...)(speech)
          batch1   Speech2Text(..., batch_search=True)(speech): BatchBeamSearch, one utterance
          batch32  Speech2Text.decode_batch of 32 utterances
        prints one JSON record: utterances/s (encode + search) and search ms per output step of each.
    python tools/bench_decode.py --mode plain|batch1|batch32 ...      one of the runs (one JSON line)
    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/bench_decode.py --mode batch32 --repeat 1 --warmup 0
    python tools/bench_decode.py --analyze-trace DIR/.../NAME_kernel_trace.csv --utts 32
        from a kernel trace taken in a run of its own: time per launch and achieved bytes/s of esp_decode_attn in
        its self-attention and its source-attention use (the launches alternate self, source through the 6 layers
        of every step), and the share of all kernel time.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FRAMES, T_ENC, D_MODEL, LAYERS, HEADS, VOCAB, BEAM, CTC_WEIGHT = 1500, 374, 256, 6, 4, 600, 20, 0.1
LIMITS = {"plain": 600, "batch1": 300, "batch32": 300}  # seconds, per timed process


class _Timer:
    """Wall time of obj.name calls, synchronised on both sides."""

    def __init__(self, obj, name):
        import torch
        self.t, self.calls = 0.0, 0
        fn = getattr(obj, name)

        def wrapped(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.t += time.perf_counter() - t0
            self.calls += 1
            return out
        setattr(obj, name, wrapped)

    def reset(self):
        self.t, self.calls = 0.0, 0


def run(args):
    import numpy as np
    import torch
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from tests.helpers import build_model, c2_cfg

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = build_model(c2_cfg(), dev, dropout=0.0)
    model.eval()
    U = 32 if args.mode == "batch32" else 1
    rng = np.random.RandomState(1)
    speeches = [rng.randn(T_FRAMES, 80).astype(np.float32) for _ in range(U)]
    kw = dict(beam_size=BEAM, ctc_weight=CTC_WEIGHT, nbest=1, maxlenratio=args.maxlenratio)
    if args.mode != "plain":
        kw["batch_search"] = True
    s2t = Speech2Text(model, **kw)
    steps = max(1, int(args.maxlenratio * T_ENC))
    enc_t = _Timer(s2t.asr_model, "encode")
    search_t = _Timer(s2t.beam_search, "forward_batch" if args.mode == "batch32" else "forward")
    call = (lambda: s2t.decode_batch(speeches)) if args.mode == "batch32" else (lambda: [s2t(speeches[0])])
    for _ in range(args.warmup):
        res = call()
    enc_t.reset()
    search_t.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.repeat):
        res = call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.repeat
    taken = getattr(s2t.beam_search, "steps", None)  # the batch search counts its output steps
    print(json.dumps({
        "metric": "decode_throughput", "mode": args.mode, "utts": U, "beam": BEAM, "ctc_weight": CTC_WEIGHT,
        "maxlenratio": args.maxlenratio, "steps_max": steps, "steps_taken": taken, "repeat": args.repeat,
        "utt_per_s": round(U / wall, 3), "wall_ms": round(wall * 1e3, 2),
        "encode_ms": round(enc_t.t / args.repeat * 1e3, 2), "search_ms": round(search_t.t / args.repeat * 1e3, 2),
        "search_ms_per_step": round(search_t.t / args.repeat * 1e3 / (taken or steps), 3),
        "best_len": [len(r[0][3].yseq) for r in res][:4]}))


def analyze_trace(path, utts, maxlenratio):
    """esp_decode_attn launches in start order alternate self, source over the layers of a step; step s (from 0)
    has N = utts rows at s = 0 and utts * beam after (rows that ended are not known here: an upper bound), a self
    prefix of s + 1 keys and T'=374 source keys.  Bytes: K and V rows read (fp32), q read and out written; for the
    source use both the bytes requested by the rows and the unique bytes (rows of one utterance share them)."""
    rows, total = [], 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            if "decode_attn_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), dur))
    rows.sort()
    out = {"trace": os.path.basename(path), "utts": utts, "decode_attn_launches": len(rows),
           "all_kernels_ms": round(total * 1e3, 3), "decode_attn_share_of_kernel_time": round(sum(d for _, d in rows) / total, 4)}
    acc = {"self": [0.0, 0.0, 0.0, 0], "source": [0.0, 0.0, 0.0, 0]}  # seconds, requested bytes, unique bytes, launches
    for i, (_, dur) in enumerate(rows):
        step, kind = i // (2 * LAYERS), ("self", "source")[i % 2]
        N = utts if step == 0 else utts * BEAM
        keys = step + 1 if kind == "self" else T_ENC
        qo = 2 * N * D_MODEL * 4
        req = N * keys * D_MODEL * 2 * 4 + qo
        uniq = req if kind == "self" else utts * keys * D_MODEL * 2 * 4 + qo
        a = acc[kind]
        a[0] += dur
        a[1] += req
        a[2] += uniq
        a[3] += 1
    for kind, (t, req, uniq, n) in acc.items():
        if n:
            out[kind] = {"launches": n, "mean_us": round(t / n * 1e6, 2), "total_ms": round(t * 1e3, 3),
                         "requested_GBps": round(req / t / 1e9, 1), "unique_GBps": round(uniq / t / 1e9, 1)}
    print(json.dumps(out, indent=1))


def drive(args):
    record = {"tool": "tools/bench_decode.py", "maxlenratio": args.maxlenratio, "runs": {}}
    for mode in ("plain", "batch1", "batch32"):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--maxlenratio", str(args.maxlenratio),
               "--repeat", str(args.repeat), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[mode])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_decode.py: the {mode} run exceeded its {LIMITS[mode]} s limit; stopping")
        if p.returncode != 0:
            raise SystemExit(f"bench_decode.py: the {mode} run failed ({p.returncode}); stopping\n{p.stderr[-2000:]}")
        record["runs"][mode] = json.loads(p.stdout.strip().splitlines()[-1])
    r = record["runs"]
    record["speedup_batch1_vs_plain"] = round(r["batch1"]["utt_per_s"] / r["plain"]["utt_per_s"], 2)
    record["speedup_batch32_vs_plain"] = round(r["batch32"]["utt_per_s"] / r["plain"]["utt_per_s"], 2)
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "plain", "batch1", "batch32"], default="all")
    ap.add_argument("--maxlenratio", type=float, default=0.08)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    ap.add_argument("--utts", type=int, default=32)
    args = ap.parse_args()
    if args.analyze_trace is not None:
        return analyze_trace(args.analyze_trace, args.utts, args.maxlenratio)
    if args.maxlenratio <= 0 or args.repeat < 1 or args.warmup < 0:
        raise SystemExit("bench_decode.py: --maxlenratio > 0 (a fixed step count), --repeat >= 1, --warmup >= 0")
    if args.mode == "all":
        return drive(args)
    run(args)


if __name__ == "__main__":
    main()
