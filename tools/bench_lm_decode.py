"""Decode timing with Transformer LM shallow fusion: the batch search of tools/bench_decode.py (C2 model shape, seeded
weights, ctc_weight 0.1, a fixed maxlenratio so that every run takes the same number of output steps) without an LM,
and with a random-weight LM of the LibriSpeech `transformer2` shape (16 layers, att_unit 512, 8 heads, unit 2048,
embed_unit 128) over the model's vocabulary at lm_weight 0.6, its step on the generic kernels
(kernels.LM_STEP_FUSED = False) and on esp_step_linear (True).

    python tools/bench_lm_decode.py [--repeat 3] [--out FILE]
        one process per shape, each with its own time limit: u1b20 (one utterance, beam 20), u1b60 (beam 60),
        u32b20 (decode_batch of 32 utterances, beam 20); inside a process the three variants alternate, --repeat
        rounds.  Prints one JSON record: utterances/s and search ms per output step, every round.
    python tools/bench_lm_decode.py --mode rows [--rows 1,8,20,...]
        the LM step alone (TransformerLM.batch_score at prefix lengths 9..24) per row count, fused against generic,
        alternating, --repeat rounds: the measurement behind kernels.LM_STEP_MAX_ROWS.  Also counts the native
        launches of one step of each path.
    python tools/bench_lm_decode.py --mode u1b20 --variants fused --repeat 1 --warmup 0
        one variant only (for a kernel trace of its own: rocprofv3 --kernel-trace --stats ... -- python tools/...).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FRAMES, T_ENC, VOCAB, CTC_WEIGHT, LM_WEIGHT = 1500, 374, 600, 0.1, 0.6
TRANSFORMER2 = dict(pos_enc=None, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16, dropout_rate=0.1)
SHAPES = {"u1b20": (1, 20), "u1b60": (1, 60), "u32b20": (32, 20)}
LIMITS = {"u1b20": 300, "u1b60": 300, "u32b20": 400, "rows": 400}  # seconds, per timed process
VARIANTS = ("none", "generic", "fused")


def _lm(dev):
    import torch
    from espnet_slurp_amd.lm import TransformerLM
    torch.manual_seed(1)
    lm = TransformerLM(VOCAB, **TRANSFORMER2).to(dev).eval()
    lm.flatten()
    return lm


def run_shape(args):
    import numpy as np
    import torch
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from tests.helpers import build_model, c2_cfg

    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_decode.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    U, beam = SHAPES[args.mode]
    torch.manual_seed(0)
    model = build_model(c2_cfg(), dev, dropout=0.0)
    model.eval()
    lm = _lm(dev)
    rng = np.random.RandomState(1)
    speeches = [rng.randn(T_FRAMES, 80).astype(np.float32) for _ in range(U)]
    kw = dict(beam_size=beam, ctc_weight=CTC_WEIGHT, nbest=1, maxlenratio=args.maxlenratio, batch_search=True)
    s2t = {"none": Speech2Text(model, **kw), "lm": Speech2Text(model, lm=lm, lm_weight=LM_WEIGHT, **kw)}
    rounds = {v: [] for v in args.variants}

    def once(variant):
        K.LM_STEP_FUSED = variant == "fused"
        s = s2t["none" if variant == "none" else "lm"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc_lens = None
        if U == 1:
            enc = s.encode(speeches[0])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            s.beam_search.forward(enc, args.maxlenratio, 0.0)
        else:
            sp = torch.tensor(np.stack(speeches))
            lengths = torch.full((U,), T_FRAMES, dtype=torch.int64)
            enc, enc_lens = s.asr_model.encode(sp.to(dev), lengths, sl_cpu=lengths)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            s.batch_beam_search.forward_batch(enc, [int(t) for t in enc_lens], args.maxlenratio, 0.0)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = s.batch_beam_search.steps
        return {"utt_per_s": round(U / (t2 - t0), 3), "search_ms_per_step": round((t2 - t1) * 1e3 / steps, 3),
                "steps": steps}

    with torch.no_grad():
        for _ in range(args.warmup):
            for v in args.variants:
                once(v)
        for _ in range(args.repeat):
            for v in args.variants:
                rounds[v].append(once(v))
    K.LM_STEP_FUSED = True
    print(json.dumps({"metric": "lm_decode", "shape": args.mode, "utts": U, "beam": beam, "rows": U * beam,
                      "lm_step_max_rows": K.LM_STEP_MAX_ROWS, "maxlenratio": args.maxlenratio, "rounds": rounds}))


def run_rows(args):
    import torch
    from espnet_slurp_amd import _native
    from espnet_slurp_amd import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_decode.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    lm = _lm(dev)
    cap = K.LM_STEP_MAX_ROWS
    K.LM_STEP_MAX_ROWS = 1 << 30  # this run measures the fused step beyond any cap
    out = {"metric": "lm_step_rows", "prefix_lengths": [9, 24], "rows": {}}
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for N in args.rows:
            ys = torch.randint(1, VOCAB - 1, (N, 24), generator=g)
            rec = {"fused_ms": [], "generic_ms": []}
            for rnd in range(args.repeat + 1):  # round 0 warms up
                for name, fused in (("generic_ms", False), ("fused_ms", True)):
                    K.LM_STEP_FUSED = fused
                    _, cache = lm.batch_score(ys[:, :8], None, None)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for L in range(9, 25):
                        _, cache = lm.batch_score(ys[:, :L], cache, None)
                    torch.cuda.synchronize()
                    if rnd:
                        rec[name].append(round((time.perf_counter() - t0) * 1e3 / 16, 4))
            out["rows"][N] = rec
        calls = []
        orig = _native.call
        _native.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        for name, fused in (("generic", False), ("fused", True)):
            K.LM_STEP_FUSED = fused
            ys = torch.randint(1, VOCAB - 1, (20, 9), generator=g)
            _, cache = lm.batch_score(ys[:, :8], None, None)
            del calls[:]
            lm.batch_score(ys, cache, None)
            out[f"launches_per_step_{name}"] = len(calls)
        _native.call = orig
    K.LM_STEP_FUSED, K.LM_STEP_MAX_ROWS = True, cap
    print(json.dumps(out))


def drive(args):
    record = {"tool": "tools/bench_lm_decode.py", "maxlenratio": args.maxlenratio, "runs": {}}
    for mode in list(SHAPES) + ["rows"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--maxlenratio", str(args.maxlenratio),
               "--repeat", str(args.repeat), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[mode])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_lm_decode.py: the {mode} run exceeded its {LIMITS[mode]} s limit; stopping")
        if p.returncode != 0:
            raise SystemExit(f"bench_lm_decode.py: the {mode} run failed ({p.returncode}); stopping\n{p.stderr[-2000:]}")
        record["runs"][mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(record["runs"][mode]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "rows"] + list(SHAPES), default="all")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--rows", default="1,8,20,40,60,64,96,128,256,640")
    ap.add_argument("--maxlenratio", type=float, default=0.08)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.variants = [v for v in args.variants.split(",") if v]
    args.rows = [int(r) for r in args.rows.split(",") if r]
    if args.maxlenratio <= 0 or args.repeat < 1 or args.warmup < 0 or any(v not in VARIANTS for v in args.variants):
        raise SystemExit("bench_lm_decode.py: --maxlenratio > 0, --repeat >= 1, --warmup >= 0, variants of " + str(VARIANTS))
    if args.mode == "all":
        return drive(args)
    if args.mode == "rows":
        return run_rows(args)
    run_shape(args)


if __name__ == "__main__":
    main()
