"""First measurements of the contextual block Transformer encoder: the egs2/slurp streaming recipe model (committed
settings, tests/golden/cbt_slurp_streaming.json: d=512, 8 heads, 12 blocks, block 40 / hop 16 / look-ahead 16; decoder
6 blocks; SpecAug and the recipe's dropouts on) on synthetic 80 x 1500 batches as bench.py makes them.  T' = 374 is
22 blocks of 42 slots per utterance: 59,136 rows and 11,264 attention problems of 42 x 42 x 64 per layer at B = 64.

    python tools/bench_cbt.py [--batch 64] [--steps 10] [--warmup 4] [--rounds 3] [--eager] [--mode both]
        training steps (forward + backward + clip + Adam) timed with device events, ending in a synchronise, with
        kernels.CBT_ATTN_FUSED True (esp_block_attn_fwd / _bwd) and False (MultiHeadedAttention's generic kernels),
        alternated round by round in one process on one box; prints utt/s, ms/step and peak memory per mode and the
        spread between rounds of the same mode (one JSON document).
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_cbt.py --eager --mode fused --rounds 1 ...
    python tools/bench_cbt.py --analyze-trace DIR/.../NAME_kernel_trace.csv --batch B
        per-launch time of the two fused attention kernels from a kernel trace taken in a run of its own, against
        their algorithmic HBM bytes (forward: qkv read + ctx and lse written; backward: qkv, dctx and lse read + dqkv
        written) and the measured 6.29 TB/s copy peak."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy on an MI355X (8.0e12 spec)
T_FRAMES = 1500


def out_frames(T):
    return ((T - 3) // 2 + 1 - 3) // 2 + 1


def recipe_conf():
    with open(os.path.join(ROOT, "tests", "golden", "cbt_slurp_streaming.json")) as f:
        conf = json.load(f)
    for k in ("reference_encoder_state_dict", "small_encoder_state_dict", "source"):
        conf.pop(k, None)
    return conf


def block_shape(B, conf):
    e = conf["encoder_conf"]
    T2 = out_frames(T_FRAMES)
    bs, hop = e["block_size"], e["hop_size"]
    nblk = -(-(T2 - bs + hop) // hop)
    return dict(T2=T2, nblk=nblk, S=bs + 2, Z=B * nblk, H=e["attention_heads"], D=e["output_size"],
                rows=B * nblk * (bs + 2))


def algorithmic_bytes(B, conf):
    s = block_shape(B, conf)
    qkv, ctx, lse = s["rows"] * 3 * s["D"] * 4, s["rows"] * s["D"] * 4, s["Z"] * s["H"] * s["S"] * 4
    return {"block_attn_fwd_kernel": qkv + ctx + lse, "block_attn_bwd_kernel": 2 * qkv + ctx + lse}


def analyze_trace(path, B):
    conf = recipe_conf()
    need = algorithmic_bytes(B, conf)
    rows, total = {}, 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            for k in need:
                if k in r["Kernel_Name"]:
                    rows.setdefault(k, []).append(dur)
    out = {"trace": os.path.basename(path), "batch": B, "shape": block_shape(B, conf),
           "all_kernels_s": round(total, 6), "hbm_peak_measured_Bps": HBM_PEAK_MEASURED, "kernels": {}}
    for k, d in sorted(rows.items()):
        d.sort()
        med = d[len(d) // 2]
        out["kernels"][k] = {"launches": len(d), "median_us": round(med * 1e6, 2), "min_us": round(d[0] * 1e6, 2),
                             "max_us": round(d[-1] * 1e6, 2), "algorithmic_bytes": need[k],
                             "achieved_Bps_median": round(need[k] / med, 1),
                             "share_of_measured_hbm_peak": round(need[k] / med / HBM_PEAK_MEASURED, 4),
                             "share_of_all_kernel_time": round(sum(d) / total, 4)}
    print(json.dumps(out, indent=1))


def one_round(fused, B, args, conf, device):
    import torch
    from tests.branchformer_helpers import args_from_conf
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.tasks.asr import build_model
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    import bench

    K.CBT_ATTN_FUSED = fused
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    model = build_model(args_from_conf(conf), device=device)
    model.train()
    opt = FusedAdam(model.parameters(), model.flat, lr=2e-4)
    trainer = Trainer(model, opt, WarmupLR(opt, warmup_steps=25000), TrainerOptions(grad_clip=5.0),
                      cuda_graph=not args.eager)
    batch = bench.synthetic_batch(B, conf["token_list_size"], 0, device)
    for _ in range(args.warmup):
        trainer.train_one_step(batch)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        stats = trainer.train_one_step(batch)
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = ev0.elapsed_time(ev1) / args.steps
    res = {"ms_per_step": round(ms, 3), "utt_per_s": round(B * 1000.0 / ms, 2),
           "wall_ms_per_step": round(wall * 1000.0 / args.steps, 3), "loss": float(stats["loss"].item()),
           "peak_hbm_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
           "params": int(sum(p.numel() for p in model.parameters()))}
    del trainer, opt, model, batch
    torch.cuda.empty_cache()
    return res


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cbt.py: no GPU (a measurement path does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    conf = recipe_conf()
    modes = {"both": [True, False], "fused": [True], "generic": [False]}[args.mode]
    rounds = {True: [], False: []}
    for _ in range(args.rounds):  # alternated: fused, generic, fused, generic, ...
        for fused in modes:
            rounds[fused].append(one_round(fused, args.batch, args, conf, device))
    out = {"metric": "train_throughput", "model": "contextual block Transformer egs2/slurp streaming (d=512, 12 blocks, "
           "block 40 / hop 16 / look-ahead 16)", "batch": args.batch, "frames": T_FRAMES, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "graph": not args.eager,
           "shape": block_shape(args.batch, conf), "unit": "utt/s"}
    for fused in modes:
        r = rounds[fused]
        ms = sorted(x["ms_per_step"] for x in r)
        med = ms[len(ms) // 2]
        out["fused" if fused else "generic"] = {
            "ms_per_step_median": med, "utt_per_s_median": round(args.batch * 1000.0 / med, 2),
            "ms_per_step_rounds": [x["ms_per_step"] for x in r],
            "spread_between_rounds": round((ms[-1] - ms[0]) / med, 4),
            "peak_hbm_GiB": max(x["peak_hbm_GiB"] for x in r), "loss": r[-1]["loss"], "params": r[-1]["params"]}
    if len(modes) == 2:
        out["generic_over_fused_step_time"] = round(out["generic"]["ms_per_step_median"]
                                                    / out["fused"]["ms_per_step_median"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mode", choices=["both", "fused", "generic"], default="both")
    ap.add_argument("--eager", action="store_true", help="launch kernel by kernel instead of replaying a HIP graph")
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.analyze_trace:
        return analyze_trace(args.analyze_trace, args.batch)
    if args.steps < 1 or args.warmup < 1 or args.rounds < 1:
        raise SystemExit("bench_cbt.py: --steps, --warmup and --rounds must be >= 1")
    run(args)


if __name__ == "__main__":
    main()
