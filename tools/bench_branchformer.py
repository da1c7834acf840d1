"""First measurements of the Branchformer encoder: the egs2/slurp_entity recipe model (committed settings,
tests/golden/branchformer_slurp_entity.json: d=512, 8 heads, 18 blocks, cgMLP 2048 units, kernel 31; decoder 6
blocks; SpecAug and the recipe's dropouts on) on synthetic 80 x 1500 batches as bench.py makes them.

    python tools/bench_branchformer.py [--batch 64] [--steps 20] [--warmup 5] [--eager]
        training steps (forward + backward + clip + Adam) timed with device events, ending in a synchronise;
        the batch size is swept downward from --batch until it fits; prints utt/s and ms/step (one JSON line).
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_branchformer.py --eager --steps 3 ...
    python tools/bench_branchformer.py --analyze-trace DIR/.../NAME_kernel_trace.csv --batch B
        per-launch time of the cgMLP kernels (csrc/cgmlp.hip) from a kernel trace taken in a run of its own, and
        their achieved bytes/s against the algorithmic bytes computed here from the shapes.

Neighbouring figure, not a target: the Conformer C4 shape (d=512, 17 blocks, B=64) runs at 360 utt/s."""
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
    with open(os.path.join(ROOT, "tests", "golden", "branchformer_slurp_entity.json")) as f:
        return json.load(f)


def algorithmic_bytes(B, conf, dv_planes=0):
    """Bytes each cgMLP kernel must move at least once per launch, from the shapes: M = B T' rows, U = 2C units."""
    M = B * out_frames(T_FRAMES)
    U = conf["encoder_conf"]["cgmlp_linear_units"]
    C = U // 2
    half = M * C * 4
    dvh = M * C * 2 * dv_planes if dv_planes else half  # one half of dv: fp32, or 1 / 3 bf16 planes
    stats = 2 * M * 4
    return {
        "csgu_stats_kernel": half + stats,                   # read v_g; write mean, rstd
        "csgu_tile_kernel<fwd>": 2 * half + half + stats,    # read v; write o
        "csgu_tile_kernel<bwd>": 2 * half + half + stats + dvh + 2 * half,  # read v, dout; write dv_r, dg, n
        "csgu_bwd_norm_kernel": 2 * half + stats + dvh + half,  # read v_g, dn; write dv_g, dn * xhat
    }


def classify(name):
    if "csgu_stats_kernel" in name:
        return "csgu_stats_kernel"
    if "csgu_bwd_norm_kernel" in name:
        return "csgu_bwd_norm_kernel"
    if "csgu_tile_kernel" in name:
        # the template's second argument: false = forward, true = backward (demangled), Lb0 / Lb1 (mangled)
        bwd = "true>" in name.replace(" ", "") or "Lb1E" in name
        return "csgu_tile_kernel<bwd>" if bwd else "csgu_tile_kernel<fwd>"
    return None


def analyze_trace(path, B):
    conf = recipe_conf()
    need = algorithmic_bytes(B, conf)
    rows = {}
    total = 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            k = classify(r["Kernel_Name"])
            if k:
                rows.setdefault(k, []).append(dur)
    out = {"trace": os.path.basename(path), "batch": B, "rows_M": B * out_frames(T_FRAMES),
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


def run(args):
    import torch
    from tests.branchformer_helpers import args_from_conf
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.tasks.asr import build_model
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    import bench

    if not torch.cuda.is_available():
        raise SystemExit("bench_branchformer.py: no GPU (a measurement path does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    conf = recipe_conf()
    V = conf["token_list_size"]
    B = args.batch
    while True:
        try:
            torch.manual_seed(0)
            model = build_model(args_from_conf(conf), device=device)
            model.train()
            opt = FusedAdam(model.parameters(), model.flat, lr=2e-4)
            trainer = Trainer(model, opt, WarmupLR(opt, warmup_steps=25000), TrainerOptions(grad_clip=5.0),
                              cuda_graph=not args.eager)
            batch = bench.synthetic_batch(B, V, 0, device)
            for _ in range(args.warmup):
                trainer.train_one_step(batch)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            del model, opt, trainer
            torch.cuda.empty_cache()
            if B <= 1:
                raise
            B //= 2
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        stats = trainer.train_one_step(batch)
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = ev0.elapsed_time(ev1) / args.steps
    print(json.dumps({
        "metric": "train_throughput", "model": "Branchformer egs2/slurp_entity (d=512, 18 blocks, cgMLP 2048, k=31)",
        "params": int(sum(p.numel() for p in model.parameters())), "batch": B, "batch_requested": args.batch,
        "frames": T_FRAMES, "steps": args.steps, "warmup": args.warmup, "graph": not args.eager,
        "ms_per_step": round(ms, 3), "value": round(B * 1000.0 / ms, 2), "unit": "utt/s",
        "wall_ms_per_step": round(wall * 1000.0 / args.steps, 3), "loss": float(stats["loss"].item()),
        "peak_hbm_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
        "neighbour": "Conformer C4 shape (d=512, 17 blocks, B=64): 360 utt/s (not a target)"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="launch kernel by kernel instead of replaying a HIP graph")
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.analyze_trace:
        return analyze_trace(args.analyze_trace, args.batch)
    if args.steps < 1 or args.warmup < 1:
        raise SystemExit("bench_branchformer.py: --steps and --warmup must be >= 1")
    run(args)


if __name__ == "__main__":
    main()
