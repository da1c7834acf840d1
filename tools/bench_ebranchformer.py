"""First measurements of the E-Branchformer encoder: d=512, 8 heads, 12 blocks, cgMLP 3072 units with kernel 31,
macaron + plain feed-forward modules of 1024 units, merge kernel 31 (the shape of ESPnet's LibriSpeech
E-Branchformer recipe); decoder, SpecAug and loss weights of the committed egs2/slurp_entity settings
(tests/golden/branchformer_slurp_entity.json); dropouts 0.1; synthetic 80 x 1500 batches as bench.py makes them.

    python tools/bench_ebranchformer.py [--batch 64] [--steps 20] [--warmup 5] [--eager] [--composed]
        training steps (forward + backward + clip + Adam) timed with device events, ending in a synchronise;
        the batch size is swept downward from --batch until it fits; prints utt/s and ms/step (one JSON line).
        --composed: kernels.EBF_MERGE_FUSED = False (the merge on esp_dwconv1d / _wgrad / esp_colsum).
    python tools/bench_ebranchformer.py --ab 5 [--out FILE]
        fused and composed alternated, each run a fresh process; the lines, medians and spreads as one JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/bench_ebranchformer.py --eager --steps 3 ...
    python tools/bench_ebranchformer.py --analyze-trace DIR/.../NAME_kernel_trace.csv --batch B
        per-launch time of the merge kernels (csrc/ebf_merge.hip) from a kernel trace taken in a run of its own,
        and their achieved bytes/s against the algorithmic bytes computed here from the shapes."""
import argparse
import copy
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy on an MI355X (8.0e12 spec)
T_FRAMES = 1500
D, MERGE_K = 512, 31
MODEL = "E-Branchformer (d=512, 8 heads, 12 blocks, cgMLP 3072 k=31, macaron + FFN 1024, merge k=31)"


def out_frames(T):
    return ((T - 3) // 2 + 1 - 3) // 2 + 1


def bench_conf():
    with open(os.path.join(ROOT, "tests", "golden", "branchformer_slurp_entity.json")) as f:
        conf = copy.deepcopy(json.load(f))
    conf["encoder"] = "e_branchformer"
    conf["encoder_conf"] = dict(
        output_size=D, attention_heads=8, attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos",
        rel_pos_type="latest", cgmlp_linear_units=3072, cgmlp_conv_kernel=31, use_linear_after_conv=False,
        gate_activation="identity", num_blocks=12, dropout_rate=0.1, positional_dropout_rate=0.1,
        attention_dropout_rate=0.1, input_layer="conv2d", layer_drop_rate=0.0, linear_units=1024,
        positionwise_layer_type="linear", use_ffn=True, macaron_ffn=True, merge_conv_kernel=MERGE_K)
    return conf


def algorithmic_bytes(B, u_planes=0):
    """Bytes each merge kernel must move at least once per launch: M = B T' rows of C = 2D channels.  The
    backward's partial sums (its workspace) are the reduce kernel's input and are counted there, not as the
    tile kernel's algorithmic traffic."""
    Tq = out_frames(T_FRAMES)
    M, C = B * Tq, 2 * D
    full = M * C * 4
    u = M * C * 2 * u_planes if u_planes else full
    par = 4 * C * (MERGE_K + 1)
    parts = B * (((Tq + 63) // 64 + 3) // 4)  # a backward block walks four 64-frame tiles
    return {
        "ebf_merge_fwd_kernel": full + u + par,       # read xc; write u
        "ebf_merge_bwd_kernel": 2 * full + full,      # read du, xc; write d1 | d2
        "ebf_merge_reduce_kernel": parts * par + 2 * par,  # read the partial sums; dW, dbias +=
    }


def classify(name):
    for k in ("ebf_merge_fwd_kernel", "ebf_merge_bwd_kernel", "ebf_merge_reduce_kernel"):
        if k in name:
            return k
    return None


def analyze_trace(path, B):
    need = algorithmic_bytes(B)
    rows = {}
    total = 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            k = classify(r["Kernel_Name"])
            if k:
                rows.setdefault(k, []).append(dur)
    out = {"trace": os.path.basename(path), "batch": B, "rows_M": B * out_frames(T_FRAMES), "channels_C": 2 * D,
           "merge_k": MERGE_K, "all_kernels_s": round(total, 6), "hbm_peak_measured_Bps": HBM_PEAK_MEASURED,
           "kernels": {}}
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
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.tasks.asr import build_model
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    import bench

    if not torch.cuda.is_available():
        raise SystemExit("bench_ebranchformer.py: no GPU (a measurement path does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    K.EBF_MERGE_FUSED = not args.composed
    conf = bench_conf()
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
        "metric": "train_throughput", "model": MODEL, "merge": "composed" if args.composed else "fused",
        "params": int(sum(p.numel() for p in model.parameters())), "batch": B, "batch_requested": args.batch,
        "frames": T_FRAMES, "steps": args.steps, "warmup": args.warmup, "graph": not args.eager,
        "ms_per_step": round(ms, 3), "value": round(B * 1000.0 / ms, 2), "unit": "utt/s",
        "wall_ms_per_step": round(wall * 1000.0 / args.steps, 3), "loss": float(stats["loss"].item()),
        "peak_hbm_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


def ab(args):
    """Fused and composed alternated, a fresh process per run (one GPU process at a time)."""
    lines = {"fused": [], "composed": []}
    base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--steps", str(args.steps),
            "--warmup", str(args.warmup)] + (["--eager"] if args.eager else [])
    for r in range(args.ab):
        for mode in ("fused", "composed"):
            p = subprocess.run(base + (["--composed"] if mode == "composed" else []), capture_output=True, text=True,
                               timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_ebranchformer.py: the {mode} run of round {r + 1} ended with {p.returncode}")
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            line["round"] = r + 1
            lines[mode].append(line)
            print(f"{mode:8s} round {r + 1}: {line['value']:.2f} utt/s  {line['ms_per_step']:.3f} ms/step  "
                  f"peak {line['peak_hbm_GiB']} GiB  loss {line['loss']:.4f}", flush=True)
    out = {"model": MODEL, "rounds": args.ab, "alternated": "fused, composed, fused, ... on one box", "modes": {}}
    for mode, ls in lines.items():
        v = sorted(x["value"] for x in ls)
        m = sorted(x["ms_per_step"] for x in ls)
        out["modes"][mode] = {"utt_s_median": v[len(v) // 2], "utt_s_min": v[0], "utt_s_max": v[-1],
                              "spread_rel": round((v[-1] - v[0]) / v[len(v) // 2], 5),
                              "ms_per_step_median": m[len(m) // 2], "peak_hbm_GiB": ls[0]["peak_hbm_GiB"],
                              "batch": ls[0]["batch"], "runs": ls}
    f, c = out["modes"]["fused"], out["modes"]["composed"]
    out["fused_over_composed"] = round(f["utt_s_median"] / c["utt_s_median"], 5)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="launch kernel by kernel instead of replaying a HIP graph")
    ap.add_argument("--composed", action="store_true", help="the merge on the existing depthwise kernels")
    ap.add_argument("--ab", type=int, default=0, metavar="ROUNDS", help="fused / composed alternated, ROUNDS each")
    ap.add_argument("--out", default=None, help="--ab: also write the JSON here")
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.analyze_trace is not None:
        return analyze_trace(args.analyze_trace, args.batch)
    if args.steps < 1 or args.warmup < 1:
        raise SystemExit("bench_ebranchformer.py: --steps and --warmup must be >= 1")
    if args.ab:
        return ab(args)
    run(args)


if __name__ == "__main__":
    main()
