"""First measurements of the RNN-Transducer training step: the C2 SLURP Conformer (egs2/slurp/asr1, 12 blocks, d=256)
with `decoder: transducer` (1 LSTM layer of 512 units, dropout 0.1 / embedding dropout 0.2), joint space 640 (tanh),
ctc_weight 0.3; SpecAug and dropouts on; synthetic 80 x 1500 batches as bench.py makes them (20-40 labels).

    python tools/bench_transducer.py [--batch 64] [--steps 20] [--warmup 5] [--eager]
        training steps (forward + backward + clip + Adam) timed with device events, ending in a synchronise;
        the batch size is swept downward from --batch until it fits; prints utt/s, ms/step and the peak memory
        (one JSON line) beside the size of the materialised logits / joint activations and the loss workspace.
    python tools/bench_transducer.py --rounds 5 [--out FILE]
        the same run five times, each a fresh process; the lines, the median and the spread as one JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/bench_transducer.py --eager --steps 3 ...
    python tools/bench_transducer.py --analyze-trace DIR/.../NAME_kernel_trace.csv [--out FILE]
        the share of all kernel time of each new kernel family (csrc/rnnt.hip, csrc/lstm.hip) from a kernel trace
        taken in a run of its own."""
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

T_FRAMES = 1500
HIDDEN, JOINT = 512, 640
MODEL = "C2 SLURP Conformer + transducer (LSTM 1 x 512, joint 640 tanh, ctc_weight 0.3)"
FAMILIES = {  # kernel-name fragment -> family
    "joint_fwd_kernel": "joint_fwd", "joint_bwd_kernel": "joint_bwd", "joint_reduce_kernel": "joint_bwd",
    "rnnt_logprobs_kernel": "rnnt_logprobs", "rnnt_alpha_beta_kernel": "rnnt_alpha_beta",
    "rnnt_grad_kernel": "rnnt_grad", "lstm_cell_fwd_kernel": "lstm_cell", "lstm_cell_bwd_kernel": "lstm_cell"}


def out_frames(T):
    return ((T - 3) // 2 + 1 - 3) // 2 + 1


def bench_args():
    from tests.helpers import slurp_args, slurp_config
    conf = copy.deepcopy(slurp_config())
    args = slurp_args(conf)
    args.decoder = "transducer"
    args.decoder_conf = dict(rnn_type="lstm", num_layers=1, hidden_size=HIDDEN, dropout=0.1, dropout_embed=0.2)
    args.joint_net_conf = dict(joint_space_size=JOINT, joint_activation_type="tanh")
    args.model_conf = dict(ctc_weight=0.3, report_cer=False, report_wer=False)
    return args, conf["token_list_size"]


def analyze_trace(path, out_path=None):
    fam, total = {}, 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            for frag, name in FAMILIES.items():
                if frag in r["Kernel_Name"]:
                    fam.setdefault(name, []).append(dur)
                    break
    out = {"trace": os.path.basename(path), "model": MODEL, "all_kernels_s": round(total, 6), "families": {}}
    for name, d in sorted(fam.items()):
        d.sort()
        out["families"][name] = {"launches": len(d), "total_ms": round(sum(d) * 1e3, 3),
                                 "median_us": round(d[len(d) // 2] * 1e6, 2), "max_us": round(d[-1] * 1e6, 2),
                                 "share_of_all_kernel_time": round(sum(d) / total, 4)}
    out["new_kernels_share"] = round(sum(sum(d) for d in fam.values()) / total, 4) if total else 0.0
    text = json.dumps(out, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    print(text)


def run(args):
    import torch
    from espnet_slurp_amd import _native
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    from espnet_slurp_amd.schedulers.warmup_lr import WarmupLR
    from espnet_slurp_amd.tasks.asr import build_model
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    import bench

    if not torch.cuda.is_available():
        raise SystemExit("bench_transducer.py: no GPU (a measurement path does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    margs, V = bench_args()
    B = args.batch
    while True:
        try:
            torch.manual_seed(0)
            model = build_model(margs, device=device)
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
    Tq, U1 = out_frames(T_FRAMES), int(batch["text"].shape[1]) + 1
    cells = B * Tq * U1
    print(json.dumps({
        "metric": "train_throughput", "model": MODEL, "params": int(sum(p.numel() for p in model.parameters())),
        "batch": B, "batch_requested": args.batch, "frames": T_FRAMES, "enc_frames": Tq, "U1": U1, "vocab": V,
        "steps": args.steps, "warmup": args.warmup, "graph": not args.eager, "ms_per_step": round(ms, 3),
        "value": round(B * 1000.0 / ms, 2), "unit": "utt/s", "wall_ms_per_step": round(wall * 1000.0 / args.steps, 3),
        "loss": float(stats["loss"].item()), "peak_hbm_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
        "logits_GiB": round(cells * V * 4 / 2 ** 30, 3), "joint_act_GiB": round(cells * JOINT * 4 / 2 ** 30, 3),
        "loss_workspace_GiB": round(_native.workspace_bytes("esp_rnnt_loss", B, Tq, U1) / 2 ** 30, 4),
        "joint_bwd_workspace_GiB": round(_native.workspace_bytes("esp_rnnt_joint_bwd", B, Tq, U1, JOINT) / 2 ** 30, 4)}))


def rounds(args):
    """The same run `--rounds` times, a fresh process per run (one GPU process at a time)."""
    base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--steps", str(args.steps),
            "--warmup", str(args.warmup)] + (["--eager"] if args.eager else [])
    lines = []
    for r in range(args.rounds):
        p = subprocess.run(base, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"bench_transducer.py: round {r + 1} ended with {p.returncode}")
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        line["round"] = r + 1
        lines.append(line)
        print(f"round {r + 1}: {line['value']:.2f} utt/s  {line['ms_per_step']:.3f} ms/step  peak "
              f"{line['peak_hbm_GiB']} GiB  loss {line['loss']:.4f}", flush=True)
    v = sorted(x["value"] for x in lines)
    m = sorted(x["ms_per_step"] for x in lines)
    out = {"model": MODEL, "rounds": args.rounds, "utt_s_median": v[len(v) // 2], "utt_s_min": v[0], "utt_s_max": v[-1],
           "spread_rel": round((v[-1] - v[0]) / v[len(v) // 2], 5), "ms_per_step_median": m[len(m) // 2],
           "peak_hbm_GiB": lines[0]["peak_hbm_GiB"], "batch": lines[0]["batch"], "runs": lines}
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
    ap.add_argument("--rounds", type=int, default=0, metavar="N", help="N runs, each a fresh process")
    ap.add_argument("--out", default=None, help="--rounds / --analyze-trace: also write the JSON here")
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.analyze_trace is not None:
        return analyze_trace(args.analyze_trace, args.out)
    if args.steps < 1 or args.warmup < 1:
        raise SystemExit("bench_transducer.py: --steps and --warmup must be >= 1")
    if args.rounds:
        return rounds(args)
    run(args)


if __name__ == "__main__":
    main()
