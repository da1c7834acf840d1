"""First measurements of Transformer LM training: a random-weight LM of the LibriSpeech train_lm_transformer2 shape
(16 layers, att_unit 512, 8 heads -> d_k 64, unit 2048, embed_unit 128, dropout 0.1) over the C2 vocabulary (600
tokens), on one fixed synthetic batch whose text lengths are drawn like the bench fixture's targets (20..40 tokens,
tests/golden/make_bench_fixture.py), so L = 41 at most and every layer's attention is B*8 problems of L x L x 64.

    python tools/bench_lm_train.py [--batch 128] [--steps 20] [--warmup 5] [--rounds 5] [--leg both] [--mode both]
        training steps (forward + backward + clip + Adam) timed with device events, ending in a synchronise.
        Legs: "eager" = the eager Trainer, kernel by kernel; "graph" = a torch.cuda.graph captured here by hand of
        ESPnetLanguageModel.forward_prepared + backward + the optimizer tail (the Trainer's graph path is ASR-only).
        Each leg runs with kernels.LM_ATTN_FUSED True (esp_causal_attn_fwd / _bwd) and False (MultiHeadedAttention's
        generic kernels), alternated round by round in one process on one box; prints tokens/s, ms/step and the
        spread between rounds of the same mode (one JSON document).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/bench_lm_train.py --leg eager --mode fused --rounds 1
    python tools/bench_lm_train.py --analyze-trace DIR/.../NAME_kernel_trace.csv [--batch B]
        per-launch time of the two fused attention kernels from a kernel trace taken in a run of its own, against
        their algorithmic HBM bytes (forward: qkv and klen read + ctx and lse written; backward: qkv, dctx, lse and
        klen read + dqkv written) and the measured 6.29 TB/s copy peak."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy on an MI355X (8.0e12 spec)
VOCAB = 600
LM_CONF = dict(pos_enc=None, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16, dropout_rate=0.1)
SEED = 20


def synthetic_batch(B):
    import numpy as np
    import torch
    rng = np.random.default_rng(SEED)
    lens = rng.integers(20, 41, size=B)
    text = np.zeros((B, int(lens.max())), dtype=np.int64)
    for i, n in enumerate(lens):
        text[i, :n] = rng.integers(1, VOCAB - 1, size=int(n))
    return torch.from_numpy(text), torch.from_numpy(lens.astype(np.int64))


def shape(B):
    _, lens = synthetic_batch(B)
    L = int(lens.max()) + 1
    D = LM_CONF["att_unit"]
    return dict(B=B, L=L, rows=B * L, ntokens=int(lens.sum()) + B, H=LM_CONF["head"], dk=D // LM_CONF["head"], D=D)


def algorithmic_bytes(B):
    s = shape(B)
    qkv, ctx, lse = s["rows"] * 3 * s["D"] * 4, s["rows"] * s["D"] * 4, s["B"] * s["H"] * s["L"] * 4
    return {"causal_attn_fwd_kernel": qkv + ctx + lse + 4 * B, "causal_attn_bwd_kernel": 2 * qkv + ctx + lse + 4 * B}


def analyze_trace(path, B):
    need = algorithmic_bytes(B)
    rows, total = {}, 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
            total += dur
            for k in need:
                if k in r["Kernel_Name"]:
                    rows.setdefault(k, []).append(dur)
    out = {"trace": os.path.basename(path), "batch": B, "shape": shape(B), "all_kernels_s": round(total, 6),
           "hbm_peak_measured_Bps": HBM_PEAK_MEASURED, "kernels": {}}
    for k, d in sorted(rows.items()):
        d.sort()
        med = d[len(d) // 2]
        out["kernels"][k] = {"launches": len(d), "median_us": round(med * 1e6, 2), "min_us": round(d[0] * 1e6, 2),
                             "max_us": round(d[-1] * 1e6, 2), "algorithmic_bytes": need[k],
                             "achieved_Bps_median": round(need[k] / med, 1),
                             "share_of_measured_hbm_peak": round(need[k] / med / HBM_PEAK_MEASURED, 4),
                             "share_of_all_kernel_time": round(sum(d) / total, 4)}
    print(json.dumps(out, indent=1))


def build(device):
    import torch
    from espnet_slurp_amd.lm import ESPnetLanguageModel, TransformerLM
    from espnet_slurp_amd.optimizers.fused_adam import FusedAdam
    torch.manual_seed(0)
    model = ESPnetLanguageModel(TransformerLM(VOCAB, **LM_CONF).to(device), VOCAB)
    model.flatten()
    model.train()
    return model, FusedAdam(model.parameters(), model.flat, lr=1e-4)


def eager_stepper(model, opt, text, lens):
    from espnet_slurp_amd.train.trainer import Trainer, TrainerOptions
    trainer = Trainer(model, opt, None, TrainerOptions(grad_clip=5.0), cuda_graph=False)
    batch = dict(text=text, text_lengths=lens)
    return lambda: trainer.train_one_step(batch)["loss"]


def graph_stepper(model, opt, text, lens, device):
    """forward_prepared + backward + clip + Adam + zero_grad as one captured graph, replayed per step; the dropout
    masks change per replay through the device RNG key (advanced inside the graph), as in the Trainer's graph path."""
    import torch
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.optimizers.fused_adam import clip_grad_norm_
    prep = model.prepare(text, lens).to_device(device)
    clip = torch.empty(3, dtype=torch.float32, device=device)
    key = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(device)

    def body():
        K.rng_advance(key)
        loss, _, _ = model.forward_prepared(prep)
        loss.backward()
        clip_grad_norm_(model.flat, 5.0, clip)
        opt.step_device(clip, None)
        model.flat.grad.zero_()
        return loss

    K.set_rng_key(key)
    try:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):  # warm-up: workspaces, LDS grants, the optimizer's device state
            body()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = body()
    finally:
        K.set_rng_key(None)

    def step():
        graph.replay()
        return loss
    return step


def one_round(leg, fused, args, device):
    import torch
    from espnet_slurp_amd import kernels as K
    K.LM_ATTN_FUSED = fused
    torch.cuda.reset_peak_memory_stats()
    model, opt = build(device)
    text, lens = synthetic_batch(args.batch)
    step = (eager_stepper(model, opt, text, lens) if leg == "eager"
            else graph_stepper(model, opt, text, lens, device))
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        loss = step()
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = ev0.elapsed_time(ev1) / args.steps
    res = {"ms_per_step": round(ms, 3), "wall_ms_per_step": round(wall * 1000.0 / args.steps, 3),
           "loss": float(loss.item()), "peak_hbm_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
           "params": int(sum(p.numel() for p in model.parameters()))}
    del step, opt, model
    torch.cuda.empty_cache()
    return res


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_train.py: no GPU (a measurement path does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    legs = {"both": ["eager", "graph"], "eager": ["eager"], "graph": ["graph"]}[args.leg]
    modes = {"both": [True, False], "fused": [True], "generic": [False]}[args.mode]
    s = shape(args.batch)
    out = {"metric": "lm_train_throughput", "model": "TransformerLM transformer2 shape (16 layers, att_unit 512, 8 heads, "
           "unit 2048, embed_unit 128, dropout 0.1), random weights", "vocab": VOCAB, "batch": args.batch,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "shape": s, "unit": "tokens/s"}
    for leg in legs:
        rounds = {True: [], False: []}
        for _ in range(args.rounds):  # alternated: fused, generic, fused, generic, ...
            for fused in modes:
                rounds[fused].append(one_round(leg, fused, args, device))
        out[leg] = {}
        for fused in modes:
            r = rounds[fused]
            ms = sorted(x["ms_per_step"] for x in r)
            med = ms[len(ms) // 2]
            out[leg]["fused" if fused else "generic"] = {
                "ms_per_step_median": med, "tokens_per_s_median": round(s["ntokens"] * 1000.0 / med, 1),
                "ms_per_step_rounds": [x["ms_per_step"] for x in r],
                "spread_between_rounds": round((ms[-1] - ms[0]) / med, 4),
                "peak_hbm_GiB": max(x["peak_hbm_GiB"] for x in r), "loss": r[-1]["loss"], "params": r[-1]["params"]}
        if len(modes) == 2:
            out[leg]["generic_over_fused_step_time"] = round(out[leg]["generic"]["ms_per_step_median"]
                                                             / out[leg]["fused"]["ms_per_step_median"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg", choices=["both", "eager", "graph"], default="both")
    ap.add_argument("--mode", choices=["both", "fused", "generic"], default="both")
    ap.add_argument("--analyze-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.analyze_trace is not None:
        return analyze_trace(args.analyze_trace, args.batch)
    if args.steps < 1 or args.warmup < 1 or args.rounds < 1:
        raise SystemExit("bench_lm_train.py: --steps, --warmup and --rounds must be >= 1")
    run(args)


if __name__ == "__main__":
    main()
