"""Decode timing of the block-synchronous search: Speech2Text(streaming=True) against batch_search=True.

The streaming recipe's model shape (tests/golden/cbt_slurp_streaming.json: contextual block Transformer encoder,
d=512, 8 heads, 12 blocks, block 40 / hop 16 / look-ahead 16; 6 decoder blocks; V=600) with seeded random weights,
80 x 1500 input -> T'=374, beam 20, ctc_weight 0.5, nbest 1 and a fixed maxlenratio (end_detect off), both searches
on the same encoder output.  First measurements, not gates: nothing ran this search before.

    python tools/bench_stream_decode.py [--maxlenratio 0.08] [--repeat 5] [--warmup 1] [--out FILE]
        one JSON record:
          search    per search and repeat, search ms, output steps taken and ms per step, alternating the two
                    searches; their medians and the spread (max - min) / median between repeats; block moves and
                    steps taken back per utterance for the streaming search
          reorder   DecoderCache.reorder_keep (esp_cache_gather into the second buffer) against reorder (gather into
                    a temporary, copy back) at the search's rows and lengths: us per call from device events
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FRAMES, BEAM, CTC_WEIGHT = 1500, 20, 0.5


def recipe_conf():
    with open(os.path.join(ROOT, "tests", "golden", "cbt_slurp_streaming.json")) as f:
        conf = json.load(f)
    for k in ("reference_encoder_state_dict", "small_encoder_state_dict", "source"):
        conf.pop(k, None)
    return conf


def _spread(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def time_search(s2t, enc, maxlenratio, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hyps = s2t.beam_search.forward(enc, maxlenratio, 0.0)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    steps = s2t.beam_search.steps
    return dict(search_ms=round(ms, 2), steps=steps, ms_per_step=round(ms / steps, 3), best_len=len(hyps[0].yseq))


def time_reorder(model, rows, length, iters, torch):
    """us per call of reorder_keep and of reorder on caches of `rows` rows x `length` positions (index: a parent
    selection with repeats), from device events around `iters` back-to-back calls, alternating three times."""
    dec = model.decoder
    index = torch.randint(0, rows, (rows,), generator=torch.Generator().manual_seed(3)).to(dec.embed[0].weight.device)
    out = {"reorder_keep": [], "reorder": []}
    for _ in range(3):
        for name in ("reorder_keep", "reorder"):
            cache = dec.init_cache(rows, capacity=max(32, length))
            cache.buf.normal_()
            cache.len = length
            fn = getattr(cache, name)
            for _ in range(5):
                fn(index)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn(index)
            b.record()
            torch.cuda.synchronize()
            out[name].append(round(a.elapsed_time(b) * 1e3 / iters, 2))
    return {"rows": rows, "len": length, "layers": len(dec.decoders), "D": dec.D,
            "bytes_moved": len(dec.decoders) * rows * length * 2 * dec.D * 4,
            "reorder_keep_us": out["reorder_keep"], "reorder_us": out["reorder"],
            "reorder_keep_us_median": statistics.median(out["reorder_keep"]),
            "reorder_us_median": statistics.median(out["reorder"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maxlenratio", type=float, default=0.08)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.maxlenratio <= 0 or args.repeat < 1 or args.warmup < 0:
        raise SystemExit("bench_stream_decode.py: --maxlenratio > 0 (a fixed step bound), --repeat >= 1, --warmup >= 0")
    import numpy as np
    import torch
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    from espnet_slurp_amd.tasks.asr import build_model
    from tests.branchformer_helpers import args_from_conf

    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_decode.py: no GPU (a measurement path does not fall back)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    conf = recipe_conf()
    model = build_model(args_from_conf(conf, dropout=0.0), device=dev)
    model.eval()
    speech = np.random.RandomState(1).randn(T_FRAMES, 80).astype(np.float32)
    kw = dict(beam_size=BEAM, ctc_weight=CTC_WEIGHT, nbest=1, maxlenratio=args.maxlenratio)
    searches = {"streaming": Speech2Text(model, streaming=True, **kw), "batch": Speech2Text(model, batch_search=True, **kw)}
    enc = searches["batch"].encode(speech)
    runs = {k: [] for k in searches}
    for it in range(args.warmup + args.repeat):
        for name, s2t in searches.items():  # alternating
            r = time_search(s2t, enc, args.maxlenratio, torch)
            if it >= args.warmup:
                runs[name].append(r)
    st = searches["streaming"].beam_search
    record = {"tool": "tools/bench_stream_decode.py", "device": torch.cuda.get_device_name(0), "enc_frames": int(enc.shape[0]),
              "beam": BEAM, "ctc_weight": CTC_WEIGHT, "maxlenratio": args.maxlenratio, "repeat": args.repeat,
              "search": {}, "block_moves_per_utt": len(st.block_trace) - 1, "steps_taken_back_per_utt": st.rollbacks,
              "block_trace": [list(t) for t in st.block_trace]}
    for name, rs in runs.items():
        per = [r["ms_per_step"] for r in rs]
        record["search"][name] = {"runs": rs, "ms_per_step_median": statistics.median(per),
                                  "ms_per_step_spread": _spread(per)}
    record["streaming_over_batch_ms_per_step"] = round(
        record["search"]["streaming"]["ms_per_step_median"] / record["search"]["batch"]["ms_per_step_median"], 3)
    record["reorder"] = [time_reorder(model, BEAM, L, 200, torch) for L in (8, 29, 128)]
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
