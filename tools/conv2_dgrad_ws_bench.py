"""A/B of the conv2 input gradient's class GEMMs: gemm_dgrad_ws_kernel (csrc/gemm_dgrad_ws.hip) against the LDS-DMA
kernel, at C2 shapes (T = 1500, F = 80, D = 256), alone:
    python tools/conv2_dgrad_ws_bench.py [B] [--rounds R] [--reps N] [--bits]
    python tools/conv2_dgrad_ws_bench.py --analyze-trace DIR
The first form alternates esp_set_dgrad_ws modes 0 (the LDS-DMA kernel) and 2 (the new kernel for every class) over R
rounds of N calls in one process and prints the time per call (the four class GEMMs summed, with the fold's two small
reductions) per mode and round; --bits: esp_conv2_dgrad_bits (dz1 stored) instead of esp_conv2_dgrad_c1fold.  Per
class: run it under rocprofv3 --kernel-trace and give the output directory to the second form, which takes the class
GEMM dispatches in order (every call launches classes K = 4D, 2D, 2D, D in this order, on either kernel) and prints
each class's mean and least time per kernel."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def analyze(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].replace(" ", "")
                new = "gemm_dgrad_ws_kernel" in name
                if new or "gemm_glds_kernel<(espg::Mode)4" in name or "gemm_glds_kernel<4," in name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), new))
    rows.sort()
    if not rows or len(rows) % 4:
        raise SystemExit(f"conv2_dgrad_ws_bench: {len(rows)} class GEMM dispatches in {d}: not whole calls")
    t = {}
    for i, (s, e, new) in enumerate(rows):
        t.setdefault((new, i % 4), []).append((e - s) * 1e-3)
    ks = ("4D", "2D", "2D", "D")
    for new in (False, True):
        tot = 0.0
        for cls in range(4):
            v = t.get((new, cls), [])
            if not v:
                continue
            v = v[len(v) // 4:]  # (the first quarter: warm-up)
            tot += sum(v) / len(v)
            print(f"{'gemm_dgrad_ws_kernel' if new else 'gemm_glds_kernel    '} class {cls} K={ks[cls]:>2}: n {len(v):3d}  "
                  f"mean {sum(v) / len(v):8.1f} us  min {min(v):8.1f} us")
        print(f"{'gemm_dgrad_ws_kernel' if new else 'gemm_glds_kernel    '} four classes: {tot / 1e3:.3f} ms")


def main():
    argv = sys.argv[1:]
    if "--analyze-trace" in argv:
        return analyze(argv[argv.index("--analyze-trace") + 1])

    def opt(name, default):
        if name in argv:
            i = argv.index(name)
            v = int(argv[i + 1])
            del argv[i:i + 2]
            return v
        return default

    rounds, reps = opt("--rounds", 3), opt("--reps", 5)
    bits_only = "--bits" in argv
    a = [v for v in argv if not v.startswith("--")]
    B = int(a[0]) if a else 384
    import torch

    from espnet_slurp_amd import kernels as K

    dev = torch.device("cuda:0")
    D, T, F = 256, 1500, 80
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, F, device=dev, generator=g)
    bits = torch.randint(-2**31, 2**31, (B * T1 * F1 * D // 32,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    dz2 = torch.randn(B * T2 * F2, D, device=dev, generator=g)
    W = torch.randn(D, D, 3, 3, device=dev, generator=g) / 48.0
    dW, db = torch.zeros(D, 9, device=dev), torch.zeros(D, device=dev)
    dz1 = torch.empty(B * T1 * F1 * D, device=dev) if bits_only else None

    def call():
        if bits_only:
            K.conv2_dgrad(dz2, W, None, dz1, B, T1, F1, D, z1bits=bits)
        else:
            K.conv2_dgrad_c1fold(dz2, W, bits, x, T, F, dW, db, B, T1, F1, D)

    for r in range(rounds):
        for mode in (0, 2):
            K.set_dgrad_ws(mode)
            n0 = K.dgrad_ws_launches()
            call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            print(f"round {r} dgrad_ws={mode} B={B} {'bits' if bits_only else 'c1fold'}: {e0.elapsed_time(e1) / reps:.3f} ms per call  "
                  f"new-kernel launches {K.dgrad_ws_launches() - n0}/{4 * (reps + 1)}", flush=True)


if __name__ == "__main__":
    main()
