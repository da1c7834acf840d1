"""Per-shape A/B of the forward GEMMs gemm_fwd_ws_kernel takes (csrc/gemm_fwd_ws.hip) against the LDS-DMA kernel:
    python tools/gemm_fwd_ws_bench.py conv Bn T1 F1 D [--rounds R] [--reps N] [--timeout S]
    python tools/gemm_fwd_ws_bench.py lin M N K      [--rounds R] [--reps N] [--timeout S]
conv: the conv2 forward of Conv2dSubsampling.fwd, z2 (Bn T2 F2, D) = relu(im2col(z1) W2r^T + b), A = the conv1 map z1
(Bn, T1, F1, D), NHWC, in I2C_KC mode, B = the (D, 9 D) weight as split planes.  lin: the FFN w_2 forward,
C = 0.5 drop_0.1(A W^T + b) + R with A (M, K), W (N, K) as split planes.

The driver alternates esp_set_fwd_ws modes 0 (the LDS-DMA kernel) and 2 (gemm_fwd_ws_kernel whenever eligible) over
--rounds rounds (default 2).  Every measurement is a fresh child process under its own time limit (--timeout, default
120 s); the first child that fails or runs out of time ends the run.  A child (--child --ws MODE: also the program of
a counters-only profiler pass) warms up, times --reps calls (default 20) with events and prints one line; the shape
and the TF/s come from the shape arithmetic, and the line says how many calls ran the new kernel."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt(argv, name, default, conv=int):
    if name in argv:
        i = argv.index(name)
        v = conv(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def child(kind, dims, mode, reps):
    sys.path.insert(0, ROOT)
    import torch

    from espnet_slurp_amd import kernels as K

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "conv":
        Bn, T1, F1, D = dims
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        M, N, Kd = Bn * T2 * F2, D, 9 * D
        z1 = torch.randn(Bn * T1 * F1 * D, device=dev, generator=g).relu_()  # (the conv1 map is a ReLU output)
        W = torch.randn(D, 9 * D, device=dev, generator=g) / (3.0 * D ** 0.5)
        b = torch.randn(D, device=dev, generator=g)
        out = torch.empty(M, D, device=dev)
        fn = lambda: K.gemm(M, D, 9 * D, z1, W, out, mode_a=K.I2C_KC, lda=0, mode_b=K.KC, ldb=9 * D, ldc=D, bias=b,  # noqa: E731
                            act=K.ACT_RELU, ic_a=(T1, F1, D, T2, F2), b_weight=True)
    else:
        M, N, Kd = dims
        A = torch.randn(M, Kd, device=dev, generator=g)
        W = torch.randn(N, Kd, device=dev, generator=g) / Kd ** 0.5
        b = torch.randn(N, device=dev, generator=g)
        R = torch.randn(M, N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev)
        fn = lambda: K.gemm(M, N, Kd, A, W, out, mode_a=K.KC, lda=Kd, mode_b=K.KC, ldb=Kd, ldc=N, bias=b, alpha=0.5,  # noqa: E731
                            beta=1.0, R=R, drop_p=0.1, seed=7, b_weight=True)
    K.set_fwd_ws(mode)
    with K.param_cast_scope():  # (the weight's planes are made once, as in a training step)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n0 = K.fwd_ws_launches()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    shape = ",".join(str(d) for d in dims)
    print(f"{kind} ({shape}) fwd_ws={mode} M={M} N={N} K={Kd}: {us:.1f} us  {2.0 * M * N * Kd / us / 1e6:.1f} TF/s  "
          f"new-kernel launches {K.fwd_ws_launches() - n0}/{reps}", flush=True)


def main():
    argv = sys.argv[1:]
    rounds, reps, limit = _opt(argv, "--rounds", 2), _opt(argv, "--reps", 20), _opt(argv, "--timeout", 120)
    mode = _opt(argv, "--ws", None)
    is_child = "--child" in argv
    a = [x for x in argv if not x.startswith("--")]
    kind, dims = a[0], [int(v) for v in a[1:]]
    if kind not in ("conv", "lin") or len(dims) != (4 if kind == "conv" else 3) or rounds < 2:
        raise SystemExit(__doc__)
    if is_child:
        return child(kind, dims, 1 if mode is None else mode, reps)
    for r in range(rounds):
        for m in (0, 2):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ws", str(m), "--reps", str(reps), kind]
            try:
                rc = subprocess.run(cmd + [str(d) for d in dims], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"gemm_fwd_ws_bench: round {r} mode {m} ran past {limit} s; stopping")
            if rc:
                raise SystemExit(f"gemm_fwd_ws_bench: round {r} mode {m} exited with {rc}; stopping")


if __name__ == "__main__":
    main()
