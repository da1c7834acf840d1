"""One conv2 weight-gradient shape, repeated (per-shape A/B timings and rocprofv3 --pmc passes):
    python tools/conv2_wgrad_bench.py Bn T1 F1 D [reps] [--ws MODE] [--no-rowsum]
dW2r (D x 9D) = dz2^T im2col(z1) with the bias gradient fused, the call of Conv2dSubsampling.bwd: A = dz2
(Bn T2 F2, D) in RC mode, B = the conv1 map z1 (Bn, T1, F1, D), NHWC, in I2C_RC mode, fp32 operands on split
products (PREC 0).  --ws 0 / 1 / 2: esp_set_wgrad_ws for the run (0: the 128-row LDS-DMA kernel, 1: the default
choice, 2: gemm_wgrad_ws_kernel whenever eligible); without it the library's current mode."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from espnet_slurp_amd import kernels as K  # noqa: E402


def main():
    argv = sys.argv[1:]
    mode = None
    if "--ws" in argv:
        i = argv.index("--ws")
        mode = int(argv[i + 1])
        del argv[i:i + 2]
    a = [x for x in argv if not x.startswith("--")]
    Bn, T1, F1, D = (int(v) for v in a[:4])
    reps = int(a[4]) if len(a) > 4 else 20
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    npix = Bn * T2 * F2
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    z1 = torch.randn(Bn * T1 * F1 * D, device=dev, generator=g).relu_()  # (the conv1 map is a ReLU output)
    dz2 = torch.randn(npix, D, device=dev, generator=g)
    dw = torch.empty(D, 9 * D, device=dev)
    rs = None if "--no-rowsum" in argv else torch.zeros(D, device=dev)
    if mode is not None:
        K.set_wgrad_ws(mode)
    fn = lambda: K.gemm(D, 9 * D, npix, dz2, z1, dw, mode_a=K.RC, lda=D, mode_b=K.I2C_RC, ldb=0, ldc=9 * D,  # noqa: E731
                        ic_b=(T1, F1, D, T2, F2), rowsum=rs)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    tag = "current" if mode is None else str(mode)
    print(f"conv2_wgrad ({Bn},{T1},{F1},{D}) ws={tag} M={D} N={9 * D} K={npix}: {us:.1f} us  "
          f"{2.0 * D * 9 * D * npix / us / 1e6:.1f} TF/s", flush=True)


if __name__ == "__main__":
    main()
