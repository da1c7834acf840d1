"""The conv2 weight gradient on gemm_wgrad_ws_kernel's gathered-B producers (csrc/gemm_wgrad_ws.hip, RC x I2C_RC:
dW2r (C x 9C) += g^T im2col(z1), the bias gradient fused as A's row sums), against the 128-row LDS-DMA kernel it
replaces (esp_set_wgrad_ws(0)) on the same inputs.

z1 is the conv1 map (Bn, T1, F1, C) in NHWC, g the gradient (Bn T2 F2, C) at conv2's output pixels (3 x 3, stride 2,
no padding).  esp_set_wgrad_ws(2) takes the new kernel for every eligible launch.  As for the Linear shapes, an unsplit
launch WITHOUT row sums is not eligible in any mode, so there the comparison is of the old kernel with itself; with
row sums, and whenever K is split, the new kernel runs.  Mode 0 runs the LDS-DMA kernel on every case here (case c
too: C = 12 keeps whole 16-byte quads in both operands), so no unsplit case is excused from bit-identity."""
import math

import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

# z1 shapes (Bn, T1, F1, C):
#  a  K = 4: one slab with a 4-row K tail; nine column tiles, each exactly one tap
#  b  K = 231: seven slabs + a 7-row tail (the ring wraps); the decode crosses map rows and utterances; a tile spans
#     four taps; the last tile is partial
#  c  even F1 (the last input column is never read), C % 32 != 0
#  d  M = 264: two row tiles, the second partial; 19 column tiles over the persistent grid
#  e  K = 2244: split-K with a short last chunk
SHAPES = {"a": (1, 5, 5, 128), "b": (3, 23, 15, 32), "c": (2, 21, 14, 12), "d": (2, 9, 7, 264), "e": (4, 67, 35, 64)}
SPLIT = {"e"}


def _out(n):
    return (n - 3) // 2 + 1


def _inputs(name):
    Bn, T1, F1, C = SHAPES[name]
    gen = torch.Generator().manual_seed(7 + ord(name))
    z1 = torch.randn(Bn, T1, F1, C, generator=gen)
    g = torch.randn(Bn * _out(T1) * _out(F1), C, generator=gen)
    dW0 = torch.randn(C, 9 * C, generator=gen)
    rs0 = torch.randn(C, generator=gen)
    return z1, g, dW0, rs0


def _cols(z1):
    """im2col(z1) in fp64: (Bn T2 F2, 9 C), columns ordered (kt, kf, c)."""
    Bn, T1, F1, C = z1.shape
    cols = F.unfold(z1.double().permute(0, 3, 1, 2), 3, stride=2)  # (Bn, C * 9, L) ordered (c, kt, kf)
    return cols.view(Bn, C, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(-1, 9 * C)


def _run(mode, z1, g, dW0, rs0, rowsum, dev):
    """dW0 + g^T im2col(z1) (beta = 1 onto the non-zero dW0) and rs0 + column sums of g, kernel chosen by `mode`."""
    Bn, T1, F1, C = z1.shape
    T2, F2 = _out(T1), _out(F1)
    z1d, gd = z1.to(dev).contiguous(), g.to(dev)
    dW = dW0.to(dev).clone()
    rs = rs0.to(dev).clone() if rowsum else None
    prev = K.set_wgrad_ws(mode)
    try:
        K.gemm(C, 9 * C, Bn * T2 * F2, gd, z1d, dW, mode_a=K.RC, lda=C, mode_b=K.I2C_RC, ldb=0, ldc=9 * C, R=dW, beta=1.0,
               ic_b=(T1, F1, C, T2, F2), rowsum=rs)
        torch.cuda.synchronize()
    finally:
        K.set_wgrad_ws(prev)
    return dW.cpu(), (rs.cpu() if rowsum else None)


_CACHE = {}


def _case(name, rowsum, dev):
    key = (name, rowsum)
    if key not in _CACHE:
        z1, g, dW0, rs0 = _inputs(name)
        old = _run(0, z1, g, dW0, rs0, rowsum, dev)
        new = _run(2, z1, g, dW0, rs0, rowsum, dev)
        new2 = _run(2, z1, g, dW0, rs0, rowsum, dev)
        _CACHE[key] = (z1, g, dW0, rs0, old, new, new2)
    return _CACHE[key]


def _splitk_gate(got, ref, den, host32, what, check=True):
    """The fp32 accuracy gate of test_gemm_f32_accuracy_vs_fp64: error / den against fp64 within 2x (max) and 4x
    (rms) of the host's own fp32 result."""
    live = den > 0  # den == 0: every product is 0 (a conv1 channel whose ReLU output is 0 everywhere), so is the sum
    assert torch.equal(got[~live].double(), ref[~live]), what
    r = ((got.double() - ref).abs() / den)[live]
    r32 = ((host32.double() - ref).abs() / den)[live]
    print(f"{what}: max {r.max().item():.3e} (host fp32 {r32.max().item():.3e}) "
          f"rms {r.pow(2).mean().sqrt().item():.3e} (host fp32 {r32.pow(2).mean().sqrt().item():.3e})")
    if check:
        assert r.max().item() <= 2.0 * r32.max().item(), (what, r.max().item(), r32.max().item())
        assert r.pow(2).mean().sqrt().item() <= 4.0 * r32.pow(2).mean().sqrt().item(), what


@pytest.mark.parametrize("rowsum", [False, True], ids=["plain", "rowsum"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv2_wgrad_ws_matches_old_kernel(dev, name, rowsum):
    """Unsplit (a-d): dW bit-identical to the old kernel's.  Split-K (e; the split counts differ): the accuracy gate
    against the fp64 reference g^T unfold(z1).  Row sums: error against the fp64 column sums of g within 2x the old
    kernel's on the same input (max and rms; the summation order changed)."""
    z1, g, dW0, rs0, (C_old, rs_old), (C_new, rs_new), _ = _case(name, rowsum, dev)
    if name not in SPLIT:
        assert torch.equal(C_new, C_old)
    cols = _cols(z1)
    ref = dW0.double() + g.double().t() @ cols
    den = g.double().abs().t() @ cols.abs() + dW0.double().abs()
    host32 = dW0 + g.t() @ cols.float()
    if name in SPLIT:
        _splitk_gate(C_new, ref, den, host32, f"split-K {name}")
    else:  # (the bit-identical result is also the right one)
        assert ((C_new.double() - ref).abs() / den).max().item() < 1e-5
    if rowsum:
        ref = rs0.double() + g.double().sum(0)
        e_new, e_old = (rs_new.double() - ref).abs(), (rs_old.double() - ref).abs()
        print(f"rowsum {name}: max {e_new.max().item():.3e} (old {e_old.max().item():.3e}) "
              f"rms {e_new.pow(2).mean().sqrt().item():.3e} (old {e_old.pow(2).mean().sqrt().item():.3e})")
        assert e_new.max().item() <= 2.0 * e_old.max().item()
        assert e_new.pow(2).mean().sqrt().item() <= 2.0 * e_old.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("rowsum", [False, True], ids=["plain", "rowsum"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv2_wgrad_ws_deterministic(dev, name, rowsum):
    """The same call twice: bitwise equal dW and row sums (fixed-order sums, no atomics)."""
    *_, (C_new, rs_new), (C_new2, rs_new2) = _case(name, rowsum, dev)
    assert torch.equal(C_new, C_new2)
    if rowsum:
        assert torch.equal(rs_new, rs_new2)


@pytest.mark.parametrize("name", ["b", "d", "e"])
def test_conv2_wgrad_ws_nonfinite_operands(dev, name):
    """inf / NaN elements in g and in z1 -- one of z1's in the last output pixel's receptive field, which the K tail's
    clamped reads repeat, one of g's in its last row -- give non-finite outputs exactly where the old kernel gives
    them, in dW and in the row sums."""
    z1, g, dW0, rs0 = _inputs(name)
    z1, g = z1.clone(), g.clone()
    Bn, T1, F1, C = z1.shape
    T2, F2 = _out(T1), _out(F1)
    g[5, 7] = float("nan")
    g[g.shape[0] - 1, C - 2] = float("inf")
    z1[0, 2, 3, 9] = float("-inf")
    z1[Bn - 1, 2 * (T2 - 1) + 1, 2 * (F2 - 1) + 2, C // 2] = float("nan")  # tap (1, 2) of the last output pixel
    C_old, rs_old = _run(0, z1, g, dW0, rs0, True, dev)
    C_new, rs_new = _run(2, z1, g, dW0, rs0, True, dev)
    assert not torch.isfinite(C_new).all()
    assert torch.equal(torch.isfinite(C_new), torch.isfinite(C_old))
    assert torch.equal(torch.isfinite(rs_new), torch.isfinite(rs_old))
    if name not in SPLIT:
        fin = torch.isfinite(C_old)
        assert torch.equal(C_new[fin], C_old[fin])


def test_conv2_wgrad_ws_subsampling_bwd(dev, monkeypatch):
    """Conv2dSubsampling.bwd (D = 64, B = 2, 67 frames: K = 2 * 16 * 19 = 608 output pixels, split-K) with the conv2
    weight gradient under modes 0 and 2: conv.2.weight.grad and conv.2.bias.grad (accumulated onto zero) within the
    split-K gate against fp64 on the operands the block hands the GEMM (dz2 and the conv1 map, captured at the call), the
    bias gradient also within the row-sum rule (2x mode 0's error), every other gradient bitwise equal between the
    two runs.  The mode is set around the block's RC x I2C_RC call alone: set for the whole backward, mode 2 would
    also move the output Linear's weight gradient (RC x RC, K = 32, fused bias gradient) onto the producer kernel,
    whose row sums are taken in another order (tests/test_gpu_gemm_wgrad_ws.py), so out.0.bias.grad would differ in
    its last bits for a reason that is not the conv2 weight gradient's."""
    from espnet_slurp_amd.blocks import Conv2dSubsampling, Seeds
    from espnet_slurp_amd.flat import FlatParams

    torch.manual_seed(5)
    B, T, Fd, D = 2, 67, 80, 64
    mod = Conv2dSubsampling(Fd, D).to(dev)
    with torch.no_grad():
        for p in mod.parameters():
            p.normal_(0, 0.1)
    flat = FlatParams(mod, dev)
    x = torch.randn(B, T, Fd)
    xs = math.sqrt(D)
    grads, gathered, ops = {}, [], []
    gemm = K.gemm
    for mode in (0, 2):

        def gemm_in_mode(*a, **kw):
            if kw.get("mode_b") != K.I2C_RC:
                return gemm(*a, **kw)
            gathered.append(mode)
            T1, F1, C = kw["ic_b"][:3]
            ops.append((a[3].detach().cpu().clone(), a[4].detach().cpu().view(-1, T1, F1, C).clone()))
            prev = K.set_wgrad_ws(mode)
            try:
                return gemm(*a, **kw)
            finally:
                K.set_wgrad_ws(prev)

        flat.grad.zero_()
        prev = K.set_wgrad_ws(0)
        monkeypatch.setattr(K, "gemm", gemm_in_mode)
        try:
            out, c = mod.fwd(x.to(dev), xs, 0.0, Seeds(3), True)
            if mode == 0:
                dout = torch.randn(B * c.T2, D, generator=torch.Generator().manual_seed(6))
            mod.bwd(c, dout.to(dev))
            torch.cuda.synchronize()
        finally:
            monkeypatch.setattr(K, "gemm", gemm)
            K.set_wgrad_ws(prev)
        grads[mode] = {n: p.grad.detach().cpu().clone() for n, p in mod.named_parameters()}
    assert gathered == [0, 2]  # the fp32 weight gradient ran, once per backward
    for n in grads[0]:
        if n not in ("conv.2.weight", "conv.2.bias"):
            assert torch.equal(grads[0][n], grads[2][n]), n

    # fp64 from the operands the GEMM itself was given (the same in both runs: everything before it is bitwise equal)
    assert torch.equal(ops[0][0], ops[1][0]) and torch.equal(ops[0][1], ops[1][1])
    g, z1 = ops[1]
    cols = _cols(z1)                                               # (pixels, (kt, kf, c))
    to_w = lambda m: m.view(D, 3, 3, D).permute(0, 3, 1, 2)        # noqa: E731  (o, (kt, kf, c)) -> (o, c, kt, kf)
    ref_w, den_w = to_w(g.double().t() @ cols), to_w(g.double().abs().t() @ cols.abs())
    host_w = to_w(g.t() @ cols.float())
    ref_b, den_b, host_b = g.double().sum(0), g.double().abs().sum(0), g.sum(0)
    for mode in (0, 2):  # (mode 0's figures are printed for comparison only)
        _splitk_gate(grads[mode]["conv.2.weight"], ref_w, den_w, host_w, f"mode {mode} conv.2.weight.grad", mode == 2)
        _splitk_gate(grads[mode]["conv.2.bias"], ref_b, den_b, host_b, f"mode {mode} conv.2.bias.grad", mode == 2)
    e_new = (grads[2]["conv.2.bias"].double() - ref_b).abs()
    e_old = (grads[0]["conv.2.bias"].double() - ref_b).abs()
    assert e_new.max().item() <= 2.0 * e_old.max().item()
    assert e_new.pow(2).mean().sqrt().item() <= 2.0 * e_old.pow(2).mean().sqrt().item()
