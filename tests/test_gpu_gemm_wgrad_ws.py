"""gemm_wgrad_ws_kernel (csrc/gemm_wgrad_ws.hip): the fp32 RC x RC weight-gradient GEMM with the operand split on
producer waves, against the 128-row LDS-DMA kernel it replaces (esp_set_wgrad_ws(0)) on the same inputs.

Shapes are (rows of dW, cols of dW, K = tokens).  esp_set_wgrad_ws(2) takes the new kernel for every eligible
launch (the default mode keeps small K on the old kernel).  An unsplit launch WITHOUT row sums is not eligible --
it keeps gemm_glds_kernel's specialised plain epilogues in every mode -- so for those cases the comparison is of
the old kernel with itself; with row sums, and whenever K is split, the new kernel runs."""
import pytest
import torch

from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

# one tile one slab; K tail; partial tile in both dimensions + tail; across tile edges, 8 slabs (the 2-stage ring
# wraps three times); split-K with a short last chunk (26 chunks of 160, the last 100)
SHAPES = [(256, 128, 32), (256, 128, 37), (200, 72, 95), (264, 136, 230), (512, 256, 4100)]
SLICED = (256, 128, 70)  # operands as column slices of wider tensors (ld > rows), as the dqkv slices are


def _inputs(shape, sliced=False):
    M, N, Kk = shape
    g = torch.Generator().manual_seed(1000 * M + 10 * N + Kk)
    if sliced:
        Aw = torch.randn(Kk, 3 * M, generator=g)
        Bw = torch.randn(Kk, N + 64, generator=g)
        A, B = Aw[:, M:2 * M], Bw[:, 32:32 + N]
    else:
        A, B = torch.randn(Kk, M, generator=g), torch.randn(Kk, N, generator=g)
    dW0 = torch.randn(M, N, generator=g)
    rs0 = torch.randn(M, generator=g)
    return A, B, dW0, rs0


def _run(mode, A, B, dW0, rs0, rowsum, dev):
    """dW0 + A^T B (beta = 1 onto the non-zero dW0) and rs0 + column sums of A, kernel chosen by `mode`."""
    M, N = dW0.shape

    def put(t):  # (a column slice stays a slice of its wider tensor on the device)
        if t._base is None:
            return t.to(dev)
        return t._base.to(dev).as_strided(t.shape, t.stride(), t.storage_offset())

    Ad, Bd = put(A), put(B)
    C = dW0.to(dev).clone()
    rs = rs0.to(dev).clone() if rowsum else None
    prev = K.set_wgrad_ws(mode)
    try:
        K.gemm(M, N, A.shape[0], Ad, Bd, C, mode_a=K.RC, lda=Ad.stride(0), mode_b=K.RC, ldb=Bd.stride(0), ldc=N, R=C,
               beta=1.0, rowsum=rs)
        torch.cuda.synchronize()
    finally:
        K.set_wgrad_ws(prev)
    return C.cpu(), (rs.cpu() if rowsum else None)


_CACHE = {}


def _case(shape, sliced, rowsum, dev):
    key = (shape, sliced, rowsum)
    if key not in _CACHE:
        A, B, dW0, rs0 = _inputs(shape, sliced)
        old = _run(0, A, B, dW0, rs0, rowsum, dev)
        new = _run(2, A, B, dW0, rs0, rowsum, dev)
        new2 = _run(2, A, B, dW0, rs0, rowsum, dev)
        _CACHE[key] = (A, B, dW0, rs0, old, new, new2)
    return _CACHE[key]


CASES = [(s, False) for s in SHAPES] + [(SLICED, True)]


@pytest.mark.parametrize("rowsum", [False, True], ids=["plain", "rowsum"])
@pytest.mark.parametrize("shape,sliced", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}{'-sliced' if sl else ''}" for s, sl in CASES])
def test_wgrad_ws_matches_old_kernel(dev, shape, sliced, rowsum):
    """Split-K off (K < 256): C bit-identical to the old kernel's.  Split-K on (the split counts differ: one unit
    per CU instead of two): the fp32 accuracy gate of test_gemm_f32_accuracy_vs_fp64 -- error / (|A|^T |B| + |dW0|)
    against fp64 within 2x (max) and 4x (rms) of the host's own fp32 matmul.  Row sums: error against the fp64
    column sums within 2x the old kernel's on the same input (max and rms; the summation order changed)."""
    A, B, dW0, rs0, (C_old, rs_old), (C_new, rs_new), _ = _case(shape, sliced, rowsum, dev)
    Kk = shape[2]
    if Kk < 256:
        assert torch.equal(C_new, C_old)
    else:
        ref = dW0.double() + A.double().t() @ B.double()
        den = A.double().abs().t() @ B.double().abs() + dW0.double().abs()
        r = (C_new.double() - ref).abs() / den
        r32 = ((dW0 + A.t() @ B).double() - ref).abs() / den
        print(f"split-K {shape}: max {r.max().item():.3e} (host fp32 {r32.max().item():.3e}) "
              f"rms {r.pow(2).mean().sqrt().item():.3e} (host fp32 {r32.pow(2).mean().sqrt().item():.3e})")
        assert r.max().item() <= 2.0 * r32.max().item(), (r.max().item(), r32.max().item())
        assert r.pow(2).mean().sqrt().item() <= 4.0 * r32.pow(2).mean().sqrt().item()
    if rowsum:
        ref = rs0.double() + A.double().sum(0)
        e_new, e_old = (rs_new.double() - ref).abs(), (rs_old.double() - ref).abs()
        print(f"rowsum {shape}: max {e_new.max().item():.3e} (old {e_old.max().item():.3e}) "
              f"rms {e_new.pow(2).mean().sqrt().item():.3e} (old {e_old.pow(2).mean().sqrt().item():.3e})")
        assert e_new.max().item() <= 2.0 * e_old.max().item()
        assert e_new.pow(2).mean().sqrt().item() <= 2.0 * e_old.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("rowsum", [False, True], ids=["plain", "rowsum"])
@pytest.mark.parametrize("shape,sliced", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}{'-sliced' if sl else ''}" for s, sl in CASES])
def test_wgrad_ws_deterministic(dev, shape, sliced, rowsum):
    """The same call twice: bitwise equal C and row sums (fixed-order sums, no atomics)."""
    *_, (C_new, rs_new), (C_new2, rs_new2) = _case(shape, sliced, rowsum, dev)
    assert torch.equal(C_new, C_new2)
    if rowsum:
        assert torch.equal(rs_new, rs_new2)


@pytest.mark.parametrize("shape", [(256, 128, 37), (264, 136, 230), (512, 256, 4100)], ids=str)
def test_wgrad_ws_nonfinite_operands(dev, shape):
    """inf / NaN operand elements (one of them in the last k-row, which the K tail's clamped reads repeat) give
    non-finite outputs in the positions where the old kernel gives them, in C and in the row sums."""
    M, N, Kk = shape
    A, B, dW0, rs0 = _inputs(shape)
    A, B = A.clone(), B.clone()
    A[5, 7] = float("nan")
    A[Kk - 1, 70] = float("inf")
    B[3, 9] = float("-inf")
    B[Kk - 1, 40] = float("inf")
    C_old, rs_old = _run(0, A, B, dW0, rs0, True, dev)
    C_new, rs_new = _run(2, A, B, dW0, rs0, True, dev)
    assert not torch.isfinite(C_new).all()
    assert torch.equal(torch.isfinite(C_new), torch.isfinite(C_old))
    assert torch.equal(torch.isfinite(rs_new), torch.isfinite(rs_old))
    fin = torch.isfinite(C_old)
    if Kk < 256:
        assert torch.equal(C_new[fin], C_old[fin])
