"""Kernel-level numerics on the MI355X: every HIP kernel against a plain PyTorch fp32/fp64 CPU
reference of the same op (or the oracle / golden fixtures)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K
from oracle import ctc_np
from oracle import espnet_cpu as O
from tests.helpers import golden, keep_scale, rel_err

pytestmark = pytest.mark.gpu


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _gemm_ref(A, B, ma, mb):
    A = A.double()
    B = B.double()
    a = A if ma == K.KC else A.t()
    b = B.t() if mb == K.KC else B
    return a @ b


@pytest.mark.parametrize("shape", [(1, 1, 1), (37, 53, 19), (128, 128, 16), (300, 260, 129), (1000, 96, 512),
                                   (130, 7, 3)])
@pytest.mark.parametrize("modes", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_modes(dev, shape, modes):
    M, N, Kk = shape
    ma, mb = modes
    A = _r(M, Kk, seed=1) if ma == K.KC else _r(Kk, M, seed=1)
    B = _r(N, Kk, seed=2) if mb == K.KC else _r(Kk, N, seed=2)
    C = torch.empty(M, N, device=dev)
    Ad, Bd = A.to(dev), B.to(dev)
    K.gemm(M, N, Kk, Ad, Bd, C, mode_a=ma, lda=Ad.stride(0), mode_b=mb, ldb=Bd.stride(0), ldc=N)
    ref = _gemm_ref(A, B, ma, mb)
    torch.cuda.synchronize()
    err = (C.cpu().double() - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, math.sqrt(Kk)) * 4, err


def _padded(rows, cols, pad, seed):
    """(rows, cols) values inside a (rows, cols+pad) buffer: a 16-B aligned pitch > extent."""
    buf = _r(rows, cols + pad, seed=seed)
    return buf, buf[:, :cols]


@pytest.mark.parametrize("shape", [(1, 1, 4), (130, 64, 36), (257, 200, 100), (64, 33, 1000), (384, 256, 2048),
                                   (5, 700, 64), (129, 60, 19), (300, 128, 77)])
@pytest.mark.parametrize("modes", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_lds_dma_paths(dev, shape, modes):
    """Aligned pitches select the LDS-DMA kernel: M/N/K tails, K % 4 != 0 inside a padded pitch,
    the 128x64 tile (N <= 64) and split-K (small M x N, long K)."""
    M, N, Kk = shape
    ma, mb = modes
    pad = (-Kk) % 4 + 4
    if ma == K.KC:
        Abuf, A = _padded(M, Kk, (-Kk) % 4 + 4, 21)
    else:
        Abuf, A = _padded(Kk, M, (-M) % 4 + 4, 21)
    if mb == K.KC:
        Bbuf, B = _padded(N, Kk, pad, 22)
    else:
        Bbuf, B = _padded(Kk, N, (-N) % 4 + 4, 22)
    Ad, Bd = Abuf.to(dev), Bbuf.to(dev)
    C = torch.empty(M, N, device=dev)
    K.gemm(M, N, Kk, Ad, Bd, C, mode_a=ma, lda=Ad.stride(0), mode_b=mb, ldb=Bd.stride(0), ldc=N)
    ref = _gemm_ref(A, B, ma, mb)
    torch.cuda.synchronize()
    err = (C.cpu().double() - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, math.sqrt(Kk)) * 4, err


@pytest.mark.parametrize("shape", [(2048, 1024, 256), (1024, 256, 2304), (256, 512, 47872)])
@pytest.mark.parametrize("modes", [(0, 0), (0, 1), (1, 1)])
def test_gemm_f32_accuracy_vs_fp64(dev, shape, modes):
    """The fp32 GEMM (bf16x6 split products in the default build, esp_f32_gemm_products) is as
    accurate as an fp32 GEMM: error / (|A| |B|) against fp64 within 2x (max) and 4x (rms) of the
    CPU's own fp32 matmul on the same operands (measured ratios <= 1 and <= 2.8,
    profiles/r03h_f32_gemm_accuracy.txt)."""
    M, N, Kk = shape
    ma, mb = modes
    g = torch.Generator().manual_seed(Kk + M)
    A = torch.randn(M, Kk, generator=g)
    B = torch.randn(Kk, N, generator=g)
    Ad = (A if ma == K.KC else A.t().contiguous()).to(dev)
    Bd = (B.t().contiguous() if mb == K.KC else B).to(dev)
    C = torch.empty(M, N, device=dev)
    K.gemm(M, N, Kk, Ad, Bd, C, mode_a=ma, lda=Ad.stride(0), mode_b=mb, ldb=Bd.stride(0), ldc=N)
    torch.cuda.synchronize()
    ref = A.double() @ B.double()
    den = A.double().abs() @ B.double().abs()
    r = (C.cpu().double() - ref).abs() / den
    r32 = ((A @ B).double() - ref).abs() / den
    assert r.max().item() <= 2.0 * r32.max().item(), (r.max().item(), r32.max().item())
    assert r.pow(2).mean().sqrt().item() <= 4.0 * r32.pow(2).mean().sqrt().item()


def test_gemm_f32_nonfinite_operands(dev):
    """A NaN or inf operand element makes its output row non-finite (the split of inf is NaN in
    the bf16x6 build, inf on the f32 MFMA): the Trainer's finite check sees both."""
    M, N, Kk = 64, 64, 96
    A = _r(M, Kk, seed=3)
    B = _r(N, Kk, seed=4)
    A[5, 7] = float("nan")
    A[9, 70] = float("inf")
    Ad, Bd = A.to(dev), B.to(dev)
    C = torch.empty(M, N, device=dev)
    K.gemm(M, N, Kk, Ad, Bd, C, mode_a=K.KC, lda=Kk, mode_b=K.KC, ldb=Kk, ldc=N)
    Cc = C.cpu()
    assert not torch.isfinite(Cc[5]).any() and not torch.isfinite(Cc[9]).any()
    others = torch.ones(M, dtype=torch.bool)
    others[[5, 9]] = False
    ref = (A[others].double() @ B.double().t())
    assert (Cc[others].double() - ref).abs().max().item() < 1e-4


def _with_bplanes(on, fn):
    prev = K._BPLANES
    K._BPLANES = on
    try:
        return fn()
    finally:
        K._BPLANES = prev


def test_f32_to_planes_exact_split(dev):
    """esp_f32_to_planes: hi + mid + lo == x exactly (fp64 sum) for normal x over 200 binades, and each
    part is the round-to-nearest-even bf16 of the exact residual: hi == bf16(x), mid == bf16(x - hi),
    lo == bf16(x - hi - mid) (torch's casts on the CPU; the residuals are exact fp32 differences) -- the
    definition the in-register split (split3_pair, ESP_SPLIT_DOT) must meet bit for bit.  Zeroed pitch
    padding."""
    x = (_r(37, 203, seed=5) * torch.exp2(torch.randint(-100, 100, (37, 203), generator=torch.Generator().manual_seed(6)).float()))
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -8 + 2.0 ** -16)])
    xd = x.to(dev)
    pl, ldp, ps = K.planes(xd, 0, 37, 203, 203)
    torch.cuda.synchronize()
    assert ldp == 208 and ps == 37 * 208
    p = pl.cpu().view(3, 37, 208)
    s = p[0, :, :203].double() + p[1, :, :203].double() + p[2, :, :203].double()
    assert torch.equal(s, x.double())
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    for got, want in ((p[0, :, :203], hi), (p[1, :, :203], mid), (p[2, :, :203], lo)):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not p[:, :, 203:].float().any()


@pytest.mark.parametrize("shape", [(300, 260, 128), (1000, 1024, 96), (129, 64, 200), (6000, 256, 192)])
@pytest.mark.parametrize("mb", [0, 1])
def test_gemm_b_planes_bit_exact(dev, shape, mb):
    """B as its three split planes (esp_gemm_f32_bp) gives the in-register split's result bit for bit
    (same six products, same order) on unsplit launches (K < 256: no split-K), with the fused
    epilogues of the weight-B call sites: forward bias + Swish + dropout + derivative (FFN w_1),
    bias + dropout + residual, input gradient * derivative (FFN w_2 backward), residual accumulation."""
    M, N, Kk = shape
    A = _r(M, Kk, seed=11).to(dev)
    B = (_r(N, Kk, seed=12) if mb == K.KC else _r(Kk, N, seed=12)).to(dev)
    bias = _r(N, seed=13).to(dev)
    R = _r(M, N, seed=14).to(dev)
    pre = _r(M, N, seed=15).to(dev)
    cases = [dict()]
    if mb == K.KC:
        cases += [dict(bias=bias, act=K.ACT_SWISH | K.ACT_AUX_DERIV, aux="aux", drop_p=0.1, seed=7),
                  dict(bias=bias, drop_p=0.1, seed=9, R=R, beta=1.0, alpha=0.5)]
    else:
        cases += [dict(bwd_act=K.ACT_MUL, pre=pre), dict(R=R, beta=1.0)]
    for kw in cases:
        outs = []
        for on in (False, True):
            C = torch.empty(M, N, device=dev)
            aux = torch.empty(M, N, device=dev) if kw.get("aux") else None
            k2 = dict(kw)
            if aux is not None:
                k2["aux"] = aux
            _with_bplanes(on, lambda: K.gemm(M, N, Kk, A, B, C, mode_a=K.KC, lda=Kk, mode_b=mb, ldb=B.stride(0), ldc=N,
                                             b_weight=True, **k2))
            outs.append((C, aux))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]), (kw.keys(), (outs[0][0] - outs[1][0]).abs().max().item())
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape", [(2048, 1024, 256), (47872 // 4, 256, 1024), (1000, 600, 2048), (512, 768, 4864)])
@pytest.mark.parametrize("mb", [0, 1])
def test_gemm_b_planes_split_k_accuracy(dev, shape, mb):
    """Long-K weight-B GEMMs (split-K may differ from the fp32-B launch): as accurate as the host's
    fp32 matmul against fp64 (the gate of test_gemm_f32_accuracy_vs_fp64) and within 2e-7 relative
    of the in-register split."""
    M, N, Kk = shape
    g = torch.Generator().manual_seed(Kk + M + mb)
    A = torch.randn(M, Kk, generator=g)
    B = torch.randn(Kk, N, generator=g)
    Bd = (B.t().contiguous() if mb == K.KC else B).to(dev)
    Ad = A.to(dev)
    Cs = []
    for on in (False, True):
        C = torch.empty(M, N, device=dev)
        _with_bplanes(on, lambda: K.gemm(M, N, Kk, Ad, Bd, C, mode_a=K.KC, lda=Kk, mode_b=mb, ldb=Bd.stride(0),
                                         ldc=N, b_weight=True))
        Cs.append(C.cpu().double())
    ref = A.double() @ B.double()
    den = A.double().abs() @ B.double().abs()
    r = (Cs[1] - ref).abs() / den
    r32 = ((A @ B).double() - ref).abs() / den
    assert r.max().item() <= 2.0 * r32.max().item(), (r.max().item(), r32.max().item())
    assert ((Cs[1] - Cs[0]).abs() / den).max().item() <= 2e-7


def test_gemm_b_planes_conv2_forward(dev):
    """The conv2 forward (implicit-im2col A, bias + ReLU epilogue) on B planes equals the fp32-B launch
    bit for bit (K = 9 C = 2304 slabs, no split-K: the grid fills the chip)."""
    Bn, H, W, C = 4, 41, 39, 64
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    z1 = _r(Bn * H * W * C, seed=31).to(dev)
    w = _r(C, 9 * C, seed=32, scale=0.05).to(dev)
    bias = _r(C, seed=33).to(dev)
    outs = []
    for on in (False, True):
        out = torch.empty(Bn * Ho * Wo, C, device=dev)
        _with_bplanes(on, lambda: K.gemm(Bn * Ho * Wo, C, 9 * C, z1, w, out, mode_a=K.I2C_KC, lda=0, mode_b=K.KC,
                                         ldb=9 * C, ldc=C, bias=bias, act=K.ACT_RELU, ic_a=(H, W, C, Ho, Wo),
                                         b_weight=True))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_gemm_epilogue(dev):
    M, N, Kk = 257, 130, 64
    X, W, b = _r(M, Kk, seed=3), _r(N, Kk, seed=4), _r(N, seed=5)
    R = _r(M, N, seed=6)
    Xd, Wd, bd, Rd = X.to(dev), W.to(dev), b.to(dev), R.to(dev)
    out = torch.empty(M, N, device=dev)
    aux = torch.empty(M, N, device=dev)
    K.linear_fwd(Xd, Wd, bd, out, act=K.ACT_SWISH, aux=aux, alpha=0.5, R=Rd, beta=1.0)
    pre = X.double() @ W.double().t() + b.double()
    ref = 0.5 * pre * torch.sigmoid(pre) + R.double()
    assert (aux.cpu().double() - pre).abs().max() < 1e-4
    assert (out.cpu().double() - ref).abs().max() < 1e-4
    # relu + dropout: deterministic in (seed, index), keep rate ~ 1-p, scale 1/(1-p)
    o1 = torch.empty(M, N, device=dev)
    o2 = torch.empty(M, N, device=dev)
    K.linear_fwd(Xd, Wd, bd, o1, act=K.ACT_RELU, drop_p=0.25, seed=1234)
    K.linear_fwd(Xd, Wd, bd, o2, act=K.ACT_RELU, drop_p=0.25, seed=1234)
    assert torch.equal(o1, o2)
    relu = torch.relu(pre).float()
    o1c = o1.cpu()
    kept = o1c != 0
    pos = relu > 0
    frac = (kept & pos).sum().item() / pos.sum().item()
    assert abs(frac - 0.75) < 0.02, frac
    assert torch.allclose(o1c[kept], relu[kept] * keep_scale(0.25), atol=1e-4)
    # the element-wise backward regenerates the same mask
    g = torch.ones(M, N, device=dev)
    dx = torch.empty(M, N, device=dev)
    K.act_bwd(g, aux, dx, K.ACT_NONE, drop_p=0.25, seed=1234)
    assert torch.equal((dx.cpu() != 0) & pos, o1c != 0)


@pytest.mark.parametrize("act", [K.ACT_RELU, K.ACT_SWISH])
def test_gemm_backward_activation_epilogue(dev, act):
    """dx = drop'(dy W) * act'(pre) in the GEMM epilogue == the separate act_bwd kernel path
    (positionwise_feed_forward.py:32 backward), dropout mask regenerated from the seed."""
    M, N, Kk = 300, 96, 160
    dy, W, pre = _r(M, N, seed=11), _r(N, Kk, seed=12), _r(M, Kk, seed=13)
    dyd, Wd, pred = dy.to(dev), W.to(dev), pre.to(dev)
    out = torch.empty(M, Kk, device=dev)
    K.linear_bwd_data_act(dyd, Wd, out, pred, act, drop_p=0.2, seed=77)
    ref = torch.empty(M, Kk, device=dev)
    K.linear_bwd_data(dyd, Wd, ref)
    K.act_bwd(ref, pred, ref, act, drop_p=0.2, seed=77)
    torch.cuda.synchronize()
    assert torch.equal(out == 0, ref == 0)
    assert (out - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    x = pre.double()
    g = (dy.double() @ W.double())
    mask = (ref.cpu() != 0).double() * keep_scale(0.2)
    d = torch.where(x > 0, 1.0, 0.0) if act == K.ACT_RELU else torch.sigmoid(x) * (1 + x * (1 - torch.sigmoid(x)))
    assert (out.cpu().double() - g * mask * d).abs().max().item() < 1e-4


@pytest.mark.parametrize("act", [K.ACT_RELU, K.ACT_SWISH])
@pytest.mark.parametrize("M,N,Kk", [(300, 96, 160), (1000, 1024, 256)])
def test_gemm_aux_derivative_then_multiply(dev, act, M, N, Kk):
    """FFN path: the w_1 forward epilogue stores h = drop(act(v)) and dh/dv = keep*scale*act'(v)
    (ACT_AUX_DERIV); the w_2 input-gradient epilogue multiplies by it (ACT_MUL).  Equals the
    pre-activation path (aux = v, bwd_act = act with the mask regenerated)."""
    X, W1, b1 = _r(M, Kk, seed=21), _r(N, Kk, seed=22), _r(N, seed=23)
    dz, W2 = _r(M, Kk, seed=24), _r(Kk, N, seed=25)
    Xd, W1d, b1d, dzd, W2d = X.to(dev), W1.to(dev), b1.to(dev), dz.to(dev), W2.to(dev)
    h1, pre = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    h2, der = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    K.linear_fwd(Xd, W1d, b1d, h1, act=act, aux=pre, drop_p=0.1, seed=99)
    K.linear_fwd(Xd, W1d, b1d, h2, act=act | K.ACT_AUX_DERIV, aux=der, drop_p=0.1, seed=99)
    assert torch.equal(h1, h2)
    v = pre.cpu().double()
    keep = (h1.cpu() != 0) | (v <= 0 if act == K.ACT_RELU else torch.zeros_like(v, dtype=torch.bool))
    d = torch.where(v > 0, 1.0, 0.0) if act == K.ACT_RELU else torch.sigmoid(v) * (1 + v * (1 - torch.sigmoid(v)))
    ref_der = torch.where(der.cpu() != 0, d * keep_scale(0.1), 0.0)
    assert (der.cpu().double() - ref_der).abs().max().item() < 1e-5
    assert torch.equal((der.cpu() != 0), keep & (d != 0))
    g1, g2 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    K.linear_bwd_data_act(dzd, W2d, g1, pre, act, drop_p=0.1, seed=99)
    K.linear_bwd_data_act(dzd, W2d, g2, der, K.ACT_MUL)
    torch.cuda.synchronize()
    assert torch.equal(g1 == 0, g2 == 0)
    assert (g1 - g2).abs().max().item() <= 2e-6 * max(1.0, g1.abs().max().item())


@pytest.mark.parametrize("M,N,Kk,pad", [(64, 48, 40, 0), (23936 // 8, 256, 64, 0), (5000, 100, 36, 0),
                                        (777, 33, 20, 3)])
def test_gemm_weight_grad_fused_bias(dev, M, N, Kk, pad):
    """dW = dy^T x with db = colsum(dy) fused in the same GEMM (split-K and not; pad != 0 makes
    the pitch unaligned and selects the register-staged kernel + the separate row-sum kernel)."""
    dyb = _r(M, N + pad, seed=14)
    dy = dyb[:, :N]
    x = _r(M, Kk, seed=15)
    dyd, xd = dyb.to(dev), x.to(dev)
    dW = torch.full((N, Kk), 0.5, device=dev)
    db = torch.full((N,), 0.25, device=dev)
    K.gemm(N, Kk, M, dyd, xd, dW, mode_a=K.RC, lda=N + pad, mode_b=K.RC, ldb=Kk, ldc=Kk, R=dW, beta=1.0, rowsum=db)
    torch.cuda.synchronize()
    refW = dy.double().t() @ x.double() + 0.5
    refb = dy.double().sum(0) + 0.25
    assert (dW.cpu().double() - refW).abs().max().item() <= 1e-5 * math.sqrt(M) * 4
    assert (db.cpu().double() - refb).abs().max().item() <= 1e-5 * math.sqrt(M) * 4


@pytest.mark.parametrize("M,N,Kk,batch", [(256, 1024, 47872 // 8, 1), (300, 260, 4000, 1), (96, 40, 3000, 3),
                                          (130, 64, 2048, 2)])
@pytest.mark.parametrize("inkernel", [0, 1])
def test_gemm_splitk_combine(dev, M, N, Kk, batch, inkernel):
    """Split-K with the separate reduction launch (0) and the in-kernel combine (1: write-through
    partials, arrival tickets, the last unit sums the splits in fixed order): equals the fp64
    product, is bit-identical run to run, leaves every ticket re-armed to 0, and runs the generic
    fused epilogue (bias + Swish + aux) after the combine.  Batched z and ragged tiles included."""
    prev = K.set_splitk_mode(inkernel)
    try:
        _splitk_case(dev, M, N, Kk, batch)
    finally:
        K.set_splitk_mode(prev)


def _splitk_case(dev, M, N, Kk, batch):
    A, B = _r(batch, M, Kk, seed=41), _r(batch, N, Kk, seed=42)
    Ad, Bd = A.to(dev), B.to(dev)
    C1 = torch.empty(batch, M, N, device=dev)
    C2 = torch.empty(batch, M, N, device=dev)
    for C in (C1, C2):
        K.gemm(M, N, Kk, Ad, Bd, C, mode_a=K.KC, lda=Kk, mode_b=K.KC, ldb=Kk, ldc=N, batch=batch,
               sa=(M * Kk, 0), sb=(N * Kk, 0), sc=(M * N, 0))
    torch.cuda.synchronize()
    ref = A.double() @ B.double().transpose(1, 2)
    assert (C1.cpu().double() - ref).abs().max().item() <= 1e-5 * math.sqrt(Kk) * 4
    assert torch.equal(C1, C2)
    ws = K._GEMM_WS.get(K._GEMM_WS_BYTES, dev)
    tickets = ws[K._GEMM_WS_BYTES - 65536:K._GEMM_WS_BYTES].view(torch.int32)
    assert int(tickets.abs().sum().item()) == 0
    if batch == 1:  # generic epilogue after the combine
        b = _r(N, seed=43)
        out, aux = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        K.linear_fwd(Ad[0], Bd[0], b.to(dev), out, act=K.ACT_SWISH, aux=aux)
        pre = ref[0] + b.double()
        torch.cuda.synchronize()
        tol = 1e-5 * math.sqrt(Kk) * 4
        assert (aux.cpu().double() - pre).abs().max().item() <= tol
        assert (out.cpu().double() - pre * torch.sigmoid(pre)).abs().max().item() <= 2 * tol


def test_colsum_shapes_and_pitches(dev):
    for (M, N, ld) in [(23936 // 4, 256, 256), (1001, 1024, 1024), (37, 30, 33), (3, 5, 8)]:
        x = _r(M, ld, seed=16)
        out = torch.full((N,), 1.0, device=dev)
        K.colsum(x.to(dev), out, accumulate=True, M=M, N=N, ld=ld)
        torch.cuda.synchronize()
        ref = x[:, :N].double().sum(0) + 1.0
        assert (out.cpu().double() - ref).abs().max().item() < 1e-4 * math.sqrt(M)


def test_gemm_batched_strided(dev):
    # attention-style (head, batch) strides: q (B*T, 3D) read per (h,b)
    B, T, H, dk = 3, 50, 4, 16
    D = H * dk
    qkv = _r(B * T, 3 * D, seed=7)
    qd = qkv.to(dev)
    S = torch.empty(H * B * T * T, device=dev)
    K.gemm(T, T, dk, qd, qd, S, mode_a=K.KC, lda=3 * D, mode_b=K.KC, ldb=3 * D, ldc=T, b_off=D,
           batch=H * B, nb2=B, sa=(dk, T * 3 * D), sb=(dk, T * 3 * D), sc=(B * T * T, T * T))
    q = qkv[:, :D].view(B, T, H, dk).permute(2, 0, 1, 3).double()
    k = qkv[:, D:2 * D].view(B, T, H, dk).permute(2, 0, 1, 3).double()
    ref = q @ k.transpose(-1, -2)
    assert (S.cpu().view(H, B, T, T).double() - ref).abs().max() < 1e-4


def test_gemm_im2col_conv(dev):
    Bn, T1, F1, C = 2, 21, 13, 8
    x = _r(Bn, C, T1, F1, seed=8)
    w = _r(C, C, 3, 3, seed=9)
    b = _r(C, seed=10)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2))  # (Bn, C, T2, F2)
    T2, F2 = ref.shape[2], ref.shape[3]
    z1 = x.permute(0, 2, 3, 1).contiguous().to(dev)  # NHWC
    w2r = w.permute(0, 2, 3, 1).contiguous().to(dev)  # (o, kt, kf, c)
    out = torch.empty(Bn * T2 * F2, C, device=dev)
    K.gemm(Bn * T2 * F2, C, 9 * C, z1, w2r, out, mode_a=K.I2C_KC, lda=0, mode_b=K.KC, ldb=9 * C, ldc=C,
           bias=b.to(dev), act=K.ACT_RELU, ic_a=(T1, F1, C, T2, F2))
    got = out.cpu().view(Bn, T2, F2, C).permute(0, 3, 1, 2).double()
    assert (got - ref).abs().max() < 1e-4
    # weight-gradient form: dW[o, kk] = sum_pix g[pix, o] * col[pix, kk]
    g = _r(Bn * T2 * F2, C, seed=11)
    dw = torch.empty(C, 9 * C, device=dev)
    K.gemm(C, 9 * C, Bn * T2 * F2, g.to(dev), z1, dw, mode_a=K.RC, lda=C, mode_b=K.I2C_RC, ldb=0, ldc=9 * C,
           ic_b=(T1, F1, C, T2, F2))
    cols = F.unfold(x.double(), 3, stride=2)  # (Bn, C*9, L) ordered (c, kt, kf)
    cols = cols.view(Bn, C, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(Bn * T2 * F2, 9 * C)
    ref_dw = g.double().t() @ cols
    assert (dw.cpu().double() - ref_dw).abs().max() < 1e-3


@pytest.mark.parametrize("C", [32, 12])
def test_gemm_im2col_lds_dma(dev, C):
    """conv2-shaped implicit im2col through the LDS-DMA kernel (C % 32 == 0 keeps a slab inside
    one tap; C = 12 crosses taps inside a slab)."""
    Bn, T1, F1 = 3, 23, 15
    x = _r(Bn, C, T1, F1, seed=31)
    w = _r(C, C, 3, 3, seed=32)
    ref = F.conv2d(x.double(), w.double(), None, stride=2)
    T2, F2 = ref.shape[2], ref.shape[3]
    z1 = x.permute(0, 2, 3, 1).contiguous().to(dev)
    w2r = w.permute(0, 2, 3, 1).contiguous().to(dev)
    out = torch.empty(Bn * T2 * F2, C, device=dev)
    K.gemm(Bn * T2 * F2, C, 9 * C, z1, w2r, out, mode_a=K.I2C_KC, lda=0, mode_b=K.KC, ldb=9 * C, ldc=C,
           ic_a=(T1, F1, C, T2, F2))
    got = out.cpu().view(Bn, T2, F2, C).permute(0, 3, 1, 2).double()
    assert (got - ref).abs().max() < 1e-4
    g = _r(Bn * T2 * F2, C, seed=33)
    dw = torch.empty(C, 9 * C, device=dev)
    K.gemm(C, 9 * C, Bn * T2 * F2, g.to(dev), z1, dw, mode_a=K.RC, lda=C, mode_b=K.I2C_RC, ldb=0, ldc=9 * C,
           ic_b=(T1, F1, C, T2, F2))
    cols = F.unfold(x.double(), 3, stride=2)
    cols = cols.view(Bn, C, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(Bn * T2 * F2, 9 * C)
    assert (dw.cpu().double() - g.double().t() @ cols).abs().max() < 1e-3


def test_layernorm(dev):
    M, D = 333, 256
    x = _r(M, D, seed=12, scale=3.0) + 1.5
    w = _r(D, seed=13) * 0.1 + 1.0
    b = _r(D, seed=14) * 0.1
    dy = _r(M, D, seed=15)
    xt = x.double().requires_grad_(True)
    wt = w.double().requires_grad_(True)
    bt = b.double().requires_grad_(True)
    y = F.layer_norm(xt, (D,), wt, bt, 1e-12)
    y.backward(dy.double())
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    yd = torch.empty(M, D, device=dev)
    mean = torch.empty(M, device=dev)
    rstd = torch.empty(M, device=dev)
    K.layernorm_fwd(xd, wd, bd, yd, mean, rstd)
    dx = torch.zeros(M, D, device=dev)
    dw = torch.zeros(D, device=dev)
    db = torch.zeros(D, device=dev)
    K.layernorm_bwd(dy.to(dev), xd, wd, mean, rstd, dx, dw, db)
    assert rel_err(yd.cpu(), y.detach()) < 1e-5
    assert rel_err(dx.cpu(), xt.grad) < 1e-5
    assert rel_err(dw.cpu(), wt.grad) < 1e-5
    assert rel_err(db.cpu(), bt.grad) < 1e-5


@pytest.mark.parametrize("Kk,T,D", [(31, 57, 64), (15, 130, 96), (9, 40, 64)])  # register-blocked 31/15, generic 9
def test_conv_module_pieces(dev, Kk, T, D):
    Bn = 3
    u = _r(Bn * T, 2 * D, seed=16)
    W = _r(D, 1, Kk, seed=17) * 0.2
    bw = _r(D, seed=18)
    gam = _r(D, seed=19) * 0.1 + 1
    bet = _r(D, seed=20) * 0.1
    ds = _r(Bn * T, D, seed=21)
    ut = u.double().requires_grad_(True)
    Wt = W.double().requires_grad_(True)
    bwt = bw.double().requires_grad_(True)
    gt = gam.double().requires_grad_(True)
    bt = bet.double().requires_grad_(True)
    g = F.glu(ut.view(Bn, T, 2 * D).transpose(1, 2), dim=1)
    y = F.conv1d(g, Wt, bwt, padding=(Kk - 1) // 2, groups=D)
    rm, rv = torch.zeros(D, dtype=torch.double), torch.ones(D, dtype=torch.double)
    z = F.batch_norm(y, rm, rv, gt, bt, training=True, momentum=0.1, eps=1e-5)
    s = z * torch.sigmoid(z)
    s.backward(ds.double().view(Bn, T, D).transpose(1, 2))
    ud = u.to(dev)
    gd = torch.empty(Bn * T, D, device=dev)
    K.glu_fwd(ud, gd)
    yd = torch.empty(Bn * T, D, device=dev)
    K.dwconv1d(gd, W.to(dev), bw.to(dev), yd, Bn, T, D, Kk)
    sd = torch.empty(Bn * T, D, device=dev)
    mean, rstd = torch.empty(D, device=dev), torch.empty(D, device=dev)
    rmd, rvd = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    K.bn_swish_fwd(yd, gam.to(dev), bet.to(dev), sd, mean, rstd, rmd, rvd)
    assert rel_err(sd.cpu(), s.detach().transpose(1, 2).reshape(Bn * T, D)) < 1e-5
    assert rel_err(rmd.cpu(), rm) < 1e-5 and rel_err(rvd.cpu(), rv) < 1e-5
    dy = torch.empty(Bn * T, D, device=dev)
    dgam, dbet = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    sums = torch.empty(2 * D, device=dev)
    K.bn_swish_bwd(ds.to(dev), yd, mean, rstd, gam.to(dev), bet.to(dev), dy, dgam, dbet, sums)
    assert rel_err(dgam.cpu(), gt.grad) < 1e-5 and rel_err(dbet.cpu(), bt.grad) < 1e-5
    dW = torch.zeros(D, 1, Kk, device=dev)
    K.dwconv1d_wgrad(dy, gd, dW, Bn, T, D, Kk)
    dbw = torch.zeros(D, device=dev)
    K.colsum(dy, dbw)
    assert rel_err(dW.cpu(), Wt.grad) < 1e-5
    # the depthwise bias feeds a training-mode BatchNorm, so its true gradient is exactly 0:
    # both sides are rounding noise; bound it absolutely (scale of the summed terms)
    assert dbw.abs().max().item() < 1e-5 * dy.abs().sum(0).max().item() + 1e-6
    dg = torch.empty(Bn * T, D, device=dev)
    K.dwconv1d(dy, W.to(dev), None, dg, Bn, T, D, Kk, flip=True)
    du = torch.empty(Bn * T, 2 * D, device=dev)
    K.glu_bwd(ud, dg, du)
    assert rel_err(du.cpu(), ut.grad) < 1e-5


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("legacy", [False, True])
def test_relpos_softmax_and_adjoint(dev, legacy, padded):
    Z, T, dk, nb = 6, 45, 16, 3
    P = T if legacy else 2 * T - 1
    ac = _r(Z, T, T, seed=22)
    bd = _r(Z, T, P, seed=23)
    klen = torch.tensor([45, 30, 7], dtype=torch.int32)
    act = ac.double().requires_grad_(True)
    bdt = bd.double().requires_grad_(True)
    sh = O.rel_shift_legacy(bdt.view(1, Z, T, P))[0] if legacy else O.rel_shift_latest(bdt.view(1, Z, T, P))[0]
    sc = (act + sh) / math.sqrt(dk)
    mask = (torch.arange(T)[None, :] < klen.long()[torch.arange(Z) % nb][:, None])[:, None, :]  # (Z,1,T)
    minv = float(np.finfo(np.float64).min)
    attn = torch.softmax(sc.masked_fill(~mask, minv), -1).masked_fill(~mask, 0.0)
    dP = _r(Z, T, T, seed=24)
    attn.backward(dP.double())
    # padded: rows live at a pitch > length (the layout the model uses, K.pitch + 4 here)
    Tp, Pp = (K.pitch(T) + 4, K.pitch(P) + 4) if padded else (T, P)

    def put(x, n, pitch):
        buf = torch.full((x.shape[0], x.shape[1], pitch), float("nan"))
        buf[:, :, :n] = x
        return buf.to(dev).contiguous()

    acd = put(ac, T, Tp)
    att = torch.full((Z * T * Tp,), float("nan"), device=dev)
    K.attn_softmax_fwd(acd, put(bd, P, Pp), 2 if legacy else 1, P, math.sqrt(dk), klen.to(dev), nb, False, att, None,
                       0.0, 0, Z, T, T, lds=Tp, ldp=Pp)
    assert rel_err(att.cpu().view(Z, T, Tp)[:, :, :T], attn.detach()) < 1e-5
    dS = put(dP, T, Tp)
    K.attn_softmax_bwd(att, dS, dS, 0.0, 0, math.sqrt(dk), Z * T, T, lds=Tp)
    assert rel_err(dS.cpu().view(Z, T, Tp)[:, :, :T], act.grad) < 1e-5
    dbd = torch.empty(Z * T * Pp, device=dev)
    K.relshift_bwd(dS, dbd, 2 if legacy else 1, Z, T, P, lds=Tp, ldp=Pp)
    assert rel_err(dbd.cpu().view(Z, T, Pp)[:, :, :P], bdt.grad) < 1e-5
    # the fused softmax-backward + rel_shift-adjoint pass gives the same dS and every dbd element
    dS2 = put(dP, T, Tp)
    dbd2 = torch.full((Z * T * Pp,), float("nan"), device=dev)
    K.attn_softmax_bwd_relpos(att, dS2, dS2, dbd2, Pp, 0.0, 0, math.sqrt(dk), Z * T, T, Tp,
                              relpos=2 if legacy else 1)
    # (the fused pass sums the row dot in quads: same terms, another order -> ulp-level differences)
    assert rel_err(dS2.cpu().view(Z, T, Tp)[:, :, :T], dS.cpu().view(Z, T, Tp)[:, :, :T]) < 1e-6
    assert rel_err(dbd2.cpu().view(Z, T, Pp)[:, :, :P], dbd.cpu().view(Z, T, Pp)[:, :, :P]) < 1e-6
    assert rel_err(dbd2.cpu().view(Z, T, Pp)[:, :, :P], bdt.grad) < 1e-5


def test_causal_softmax_with_dropout(dev):
    Z, Tq, Tk, nb = 4, 9, 9, 2
    s = _r(Z, Tq, Tk, seed=25)
    klen = torch.tensor([9, 5], dtype=torch.int32)
    sd = s.to(dev).contiguous()
    att = torch.empty(Z * Tq * Tk, device=dev)
    pd = torch.empty(Z * Tq * Tk, device=dev)
    K.attn_softmax_fwd(sd, None, 0, 0, 1.0, klen.to(dev), nb, True, att, pd, 0.5, 99, Z, Tq, Tk)
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    m = (j <= i)[None] & (j[None] < klen.long()[torch.arange(Z) % nb][:, None, None])
    ref = torch.softmax(s.masked_fill(~m, float("-inf")), -1).masked_fill(~m, 0.0)
    assert rel_err(att.cpu().view(Z, Tq, Tk), ref) < 1e-6
    a, p = att.cpu(), pd.cpu()
    kept = p != 0
    assert torch.allclose(p[kept], a[kept] * 2.0, atol=1e-6)


def test_ctc_against_golden_and_numpy(dev):
    g = golden("ctc")
    logits = torch.from_numpy(g["logits"])  # (T, B, V)
    T, B, V = logits.shape
    x = logits.permute(1, 0, 2).contiguous().to(dev)  # (B, T, V)
    lp = torch.empty(B * T, V, device=dev)
    K.log_softmax(x, lp, B * T, V)
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    grad = torch.empty(B * T, V, device=dev)
    ilen = torch.from_numpy(g["ilens"]).int().to(dev)
    tlen = torch.from_numpy(g["tlens"]).int().to(dev)
    tg = torch.from_numpy(g["targets"]).to(dev)
    K.ctc_loss(lp, tg, tg.shape[1], ilen, tlen, B, T, V, 0, 1.0 / B, True, nll, grad)
    nl = nll.cpu().numpy()
    ref = g["nll"]
    fin = np.isfinite(nl)
    assert (~fin).sum() == 1 and not np.isfinite(nl[3])  # infeasible utterance -> inf (zeroed in the loss)
    assert np.abs(nl[fin] - ref[fin]).max() < 1e-4
    gr = grad.cpu().view(B, T, V).permute(1, 0, 2).numpy()
    assert np.abs(gr - g["grad"]).max() < 1e-5
    nll_np, g_np = ctc_np.ctc_loss_np(g["logits"], g["ilens"], g["targets"], g["tlens"])
    assert np.abs(gr - g_np / B).max() < 1e-5
    out4 = torch.empty(4, device=dev)
    K.reduce_losses(nll, B, True, None, None, 0, 1.0, 1.0, out4)
    assert abs(out4[0].item() - float(g["loss"])) < 1e-4


def test_forced_align_and_argmax_bit_exact(dev):
    g = golden("align")
    for ci in range(4):
        lpz = torch.from_numpy(g[f"lpz{ci}"]).to(dev).contiguous()
        y = torch.from_numpy(g[f"y{ci}"]).to(dev)
        ali = K.ctc_forced_align(lpz, y, 0).cpu().numpy()
        assert (ali == g[f"ali{ci}"]).all(), (ci, ali, g[f"ali{ci}"])
        h = torch.from_numpy(g[f"h{ci}"]).to(dev).contiguous()
        am = torch.empty(h.shape[0], dtype=torch.int64, device=dev)
        K.argmax(h, am, h.shape[0], h.shape[1])
        assert (am.cpu().numpy() == g[f"argmax{ci}"]).all()


def test_forced_align_and_argmax_bit_exact_c2_shape(dev):
    """esp_ctc_forced_align / esp_argmax bit-exact against the reference's own forced_align and argmax at
    the C2 workload shape (align_c2.npz from make_golden.py align_c2: T' = 374, V = 600, U = 40 / 20;
    trained-like, random, quantised-tie and all-tie logits, repeated labels; the s = 0 wrap is taken on
    3-7 frames of cases 1, 2, 3 and 5)."""
    g = golden("align_c2")
    n = len(g["kinds"])
    for ci in range(n):
        lpz = torch.from_numpy(g[f"lpz{ci}"]).to(dev).contiguous()
        y = torch.from_numpy(g[f"y{ci}"]).to(dev)
        ali = K.ctc_forced_align(lpz, y, 0).cpu().numpy()
        assert (ali == g[f"ali{ci}"]).all(), (ci, str(g["kinds"][ci]), int((ali != g[f"ali{ci}"]).sum()))
        am = torch.empty(lpz.shape[0], dtype=torch.int64, device=dev)
        K.argmax(lpz, am, lpz.shape[0], lpz.shape[1])
        assert (am.cpu().numpy() == g[f"argmax{ci}"]).all(), ci
        if f"h{ci}" in g:
            h = torch.from_numpy(g[f"h{ci}"]).to(dev).contiguous()
            K.argmax(h, am, h.shape[0], h.shape[1])
            assert (am.cpu().numpy() == g[f"argmax_h{ci}"]).all(), ci


def test_forced_align_batch_matches_per_utterance(dev):
    """esp_ctc_forced_align_batch: the six align_c2 utterances in one launch, ragged (frames 374 / 300 /
    1 / ..., labels 40 / 20 / 7 / ...), each row bit-equal to the reference alignment (full rows) or to the
    oracle's on the truncated utterance, -1 past its frames; an utterance with no labels is all -1."""
    g = golden("align_c2")
    n = len(g["kinds"])
    T, V = g["lpz0"].shape
    Umax = max(len(g[f"y{ci}"]) for ci in range(n))
    lpz = np.stack([g[f"lpz{ci}"] for ci in range(n)] + [g["lpz1"]])
    ys = np.zeros((n + 1, Umax), dtype=np.int64)
    tl = [T, 300, T, 57, T, 1, T]
    ul = [len(g[f"y{ci}"]) for ci in range(n)] + [0]
    ul[3] = 7
    for ci in range(n):
        ys[ci, : len(g[f"y{ci}"])] = g[f"y{ci}"]
    out = K.ctc_forced_align_batch(torch.from_numpy(lpz).to(dev), tl, torch.from_numpy(ys).to(dev), ul, 0).cpu().numpy()
    for b in range(n + 1):
        if ul[b] == 0:
            assert (out[b] == -1).all()
            continue
        if tl[b] == T and ul[b] == len(g[f"y{b}"]):
            exp = g[f"ali{b}"]
        else:
            exp = np.array(ctc_np.forced_align_np(lpz[b, : tl[b]], ys[b, : ul[b]]), dtype=np.int64)
        assert (out[b, : tl[b]] == exp).all(), b
        assert (out[b, tl[b]:] == -1).all(), b


def test_label_smoothing_and_accuracy(dev):
    R, V = 37, 50
    x = _r(R, V, seed=26, scale=3.0)
    tgt = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(3))
    tgt[::5] = -1
    xt = x.double().requires_grad_(True)
    ref = O.label_smoothing_loss(xt.view(1, R, V), tgt.view(1, R), V, -1, 0.1)
    ref.backward()
    acc = O.th_accuracy(x, tgt.view(1, R), -1)
    xd = x.to(dev)
    grad = torch.empty(R, V, device=dev)
    rl = torch.empty(R, dtype=torch.float64, device=dev)
    rs = torch.empty(2 * R, dtype=torch.int32, device=dev)
    K.label_smoothing(xd, tgt.to(dev), V, -1, 0.1, 1.0, grad, rl, rs)
    out4 = torch.empty(4, device=dev)
    K.reduce_losses(None, 1, True, rl, rs, R, 1.0, 0.0, out4)
    assert abs(out4[1].item() - ref.item()) < 1e-4 * max(1, abs(ref.item()))
    assert abs(out4[2].item() - acc) < 1e-6
    assert rel_err(grad.cpu(), xt.grad) < 1e-5


def test_specaug_and_mvn_golden(dev):
    g = golden("specaug")
    x = torch.from_numpy(g["x"])
    B, T, F_ = x.shape
    lens = torch.full((B,), T, dtype=torch.int32).to(dev)
    for s in (3, 4):
        warp = torch.tensor([[int(g[f"tw{s}_center"]), int(g[f"tw{s}_warped"])]] * B, dtype=torch.int32)
        y = torch.empty(B, T, F_, device=dev)
        K.specaug(x.to(dev), y, lens, warp.to(dev), None, None)
        assert np.abs(y.cpu().numpy() - g[f"tw{s}_y"]).max() < 1e-5
    for key, dim in (("freq", 2), ("time", 1)):
        m = torch.from_numpy(np.stack([g[f"{key}_pos"], g[f"{key}_len"]], -1)).int().to(dev)
        y = torch.empty(B, T, F_, device=dev)
        K.specaug(x.to(dev), y, lens, None, m if key == "freq" else None, m if key == "time" else None)
        assert np.array_equal(y.cpu().numpy(), g[f"{key}_y"])
    xm = torch.from_numpy(g["mvn_x"]).to(dev).contiguous()
    K.utterance_mvn(xm, torch.from_numpy(g["mvn_lens"]).int().to(dev))
    assert np.abs(xm.cpu().numpy() - g["mvn_y"]).max() < 1e-5


def test_embed_bwd_many_rows(dev):
    """Embedding gradient over > 256 token rows (several compaction chunks per vocab row), D not
    a multiple of 256, repeated and absent tokens: equals index_add in fp64."""
    nrows, V, D = 1000, 50, 320
    g = torch.Generator().manual_seed(43)
    tok = torch.randint(0, V - 5, (nrows,), generator=g)  # the last 5 rows of dE stay untouched
    dy = _r(nrows, D, seed=44)
    dE = _r(V, D, seed=45)
    ref = dE.double().index_add(0, tok, dy.double() * 16.0)
    out = dE.to(dev)
    K.embed_bwd(tok.to(dev), dy.to(dev), out, 16.0, 0.0, 0)
    assert (out.cpu().double() - ref).abs().max().item() < 1e-4


def test_embed_bwd_grouped_rows_with_dropout_bit_exact(dev):
    """The grouped-load path of embed_bwd_kernel (EMB_GROUP = 32 matching rows of a 256-row chunk
    loaded before their adds): one token fills ~90 % of the rows (the decoder's eos padding), D not a
    multiple of 256, dropout on.  Reference: dy dropped by esp_scale_dropout (the same element
    indices r * D + d, so the same masks), then per vocab row an fp32 sum in ascending row order --
    bit-equal, since the kernel's adds stay in that order (xscale a power of two: x * xscale exact)."""
    nrows, V, D, p, seed = 1000, 40, 320, 0.1, 1234
    g = torch.Generator().manual_seed(47)
    tok = torch.randint(0, V - 3, (nrows,), generator=g)
    tok[torch.rand(nrows, generator=g) < 0.9] = 7
    dy = _r(nrows, D, seed=48)
    dE0 = _r(V, D, seed=49)
    dyd = torch.empty(nrows, D, device=dev)
    K.scale_dropout(dy.to(dev), dyd, 1.0, p, seed)
    y = (dyd.cpu().numpy() * np.float32(16.0)).astype(np.float32)
    ref = dE0.numpy().copy()
    tk = tok.numpy()
    for v in range(V):
        rows = np.nonzero(tk == v)[0]
        if len(rows) == 0:
            continue
        acc = np.zeros(D, dtype=np.float32)
        for r in rows:
            acc = (acc + y[r]).astype(np.float32)
        ref[v] = (ref[v] + acc).astype(np.float32)
    out = dE0.to(dev)
    K.embed_bwd(tok.to(dev), dy.to(dev), out, 16.0, p, seed)
    got = out.cpu().numpy()
    assert (tk == 7).sum() > 800 and np.array_equal(got, ref), np.abs(got - ref).max()


def test_specaug_time_warp_unequal_lengths(dev):
    """Per-utterance branch of TimeWarp.forward (time_warp.py:76-86): each x[b, :len_b] is warped
    with its own (center, warped), the result zero-padded (pad_list(ys, 0.0)); an utterance too
    short to warp (center 0) is copied."""
    B, T, F_ = 3, 200, 16
    x = _r(B, T, F_, seed=41)
    lens = [200, 150, 9]
    warp = [(60, 64), (100, 93), (0, 0)]
    ref = torch.zeros(B, T, F_)
    for b, (n, (c, w)) in enumerate(zip(lens, warp)):
        xb = x[b:b + 1, :n]
        ref[b, :n] = (O.time_warp_fixed(xb, c, w) if c > 0 else xb)[0]
    y = torch.empty(B, T, F_, device=dev)
    K.specaug(x.to(dev), y, torch.tensor(lens, dtype=torch.int32).to(dev),
              torch.tensor(warp, dtype=torch.int32).to(dev), None, None)
    assert (y.cpu() - ref).abs().max().item() < 1e-5


def test_adam_and_clip(dev):
    n = 1003
    p0 = _r(n, seed=27)
    gr = _r(n, seed=28) * 10
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    pd, gd = p0.to(dev), gr.to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    clip = torch.empty(3, device=dev)
    for step in range(1, 4):
        pt.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_([pt], 5.0)
        opt.step()
        K.grad_norm(gd, 5.0, clip)
        assert abs(clip[0].item() - norm.item()) < 1e-4 * norm.item()
        K.adam(pd, gd, m, v, clip, 0.01, 0.9, 0.999, 1e-8, 1e-6, step)
    assert rel_err(pd.cpu(), pt.detach()) < 1e-5
    bad = gd.clone()
    bad[7] = float("nan")
    K.grad_norm(bad, 5.0, clip)
    assert clip[2].item() == 0.0
    before = pd.clone()
    K.adam(pd, bad, m, v, clip, 0.01, 0.9, 0.999, 1e-8, 0.0, 4)
    assert torch.equal(before, pd)  # non-finite grad norm -> step skipped (trainer.py:651)


def test_subsampling_conv1_and_col2im(dev):
    Bn, T, F_, D = 2, 31, 80, 8
    x = _r(Bn, T, F_, seed=29)
    w0 = _r(D, 1, 3, 3, seed=30)
    b0 = _r(D, seed=31)
    z = torch.empty(Bn * 15 * 39 * D, device=dev)
    K.conv1_fwd(x.to(dev), w0.to(dev), b0.to(dev), z, Bn, T, F_, D)
    xt = x.double().unsqueeze(1)
    w0t = w0.double().requires_grad_(True)
    b0t = b0.double().requires_grad_(True)
    ref = F.relu(F.conv2d(xt, w0t, b0t, stride=2))
    assert rel_err(z.cpu().view(Bn, 15, 39, D).permute(0, 3, 1, 2), ref.detach()) < 1e-6
    dz = _r(Bn, 15, 39, D, seed=32)
    ref.backward(dz.double().permute(0, 3, 1, 2))
    dzm = dz.to(dev).contiguous() * (z.view(Bn, 15, 39, D) > 0)
    dW, db = torch.zeros(D, 9, device=dev), torch.zeros(D, device=dev)
    K.conv1_wgrad(x.to(dev), dzm.contiguous(), dW, db, Bn, T, F_, D)
    assert rel_err(dW.cpu().view(D, 1, 3, 3), w0t.grad) < 1e-5
    assert rel_err(db.cpu(), b0t.grad) < 1e-5


@pytest.mark.parametrize("T1,F1", [(31, 39), (32, 40), (9, 7)])
def test_conv2_dgrad_parity_classes_vs_column_path(dev, T1, F1):
    """esp_conv2_dgrad (4 implicit parity-class GEMMs, zero-page gather at the grid edges, ReLU
    mask + pixel row map in the epilogue) == the column GEMM + col2im it replaces."""
    B, D = 3, 64
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    g = torch.Generator().manual_seed(31)
    dz2 = torch.randn(B * T2 * F2, D, generator=g).to(dev)
    W = (torch.randn(D, D, 3, 3, generator=g) * 0.1).to(dev)
    z1 = torch.relu(torch.randn(B * T1 * F1 * D, generator=g)).to(dev)
    w2r = torch.empty(D * 9 * D, device=dev)
    K.permute3(W, w2r, D, D, 9)
    dcol = torch.empty(B * T2 * F2, 9 * D, device=dev)
    K.gemm(B * T2 * F2, 9 * D, D, dz2, w2r, dcol, mode_a=K.KC, lda=D, mode_b=K.RC, ldb=9 * D, ldc=9 * D)
    ref = torch.empty(B * T1 * F1 * D, device=dev)
    K.col2im_relu(dcol, z1, ref, B, T1, F1, D)
    got = torch.full((B * T1 * F1 * D,), float("nan"), device=dev)
    K.conv2_dgrad(dz2, W, z1, got, B, T1, F1, D)
    torch.cuda.synchronize()
    assert not torch.isnan(got).any()
    assert rel_err(got.cpu(), ref.cpu()) < 1e-5


@pytest.mark.parametrize("T1,F1,D", [(31, 39, 64), (32, 40, 128), (9, 7, 256)])
def test_conv2_dgrad_bits_mask_bit_exact(dev, T1, F1, D):
    """esp_conv1_fwd_bits' packed ReLU bit map is (z1 > 0) bit for bit (the same launch also writes z1 and
    its bf16 copy unchanged), and esp_conv2_dgrad_bits (the mask from the bit map) equals esp_conv2_dgrad
    (the mask from the fp32 map) exactly -- fp32 and bf16 dz2 -- at ragged grids and a padded C2 batch
    whose conv1 map has exact zeros."""
    B = 3
    T, F = 2 * T1 + 1, 2 * F1 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, T, F, generator=g)
    x[1, T // 2:] = 0.0  # padded frames: conv1 = relu(bias) there, exact zeros where the bias is <= 0
    x = x.to(dev)
    w0, b0 = (torch.randn(D, 1, 3, 3, generator=g) * 0.3).to(dev), (torch.randn(D, generator=g) * 0.1).to(dev)
    W = (torch.randn(D, D, 3, 3, generator=g) * 0.05).to(dev)
    npx = B * T1 * F1
    z1, z1b = torch.empty(npx * D, device=dev), torch.empty(npx * D, device=dev)
    z16 = torch.empty(npx * D, dtype=torch.bfloat16, device=dev)
    bits = torch.full((npx * D // 32,), -1, dtype=torch.int32, device=dev)
    K.conv1_fwd(x, w0, b0, z1, B, T, F, D)
    K.conv1_fwd(x, w0, b0, z1b, B, T, F, D, z16=z16, zbits=bits)
    torch.cuda.synchronize()
    assert torch.equal(z1, z1b)
    assert torch.equal(z16.view(torch.int16), z1.bfloat16().view(torch.int16))
    pos = (z1.view(npx, D // 32, 32) > 0).cpu().to(torch.int64)
    want = (pos << torch.arange(32, dtype=torch.int64)).sum(-1)
    assert torch.equal(bits.cpu().to(torch.int64) & 0xFFFFFFFF, want.view(-1))
    dz2 = torch.randn(B * T2 * F2, D, generator=g).to(dev)
    forms = [dict()] + ([dict(dz2_16=K.to_bf16(dz2, B * T2 * F2, D, D))] if D % 64 == 0 else [])
    for kw in forms:
        ref = torch.empty(npx * D, device=dev)
        got = torch.full((npx * D,), float("nan"), device=dev)
        with K.gemm_compute("bf16" if kw else "fp32"):
            K.conv2_dgrad(dz2, W, z1, ref, B, T1, F1, D, **kw)
            K.conv2_dgrad(None if kw else dz2, W, None, got, B, T1, F1, D, z1bits=bits, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), kw.keys()


@pytest.mark.parametrize("T1,F1,D,bf16", [(31, 39, 128, False), (20, 13, 256, False), (9, 7, 128, False),
                                           (31, 39, 128, True), (13, 17, 512, False)])
def test_conv2_dgrad_c1fold_matches_two_pass(dev, T1, F1, D, bf16):
    """esp_conv2_dgrad_c1fold (conv1's weight / bias gradient folded into the implicit conv2 input gradient's
    epilogue, dz1 never stored) against the two-pass form it replaces (esp_conv2_dgrad_bits -> dz1 ->
    esp_conv1_wgrad) and against the fp64 sums over that dz1; the fold sums in a different (fixed) order, so
    the gate is fp32 rounding.  bf16: dz2 in bf16 (the bf16 mode's class GEMMs)."""
    B = 3
    T, F = 2 * T1 + 2, 2 * F1 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    g = torch.Generator().manual_seed(43)
    x = torch.randn(B, T, F, generator=g).to(dev)
    w0, b0 = (torch.randn(D, 1, 3, 3, generator=g) * 0.3).to(dev), (torch.randn(D, generator=g) * 0.1).to(dev)
    W = (torch.randn(D, D, 3, 3, generator=g) * 0.05).to(dev)
    npx = B * T1 * F1
    z1 = torch.empty(npx * D, device=dev)
    bits = torch.empty(npx * D // 32, dtype=torch.int32, device=dev)
    K.conv1_fwd(x, w0, b0, z1, B, T, F, D, zbits=bits)
    dz2 = torch.randn(B * T2 * F2, D, generator=g).to(dev)
    kw = dict(dz2_16=K.to_bf16(dz2, B * T2 * F2, D, D)) if bf16 else {}
    dWa, dba = torch.full((D, 9), 0.25, device=dev), torch.full((D,), -0.5, device=dev)
    dWb, dbb = dWa.clone(), dba.clone()
    dz1 = torch.empty(npx * D, device=dev)
    with K.gemm_compute("bf16" if bf16 else "fp32"):
        K.conv2_dgrad(None if bf16 else dz2, W, None, dz1, B, T1, F1, D, z1bits=bits, **kw)
        K.conv1_wgrad(x, dz1, dWa, dba, B, T, F, D)
        K.conv2_dgrad_c1fold(None if bf16 else dz2, W, bits, x, T, F, dWb, dbb, B, T1, F1, D, **kw)
    torch.cuda.synchronize()
    # fp64 sums over the same dz1
    xd = x.double().cpu()
    pt = torch.stack([xd[:, kt:kt + 2 * T1 - 1:2, kf:kf + 2 * F1 - 1:2] for kt in range(3) for kf in range(3)], -1)
    dzd = dz1.double().cpu().view(B, T1, F1, D)
    wref = 0.25 + torch.einsum("btfc,btfk->ck", dzd, pt)
    bref = -0.5 + dzd.sum((0, 1, 2))
    assert rel_err(dWb.cpu(), wref) < 5e-6 and rel_err(dbb.cpu(), bref) < 5e-6
    assert rel_err(dWb.cpu(), dWa.cpu().double()) < 1e-5 and rel_err(dbb.cpu(), dba.cpu().double()) < 1e-5


@pytest.mark.parametrize("T1,F1", [(31, 39), (9, 7), (33, 40)])
def test_conv2_bf16_operands_match_staged_rounding(dev, T1, F1):
    """The bf16 mode's conv2 forward (esp_conv2_fwd_bf16: implicit im2col over conv1's bf16 copy of z1,
    bf16 weights, PREC 2) and input gradient (esp_conv2_dgrad_bf16: dz2 and the class weights in bf16)
    and weight gradient (esp_conv2_wgrad_bf16: the gathered im2col B in the bf16 RC image, fused bias
    gradient) against the same GEMMs on fp32 operands rounded to bf16 in LDS staging (PREC 1): the same
    bf16 products, fp32 accumulation-order differences only.  conv1's bf16 copy is bit-equal to torch's
    RNE."""
    B, D = 3, 128
    T, F = 2 * T1 + 1, 2 * F1 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    g = torch.Generator().manual_seed(37)
    x = torch.randn(B, T, F, generator=g).to(dev)
    w0, b0 = (torch.randn(D, 1, 3, 3, generator=g) * 0.3).to(dev), (torch.randn(D, generator=g) * 0.1).to(dev)
    W = (torch.randn(D, D, 3, 3, generator=g) * 0.05).to(dev)
    bias = (torch.randn(D, generator=g) * 0.1).to(dev)
    z1 = torch.empty(B * T1 * F1 * D, device=dev)
    z16 = torch.empty(B * T1 * F1 * D, dtype=torch.bfloat16, device=dev)
    K.conv1_fwd(x, w0, b0, z1, B, T, F, D, z16=z16)
    w2r = torch.empty(D * 9 * D, device=dev)
    K.permute3(W, w2r, D, D, 9)
    ref = torch.empty(B * T2 * F2, D, device=dev)
    got = torch.empty(B * T2 * F2, D, device=dev)
    dz2 = torch.randn(B * T2 * F2, D, generator=g).to(dev)
    dref = torch.empty(B * T1 * F1 * D, device=dev)
    dgot = torch.full((B * T1 * F1 * D,), float("nan"), device=dev)
    with K.gemm_compute("bf16"):
        K.gemm(B * T2 * F2, D, 9 * D, z1, w2r, ref, mode_a=K.I2C_KC, lda=0, mode_b=K.KC, ldb=9 * D, ldc=D,
               bias=bias, act=K.ACT_RELU, ic_a=(T1, F1, D, T2, F2))
        assert K.conv2_bf16_ok(D)
        K.conv2_fwd_bf16(z16, K.to_bf16(w2r, D, 9 * D, 9 * D), bias, got, B, T1, F1, D)
        K.conv2_dgrad(dz2, W, z1, dref, B, T1, F1, D)
        K.conv2_dgrad(dz2, W, z1, dgot, B, T1, F1, D, dz2_16=K.to_bf16(dz2, B * T2 * F2, D, D))
        # weight gradient + fused bias gradient (an even pixel count: B * T2 * F2)
        npix = B * T2 * F2
        if npix % 2 == 0:
            wref, wgot = torch.empty(D, 9 * D, device=dev), torch.empty(D, 9 * D, device=dev)
            bref, bgot = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
            K.gemm(D, 9 * D, npix, dz2, z1, wref, mode_a=K.RC, lda=D, mode_b=K.I2C_RC, ldb=0, ldc=9 * D,
                   ic_b=(T1, F1, D, T2, F2), rowsum=bref)
            K.conv2_wgrad_bf16(K.to_bf16(dz2, npix, D, D), z16, wgot, bgot, B, T1, F1, D)
    torch.cuda.synchronize()
    assert torch.equal(z16.view(torch.int16), z1.bfloat16().view(torch.int16))
    assert rel_err(got.cpu(), ref.cpu()) < 1e-5
    assert not torch.isnan(dgot).any()
    assert rel_err(dgot.cpu(), dref.cpu()) < 1e-5
    if npix % 2 == 0:
        assert rel_err(wgot.cpu(), wref.cpu()) < 1e-5
        # the fused bias gradient sums the bf16 dz2 values (torch autocast's bf16 gradient), where the
        # fp32-operand launch sums fp32 dz2
        assert rel_err(bgot.cpu(), dz2.bfloat16().double().sum(0).cpu()) < 1e-6
        assert rel_err(bref.cpu(), dz2.double().sum(0).cpu()) < 1e-6


@pytest.mark.parametrize("M,D", [(11968, 512), (3000, 768), (47872, 256)])
def test_bn_swish_large_rows_and_channels(dev, M, D):
    """BatchNorm + Swish statistics at the C4 / C5 shapes (B*T' = 32*374 rows, D = 512): the
    reduction uses up to 1536 row chunks of fp64 partials, D (2D) per chunk — the workspace the
    wrapper reserves must cover that (a D=512, B=32 undersized workspace once corrupted
    neighbouring allocations).  Forward / backward vs fp64 torch."""
    y = _r(M, D, seed=61) * 2 + 0.5
    g, b = _r(D, seed=62) * 0.1 + 1, _r(D, seed=63) * 0.1
    ds = _r(M, D, seed=64)
    yd = y.to(dev)
    s = torch.empty(M, D, device=dev)
    mean, rstd = torch.empty(D, device=dev), torch.empty(D, device=dev)
    rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    guard = torch.full((1 << 20,), 7.0, device=dev)  # allocated next: must stay untouched
    K.bn_swish_fwd(yd, g.to(dev), b.to(dev), s, mean, rstd, rm, rv)
    dy = torch.empty(M, D, device=dev)
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    sums = torch.empty(2 * D, device=dev)
    K.bn_swish_bwd(ds.to(dev), yd, mean, rstd, g.to(dev), b.to(dev), dy, dg, db, sums)
    torch.cuda.synchronize()
    assert torch.all(guard == 7.0)
    y64 = y.double().requires_grad_(True)
    mu = y64.mean(0)
    var = y64.var(0, unbiased=False)
    z = (y64 - mu) / torch.sqrt(var + 1e-5) * g.double() + b.double()
    out = z * torch.sigmoid(z)
    out.backward(ds.double())
    assert (s.cpu().double() - out.detach()).abs().max().item() < 1e-4
    assert (dy.cpu().double() - y64.grad).abs().max().item() < 1e-4 * max(1.0, y64.grad.abs().max().item())
    assert torch.isfinite(mean).all() and torch.isfinite(rm).all()


@pytest.mark.parametrize("with_r", [False, True])
def test_gemm_ragged_n_padded_rows(dev, with_r):
    """N % 4 != 0 with a row pitch padded to whole quads (the attention probability layout,
    T'=374 in rows of 376): the specialised plain epilogue stores the last quad element by
    element and never touches the padding columns."""
    Z, M, N, Kd, ld = 6, 374, 374, 64, 376
    A, B = _r(Z, M, Kd, seed=71), _r(Z, N, Kd, seed=72)
    C = torch.full((Z, M, ld), 7.5, device=dev)
    R = _r(Z, M, ld, seed=73).to(dev) if with_r else None
    R0 = R.clone() if with_r else None
    K.gemm(M, N, Kd, A.to(dev), B.to(dev), C, lda=Kd, ldb=Kd, ldc=ld, batch=Z, nb2=1, sa=(M * Kd, 0),
           sb=(N * Kd, 0), sc=(M * ld, 0), R=R, beta=1.0 if with_r else 0.0)
    ref = A.double() @ B.double().transpose(1, 2)
    if with_r:
        ref = ref + R0.cpu().double()[:, :, :N]
    out = C.cpu()
    assert (out[:, :, :N].double() - ref).abs().max().item() < 1e-4
    assert torch.all(out[:, :, N:] == 7.5)


@pytest.mark.parametrize("T", [64, 75])
def test_dropout_pair_hash_masks_agree(dev, T):
    """One hash per element pair (esp::keep_pair) and one per element (esp::keep_elem) draw the same
    mask: the float4 elementwise kernel, the scalar kernel (misaligned output), the GEMM
    bias+dropout(+residual) epilogues all keep the same (row, col) elements; the keep rate is 1 - p.
    T = 75 makes the GEMM M odd in quads of rows (the FULL / partial tile split)."""
    p, seed = 0.1, 12345
    M, N, Kk = 4 * T, 64, 32
    ones = torch.ones(M * N, device=dev)
    m4 = K.scale_dropout(ones, torch.empty_like(ones), drop_p=p, seed=seed)  # float4 pair path
    buf = torch.empty(M * N + 1, device=dev)
    m1 = K.scale_dropout(ones, buf[1:], drop_p=p, seed=seed)  # misaligned: scalar per-element path
    torch.cuda.synchronize()
    assert torch.equal(m4 != 0, m1 != 0)
    rate = (m4 != 0).float().mean().item()
    assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / (M * N))
    x = (_r(M, Kk, seed=3).abs() + 0.1).to(dev)
    W = (_r(N, Kk, seed=4).abs() + 0.1).to(dev)
    b = torch.zeros(N, device=dev)
    y0 = K.linear_fwd(x, W, b, torch.empty(M, N, device=dev))
    yd = K.linear_fwd(x, W, b, torch.empty(M, N, device=dev), drop_p=p, seed=seed)
    yr = K.linear_fwd(x, W, b, torch.empty(M, N, device=dev), drop_p=p, seed=seed,
                      R=torch.zeros(M, N, device=dev))
    torch.cuda.synchronize()
    mask = (m4 != 0).view(M, N)
    assert torch.equal(yd != 0, mask) and torch.equal(yr != 0, mask)
    assert rel_err(yd.cpu(), torch.where(mask, y0 * keep_scale(p), torch.zeros_like(y0)).cpu()) < 1e-6


def test_dropout_quantized_p_scale_and_tiny_p(dev):
    """The rescale matches the quantized keep probability (1/(1 - round(p*65536)/65536)), and a
    p below half a quantum still drops (it takes the smallest quantum, 1/65536)."""
    n = 1 << 22
    ones = torch.ones(n, device=dev)
    y = K.scale_dropout(ones, torch.empty_like(ones), drop_p=0.1, seed=7)
    kept = y[y != 0]
    assert torch.all(kept == kept[0])
    assert abs(kept[0].item() - 65536.0 / (65536 - 6554)) < 1e-6
    y = K.scale_dropout(ones, torch.empty_like(ones), drop_p=1e-7, seed=7)
    dropped = int((y == 0).sum().item())
    assert 0 < dropped < 8 * n / 65536, dropped  # ~n/65536 = 64 expected


def test_workspace_too_small_is_rejected(dev):
    """A launcher given less scratch than esp_*_workspace_bytes reports fails loudly before
    launching (no silent overrun, VERDICT r2 'weak' 8)."""
    from espnet_slurp_amd import _native
    M, N = 1000, 64
    x = torch.randn(M, N, device=dev)
    out = torch.zeros(N, device=dev)
    need = _native.workspace_bytes("esp_colsum", M, N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with pytest.raises(_native.NativeError, match="workspace"):
        _native.call("esp_colsum", x.data_ptr(), M, N, N, out.data_ptr(), 0, ws.data_ptr(), need - 4,
                     torch.cuda.current_stream().cuda_stream)
    _native.call("esp_colsum", x.data_ptr(), M, N, N, out.data_ptr(), 0, ws.data_ptr(), need,
                 torch.cuda.current_stream().cuda_stream)
    assert torch.allclose(out, x.sum(0), atol=1e-4)


def test_guard_mode_canaries(dev, monkeypatch):
    """ESP_GUARD=1: workspace launches leave their canaries intact (a BatchNorm / LayerNorm /
    GEMM step at a ragged size), and a canary overwrite is reported naming the launcher."""
    monkeypatch.setattr(K, "GUARD", True)
    M, D = 1013, 256
    y = torch.randn(M, D, device=dev)
    g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    s, mean, rstd = torch.empty_like(y), torch.empty(D, device=dev), torch.empty(D, device=dev)
    K.bn_swish_fwd(y, g, b, s, mean, rstd, None, None)
    dw, db, dx = torch.zeros(D, device=dev), torch.zeros(D, device=dev), torch.empty_like(y)
    K.layernorm_bwd(y, y, g, mean[:1].expand(M).contiguous(), rstd[:1].expand(M).contiguous(), dx, dw, db)
    K.linear_fwd(y, torch.randn(64, D, device=dev), None, torch.empty(M, 64, device=dev))
    K.check_guards()  # clean
    n = _native_ws("esp_bn_swish_fwd", M, D)
    buf = K.WS.get(n + K.GUARD_BYTES, dev)
    K.bn_swish_fwd(y, g, b, s, mean, rstd, None, None)
    buf[n + 3] = 0  # an overrun of one byte past the launcher's workspace
    K._guard_post("esp_bn_swish_fwd", buf, n)
    with pytest.raises(RuntimeError, match="esp_bn_swish_fwd"):
        K.check_guards()


def _native_ws(name, *dims):
    from espnet_slurp_amd import _native
    return _native.workspace_bytes(name, *dims)


@pytest.mark.parametrize("shape", [(300, 264, 128), (1000, 1024, 96), (136, 64, 200), (6000, 256, 192)])
@pytest.mark.parametrize("mb", [0, 1])
def test_gemm_planes_both_operands_bit_exact(dev, shape, mb):
    """A as kernels.Planes and B a weight (esp_gemm_f32_pl, both operands' planes from LDS: no split
    in the k-loop) equals the in-register split bit for bit on unsplit launches (K < 256), with the
    fused epilogues of the forward / input-gradient call sites, K tails (200) and ragged M / N."""
    M, N, Kk = shape
    A = _r(M, Kk, seed=61).to(dev)
    B = (_r(N, Kk, seed=62) if mb == K.KC else _r(Kk, N, seed=62)).to(dev)
    bias = _r(N, seed=63).to(dev)
    R = _r(M, N, seed=64).to(dev)
    pre = _r(M, N, seed=65).to(dev)
    Ap = K.Planes.of(A)
    assert torch.equal(Ap.float().cpu(), A.cpu())
    cases = [dict()]
    if mb == K.KC:
        cases += [dict(bias=bias, act=K.ACT_SWISH | K.ACT_AUX_DERIV, aux="aux", drop_p=0.1, seed=7),
                  dict(bias=bias, drop_p=0.1, seed=9, R=R, beta=1.0, alpha=0.5), dict(bias=bias)]
    else:
        cases += [dict(bwd_act=K.ACT_MUL, pre=pre), dict(R=R, beta=1.0)]
    for kw in cases:
        outs = []
        for planes in (False, True):
            C = torch.empty(M, N, device=dev)
            aux = torch.empty(M, N, device=dev) if kw.get("aux") else None
            k2 = dict(kw)
            if aux is not None:
                k2["aux"] = aux
            X = Ap if planes else A
            _with_bplanes(planes, lambda: K.gemm(M, N, Kk, X, B, C, mode_a=K.KC, lda=Ap.ld if planes else Kk,
                                                 mode_b=mb, ldb=B.stride(0), ldc=N, b_weight=True, **k2))
            outs.append((C, aux))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]), (kw.keys(), (outs[0][0] - outs[1][0]).abs().max().item())
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape", [(256, 512, 192), (768, 256, 2000), (1024, 264, 47872 // 8)])
def test_gemm_weight_gradient_planes(dev, shape):
    """Weight gradient dW += dy^T x with x as Planes (RC x RC: B planes, A split) and the fused bias
    gradient: equal to the fp32-x launch (bit for bit without split-K, else within 2e-7 of |dy||x|)."""
    N, Kd, M = shape  # dW (N, Kd), rows M
    dy = _r(M, N, seed=71).to(dev)
    x = _r(M, Kd, seed=72).to(dev)
    xp = K.Planes.of(x)
    res = []
    for planes in (False, True):
        dW = torch.zeros(N, Kd, device=dev)
        db = torch.zeros(N, device=dev)
        _with_bplanes(planes, lambda: K.linear_bwd_weight(dy, xp if planes else x, dW, db))
        res.append((dW.cpu().double(), db.cpu().double()))
    torch.cuda.synchronize()
    den = dy.abs().t().cpu().double() @ x.abs().cpu().double()
    if M < 256:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert ((res[0][0] - res[1][0]).abs() / den).max().item() <= 2e-7
    assert (res[0][1] - res[1][1]).abs().max().item() <= 1e-5 * math.sqrt(M)


@pytest.mark.parametrize("MD", [(777, 256), (64, 512), (5, 80)])
def test_layernorm_planes(dev, MD):
    """esp_layernorm_fwd_planes: the planes hold y exactly (hi + mid + lo, hi = bf16(y)), y / mean /
    rstd equal the fp32 LayerNorm kernel's within fp32 rounding (the row sums run in another lane
    order), and the bf16 form (n = 1) is bf16(y)."""
    M, D = MD
    x = (_r(M, D, seed=81) * 3 + 1).to(dev)
    w, b = _r(D, seed=82).to(dev), _r(D, seed=83).to(dev)
    y = torch.empty(M, D, device=dev)
    m0, r0 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    K.layernorm_fwd(x, w, b, y, m0, r0)
    yp = K.Planes(M, D, dev, 3)
    m1, r1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    K.layernorm_fwd_planes(x, w, b, yp, m1, r1)
    y1 = K.Planes(M, D, dev, 1)
    K.layernorm_fwd_planes(x, w, b, y1, torch.empty(M, device=dev), torch.empty(M, device=dev))
    torch.cuda.synchronize()
    yf = yp.float()
    assert (yf - y).abs().max().item() <= 4e-6 * max(1.0, y.abs().max().item())
    assert torch.allclose(m1, m0, rtol=1e-6, atol=1e-6) and torch.allclose(r1, r0, rtol=1e-6, atol=0)
    hi = yp.buf.view(3, M, yp.ld)[0, :, :D]
    assert torch.equal(hi, yf.to(torch.bfloat16))
    assert torch.equal(y1.buf.view(M, y1.ld)[:, :D], yf.to(torch.bfloat16))


def test_layernorm_dual_and_weight_gradient_on_twin_planes(dev):
    """esp_layernorm_fwd_dual (round 5): its fp32 y equals the planes' value exactly (hi + mid + lo == y,
    the same kernel writes both), y / mean / rstd equal esp_layernorm_fwd_planes' bit for bit; and the
    weight gradient that takes y's attached planes as B (PREC 3: only dy split in the k-loop) equals the
    one that splits fp32 y in registers, bit for bit (same split, same products, same order), fused bias
    gradient included, at an RC x RC shape with split-K (K = 12000 rows)."""
    M, D, N = 12000, 256, 768
    x = (_r(M, D, seed=84) * 3 + 1).to(dev)
    w, b = _r(D, seed=85).to(dev), _r(D, seed=86).to(dev)
    yp = K.Planes(M, D, dev, 3)
    m0, r0 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    K.layernorm_fwd_planes(x, w, b, yp, m0, r0)
    y = torch.empty(M, D, device=dev)
    m1, r1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    K.layernorm_fwd_dual(x, w, b, y, m1, r1)
    tw = K.twin_planes(y)
    assert tw is not None and tw.n == 3
    assert torch.equal(tw.float(), y) and torch.equal(tw.buf, yp.buf)
    assert torch.equal(m1, m0) and torch.equal(r1, r0)
    dy = _r(M, N, seed=87).to(dev)
    res = []
    for twin in (False, True):
        yy = y if twin else y.clone()  # (a clone carries no planes)
        assert (K.twin_planes(yy) is not None) == twin
        dW = torch.zeros(N, D, device=dev)
        db = torch.zeros(N, device=dev)
        K.linear_bwd_weight(dy, yy, dW, db)
        res.append((dW, db))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ref = dy.double().t() @ y.double()
    assert (res[1][0].double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_softmax_bwd_relpos_band_matches_full_rows(dev):
    """esp_attn_softmax_bwd_relpos_band (round 5): into a kept buffer that is zero outside the rel_shift
    band, two successive launches on different inputs give dS and the whole dbd (band AND the zeros) of the
    full-row kernel, bit for bit -- the band kernel never writes outside the band and overwrites all of it.
    Dropout on, T' = 374 (pitch 376 / 748), latest rel_shift."""
    Z, T, pa, seed = 24, 374, 0.1, 99
    Tp, Pp = K.pitch(T), K.pitch(2 * T - 1)
    K.release_relpos_band_buffers()  # (earlier tests in this process may hold the shape slots)
    band = K.relpos_band_buffer(Z, T, Pp, dev)
    assert band is not None and band.abs().max().item() == 0.0
    for rep in range(2):
        attn = torch.softmax(_r(Z * T, Tp, seed=100 + rep), dim=1).to(dev).reshape(-1)
        dP = _r(Z * T * Tp, seed=110 + rep).to(dev)
        dS0, dS1 = torch.empty_like(dP), torch.empty_like(dP)
        full = torch.full((Z * T * Pp,), float("nan"), device=dev)
        K.attn_softmax_bwd_relpos(attn, dP, dS0, full, Pp, pa, seed, 8.0, Z * T, T, Tp, relpos=1)
        K.attn_softmax_bwd_relpos_band(attn, dP, dS1, band, Pp, pa, seed, 8.0, Z * T, T, Tp)
        torch.cuda.synchronize()
        cols = slice(0, 2 * T - 1)
        assert torch.equal(dS0.view(Z * T, Tp)[:, :T], dS1.view(Z * T, Tp)[:, :T])
        assert torch.equal(full.view(Z * T, Pp)[:, cols], band.view(Z * T, Pp)[:, cols])


@pytest.mark.parametrize("B,T", [(48, 374), (1, 384), (1, 320), (5, 320), (4, 512), (2, 130)])
def test_relpos_dqv_band_matches_dense_gemm(dev, B, T):
    """esp_relpos_dqv (round 5): each 128-row tile's k-loop over its rows' rel_shift band only equals the
    dense dbd.p GEMM over all 2T-1 columns bit for bit (the skipped slabs hold zeros; the kept slabs are the
    dense GEMM's, same order), and the fp64 product.  B=48, H=4 (576 tiles: no split-K), T' = 374; the small
    batches run split-K (Z * ceil(T/128) < 512), where a split's chunk can lie wholly outside a tile's band:
    T' % 32 == 0 makes the band's first column non-zero, which such a split must not add a second time
    (round-6 fix of tile_coord).  Under split-K the dense GEMM splits K differently, so the two agree to
    rounding there and both are gated against fp64."""
    H, dk = 4, 64
    Z, D, P = B * H, H * dk, 2 * T - 1
    Pp = K.pitch(P)
    g = torch.Generator().manual_seed(5)
    dbd = torch.zeros(Z * T, Pp)
    vals = torch.randn(Z * T, T, generator=g)
    i = torch.arange(T).repeat(Z)
    cols = (T - 1 - i)[:, None] + torch.arange(T)[None, :]
    dbd.scatter_(1, cols, vals)
    p = torch.randn(P, D, generator=g) * 0.1
    dbd, p = dbd.to(dev).reshape(-1), p.to(dev)
    out0 = torch.empty(B * T, D, device=dev)
    out1 = torch.empty(B * T, D, device=dev)
    K.gemm(T, dk, P, dbd, p, out0, mode_a=K.KC, lda=Pp, mode_b=K.RC, ldb=D, ldc=D,
           batch=Z, nb2=B, sa=(B * T * Pp, T * Pp), sb=(dk, 0), sc=(dk, T * D))
    K.relpos_dqv(dbd, Pp, p, D, out1, D, B, H, T)
    torch.cuda.synchronize()
    if B * H * ((T + 127) // 128) >= 512:
        assert torch.equal(out0, out1)
    d = dbd.view(H, B, T, Pp)[..., :P].double().cpu()
    ref = torch.einsum("hbik,khd->bihd", d, p.double().cpu().view(P, H, dk)).reshape(B * T, D)
    for o in (out0, out1):
        assert (o.double().cpu() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_gemm_planes_output_epilogues(dev):
    """C written as planes (esp_gemm_f32_pl c_nplanes = 3): the FFN w_1 epilogue (bias + Swish / ReLU
    + dropout, derivative to aux) with A and B as planes, and the batched attention context P.V
    (fp32 operands, strided output): the planes hold exactly the fp32 epilogue's values (hi + mid + lo
    == the fp32 C of the same launch) and aux is unchanged."""
    M, N, Kk = 1000, 1024, 192  # K < 256: no split-K for the fp32-C launch either (a planes C never splits)
    A = _r(M, Kk, seed=91).to(dev)
    W = _r(N, Kk, seed=92, scale=0.1).to(dev)
    bias = _r(N, seed=93).to(dev)
    Ap = K.Planes.of(A)
    for act, p in ((K.ACT_SWISH, 0.1), (K.ACT_RELU, 0.1), (K.ACT_SWISH, 0.0)):
        outs = []
        for pl in (False, True):
            C = K.Planes(M, N, dev) if pl else torch.empty(M, N, device=dev)
            aux = torch.empty(M, N, device=dev)
            K.gemm(M, N, Kk, Ap, W, C, mode_a=K.KC, lda=Ap.ld, mode_b=K.KC, ldb=Kk, ldc=N, bias=bias,
                   act=act | K.ACT_AUX_DERIV, aux=aux, drop_p=p, seed=5, b_weight=True)
            outs.append((C.float() if pl else C, aux))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), act
    # P.V: z = 6 (head, utterance) pairs of T = 77 rows, d_k = 64, context rows strided into [B*T, D]
    Bn, H, T, dk = 2, 3, 77, 64
    D, Tp = H * dk, 80
    P = _r(H * Bn * T * Tp, seed=94).to(dev)
    V = _r(Bn * T, 3 * D, seed=95).to(dev)
    outs = []
    for pl in (False, True):
        C = K.Planes(Bn * T, D, dev) if pl else torch.empty(Bn * T, D, device=dev)
        K.gemm(T, dk, T, P, V, C, mode_a=K.KC, lda=Tp, mode_b=K.RC, ldb=3 * D, ldc=D, b_off=2 * D, batch=H * Bn,
               nb2=Bn, sa=(Bn * T * Tp, T * Tp), sb=(dk, T * 3 * D), sc=(dk, T * D))
        outs.append(C.float() if pl else C)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_bn_swish_planes(dev):
    """esp_bn_swish_fwd_planes: the same statistics (mean, rstd, running averages) as the fp32 kernel and
    planes holding exactly its s values (hi + mid + lo == s)."""
    M, D = 3000, 256
    y = _r(M, D, seed=101).to(dev)
    g, b = _r(D, seed=102).to(dev), _r(D, seed=103).to(dev)
    outs = []
    for pl in (False, True):
        s = K.Planes(M, D, dev) if pl else torch.empty(M, D, device=dev)
        mean, rstd = torch.empty(D, device=dev), torch.empty(D, device=dev)
        rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
        K.bn_swish_fwd(y, g, b, s, mean, rstd, rm, rv)
        outs.append((s.float() if pl else s, mean, rstd, rm, rv))
    torch.cuda.synchronize()
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(a, c)


def test_scale_dropout_planes_same_masks(dev):
    """esp_scale_dropout_planes: the planes hold exactly esp_scale_dropout's values (same masks)."""
    M, D = 1000, 256
    x = _r(M, D, seed=111).to(dev)
    y = torch.empty(M, D, device=dev)
    K.scale_dropout(x, y, alpha=0.5, drop_p=0.1, seed=77)
    yp = K.Planes(M, D, dev)
    K.scale_dropout(x, yp, alpha=0.5, drop_p=0.1, seed=77)
    torch.cuda.synchronize()
    assert torch.equal(yp.float(), y)


def test_ffn_backward_planes_matches_fp32(dev):
    """The FFN backward with its branch gradients as planes (dz from the dropout backward, dh from the
    derivative-multiply epilogue) gives the fp32 path's input and parameter gradients to a few ulps
    (1e-6 relative: the planes launches reduce split-K partials in another order)."""
    from espnet_slurp_amd.blocks import PositionwiseFeedForward, Seeds
    from espnet_slurp_amd.flat import FlatParams
    torch.manual_seed(3)
    res = []
    for xplanes in (False, True):
        prev = K._XPLANES
        K._XPLANES = xplanes
        try:
            ff = PositionwiseFeedForward(256, 1024, 0.1, K.ACT_SWISH).to(dev)
            torch.manual_seed(3)
            for p in ff.parameters():
                with torch.no_grad():
                    p.copy_(torch.randn_like(p) * 0.05)
            flat = FlatParams(ff, dev)
            x = _r(2000, 256, seed=121).to(dev)
            dout = _r(2000, 256, seed=122).to(dev)
            with K.param_cast_scope():
                xin = K.Planes.of(x) if xplanes else x
                out, c = ff.fwd(xin, x, 0.5, 0.1, Seeds(5), True)
                dx = ff.bwd(c, dout)
            torch.cuda.synchronize()
            res.append((out.clone(), dx.clone(), flat.grad.clone()))
        finally:
            K._XPLANES = prev
    for a, b in zip(res[0], res[1]):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item()), (a - b).abs().max().item()
