"""The latest rel-pos attention backward that reads dS directly (kernels.RELPOS_BWD_DS): the dS-only score
gradient (esp_attn_dscores / esp_attn_bwd_prep with dbd NULL), dq = dS k + Dbd p from the staged dS rows
(esp_relpos_dq), dp along dS's diagonals (esp_relpos_dp), and the block wiring -- against the row-wise adjoint
pass + dbd path it replaces, and against the fp64 oracle.  H = 4, D = 256 (d_k = 64)."""
import functools
import math

import pytest
import torch

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd.blocks import RelPositionMultiHeadedAttention, Seeds
from espnet_slurp_amd.asr.encoder.abs_encoder import pos_table
from espnet_slurp_amd.flat import FlatParams
from oracle import espnet_cpu as O
from tests.helpers import rel_err
from tests.test_gpu_blocks import _check_grads, _params64

pytestmark = pytest.mark.gpu

H, D, DK = 4, 256, 64


def _flags(monkeypatch, ds: bool):
    monkeypatch.setattr(K, "RELPOS_BWD_DS", ds)
    monkeypatch.setattr(K, "FUSED_ATTN_BWD", False)
    monkeypatch.setattr(K, "ATTN_DSCORES", False)
    monkeypatch.setattr(K, "FLASH_ATTN", False)
    monkeypatch.setattr(K, "ATTN_FWD32", False)


def _module(dev, p_drop, seed, std=0.1):
    torch.manual_seed(seed)
    mod = RelPositionMultiHeadedAttention(H, D, p_drop, False).to(dev)
    with torch.no_grad():
        for p in mod.parameters():
            p.normal_(0, std)
    mod.flat = FlatParams(mod, dev)
    return mod


@pytest.mark.parametrize("T,p_drop", [(29, 0.1), (77, 0.1), (130, 0.1), (374, 0.1), (77, 0.0)])
def test_ds_only_score_gradient_matches_rowpass(dev, monkeypatch, T, p_drop):
    """esp_attn_bwd_prep + esp_attn_dscores with dbd NULL write the dS of the dP GEMM + the row-wise softmax /
    dropout / rel_shift adjoint pass (same probabilities, same seed: the mask index is row * T + j in both).
    T' = 374: score pitch 376 and a ragged last quad."""
    _flags(monkeypatch, True)
    B = 2
    Z, M, Tp, Pp = H * B, B * T, K.pitch(T), K.pitch(2 * T - 1)
    mod = _module(dev, p_drop, 4)
    klen = torch.tensor([T, (T * 3) // 5]).int().to(dev)
    x = torch.randn(M, D, device=dev)
    res = torch.randn(M, D, device=dev)
    pos = pos_table("latest", T, D, dev)
    _, c = mod.fwd(x, res, pos, klen, B, T, 0.0, Seeds(7), True)
    assert c.bwd_ds and (c.pa > 0) == (p_drop > 0)
    dctx = torch.randn(M, D, device=dev)
    dS0 = torch.zeros(Z * T * Tp, device=dev)
    K.gemm(T, T, DK, dctx, c.qkv, dS0, mode_a=K.KC, lda=D, mode_b=K.KC, ldb=3 * D, ldc=Tp, b_off=2 * D,
           batch=Z, nb2=B, sa=(DK, T * D), sb=(DK, T * 3 * D), sc=(B * T * Tp, T * Tp))
    dbd = torch.zeros(Z * T * Pp, device=dev)
    K.attn_softmax_bwd_relpos(c.attn, dS0, dS0, dbd, Pp, c.pa, c.sa, math.sqrt(DK), Z * T, T, Tp, relpos=1)
    dot = torch.empty(Z * T, device=dev)
    dS1 = torch.zeros(Z * T * Tp, device=dev)
    K.attn_bwd_prep(dctx, D, c.ctx, D, B, H, DK, T, dot, None, 0, 1)
    K.attn_dscores(dctx, D, c.qkv, 3 * D, c.attn, dot, dS1, None, 0, 1, B, H, DK, math.sqrt(DK), c.pa, c.sa, T, Tp,
                   v_off=2 * D)
    torch.cuda.synchronize()
    a, b = dS1.view(-1, Tp)[:, :T].cpu(), dS0.view(-1, Tp)[:, :T].cpu()
    e = rel_err(a, b)
    print(f"T={T} p={p_drop}: dS rel err {e:.3g}")
    assert float(b.abs().max()) > 0 and e < 1e-5


@functools.lru_cache(maxsize=None)
def _dense_case(T, B):
    """Dense random dS (pitch columns random too: they must not be read), k, p, q_v; the dbd-based references
    (dq_u GEMM, esp_relshift_bwd + the dense dbd.p GEMM, esp_colsum, the dbd^T q_v GEMM) and the dS-only
    kernels' results, computed once per shape."""
    dev = torch.device("cuda:0")
    Z, M, P = H * B, B * T, 2 * T - 1
    Tp, Pp = K.pitch(T), K.pitch(P)
    g = torch.Generator().manual_seed(100 * T + B)
    dS = torch.randn(Z * T * Tp, generator=g).to(dev)
    qkv = (torch.randn(M, 3 * D, generator=g) * 0.5).to(dev)
    p = (torch.randn(P, D, generator=g) * 0.5).to(dev)
    q_v = (torch.randn(Z * T * DK, generator=g) * 0.5).to(dev)
    # references through dbd
    dq0 = torch.zeros(M, 3 * D, device=dev)
    K.gemm(T, DK, T, dS, qkv, dq0, mode_a=K.KC, lda=Tp, mode_b=K.RC, ldb=3 * D, ldc=3 * D, b_off=D,
           batch=Z, nb2=B, sa=(B * T * Tp, T * Tp), sb=(DK, T * 3 * D), sc=(DK, T * 3 * D))
    dbd = torch.zeros(Z * T * Pp, device=dev)
    K.relshift_bwd(dS, dbd, 1, Z, T, P, lds=Tp, ldp=Pp)
    tmp = torch.empty(M, D, device=dev)
    K.gemm(T, DK, P, dbd, p, tmp, mode_a=K.KC, lda=Pp, mode_b=K.RC, ldb=D, ldc=D,
           batch=Z, nb2=B, sa=(B * T * Pp, T * Pp), sb=(DK, 0), sc=(DK, T * D))
    du0 = torch.zeros(D, device=dev)
    dv0 = torch.zeros(D, device=dev)
    K.colsum(dq0, du0, accumulate=True, M=M, N=D, ld=3 * D)
    K.colsum(tmp, dv0, accumulate=True)
    dp0 = torch.empty(P, D, device=dev)
    K.gemm(P, DK, B * T, dbd, q_v, dp0, mode_a=K.RC, lda=Pp, mode_b=K.RC, ldb=DK, ldc=D,
           batch=H, nb2=1, sa=(B * T * Pp, 0), sb=(B * T * DK, 0), sc=(DK, 0))
    # the dS-only kernels
    dq1 = torch.zeros(M, 3 * D, device=dev)
    bias_part = torch.empty(Z * ((T + 31) // 32) * 2 * DK, device=dev)
    K.relpos_dq(dS, Tp, qkv, 3 * D, p, D, dq1, 3 * D, bias_part, B, H, T, k_off=D)
    du1 = torch.zeros(D, device=dev)
    dv1 = torch.zeros(D, device=dev)
    dp1 = torch.empty(P, D, device=dev)
    K.relpos_dp(dS, Tp, q_v, 1, B, H, T, dp1, D, bias_part, None, du1, dv1, dq1, 3 * D)
    torch.cuda.synchronize()
    return dict(dq0=(dq0[:, :D] + tmp).cpu(), dq1=dq1[:, :D].cpu(), rest1=dq1[:, D:].cpu(), du0=du0.cpu(),
                du1=du1.cpu(), dv0=dv0.cpu(), dv1=dv1.cpu(), dp0=dp0.cpu(), dp1=dp1.cpu())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [29, 77, 130, 374])
def test_relpos_dq_dense_ds(dev, T, B):
    """esp_relpos_dq on dense random dS (no masked zeros that would hide a read outside a row's band) equals
    dq_u from the GEMM + dq_v from esp_relshift_bwd and the dense dbd.p GEMM, and its two column sums equal
    esp_colsum's.  T' = 29: one partial tile; 77: odd, pitch 80; 130: 2 rows past a 128-row boundary; 374."""
    r = _dense_case(T, B)
    errs = {n: rel_err(r[n + "1"], r[n + "0"]) for n in ("dq", "du", "dv")}
    print(f"T={T} B={B}: {errs}")
    assert float(r["rest1"].abs().max()) == 0.0  # only columns 0..D of dqkv are written
    assert all(e < 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("T", [29, 77, 130])
def test_relpos_dp_from_ds_dense(dev, T, B):
    """dp along dS's diagonals (esp_relpos_dp, empty (position tile, rho chunk) pairs skipped) equals the
    dbd^T q_v GEMM on the same dense dS; B = 5 is a partial batch group of the fixed-order partials."""
    r = _dense_case(T, B)
    e = rel_err(r["dp1"], r["dp0"])
    print(f"T={T} B={B}: dp rel err {e:.3g}")
    assert e < 1e-5


@pytest.mark.parametrize("T,klens", [(29, [29, 23, 15]), (77, [77, 40, 9]), (130, [130, 129, 64])])
def test_block_ds_backward_matches_oracle(dev, monkeypatch, T, klens):
    """RelPositionMultiHeadedAttention forward + backward on the dS-only path against the fp64 oracle."""
    _flags(monkeypatch, True)
    B = 3
    klen = torch.tensor(klens)
    mod = _module(dev, 0.0, 3)
    x = torch.randn(B * T, D)
    res = torch.randn(B * T, D)
    dout = torch.randn(B * T, D)
    pos = pos_table("latest", T, D, dev)
    out, c = mod.fwd(x.to(dev), res.to(dev), pos, klen.int().to(dev), B, T, 0.0, Seeds(1), True)
    assert c.bwd_ds
    dx = mod.bwd(c, dout.to(dev))
    P = _params64(mod, "a")
    xt = x.double().view(B, T, D).requires_grad_(True)
    mask = (~O.make_pad_mask(klen, T))[:, None, :]
    ref = O.rel_mha(P, "a", xt, pos.cpu().double()[None], mask, H, False) + res.double().view(B, T, D)
    ref.backward(dout.double().view(B, T, D))
    assert rel_err(out.cpu(), ref.detach().reshape(B * T, D)) < 1e-5
    assert rel_err(dx.cpu(), xt.grad.reshape(B * T, D)) < 1e-5
    _check_grads(mod, P, "a")


@pytest.mark.parametrize("T", [100, 374])
def test_block_ds_backward_matches_rowpass_with_dropout(dev, monkeypatch, T):
    """Same Seeds, attention dropout 0.1: the dS-only backward gives the row-pass path's dx and gradients."""
    B = 2
    klen = torch.tensor([T, (T * 3) // 5]).int().to(dev)
    mod = _module(dev, 0.1, 4, std=0.05)
    x = torch.randn(B * T, D, device=dev)
    res = torch.randn(B * T, D, device=dev)
    pos = pos_table("latest", T, D, dev)
    dout = torch.randn(B * T, D, device=dev)
    got = []
    for ds in (True, False):
        _flags(monkeypatch, ds)
        mod.flat.grad.zero_()
        out, c = mod.fwd(x, res, pos, klen, B, T, 0.0, Seeds(7), True)
        assert c.bwd_ds == ds and c.pa > 0
        dx = mod.bwd(c, dout)
        got.append((out.cpu(), dx.cpu(), mod.flat.grad.cpu().clone()))
    K.release_relpos_band_buffers()
    assert torch.equal(got[0][0], got[1][0])
    e_dx, e_g = rel_err(got[0][1], got[1][1]), rel_err(got[0][2], got[1][2])
    print(f"T={T}: dx {e_dx:.3g} flat.grad {e_g:.3g}")
    assert e_dx < 1e-5 and e_g < 1e-5


def test_ds_backward_deterministic_and_graph_safe(dev, monkeypatch):
    """T' = 77, B = 3: two eager backwards give bitwise equal gradients, and the backward captured once on one
    stream and replayed twice gives the eager bits (no allocation or host sync in the native calls, fixed-order
    reductions)."""
    _flags(monkeypatch, True)
    B, T = 3, 77
    klen = torch.tensor([77, 40, 9]).int().to(dev)
    mod = _module(dev, 0.1, 5)
    x = torch.randn(B * T, D, device=dev)
    res = torch.randn(B * T, D, device=dev)
    pos = pos_table("latest", T, D, dev)
    dout = torch.randn(B * T, D, device=dev)
    _, c = mod.fwd(x, res, pos, klen, B, T, 0.0, Seeds(9), True)
    assert c.bwd_ds
    eager = []
    for _ in range(2):
        mod.flat.grad.zero_()
        dx = mod.bwd(c, dout)
        eager.append((dx.clone(), mod.flat.grad.clone()))
    assert torch.equal(eager[0][0], eager[1][0]) and torch.equal(eager[0][1], eager[1][1])
    assert float(eager[0][1].abs().max()) > 0
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up on a side stream, as the Trainer's capture does
        mod.bwd(c, dout)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dx_g = mod.bwd(c, dout)
    for _ in range(2):
        mod.flat.grad.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(dx_g, eager[0][0]) and torch.equal(mod.flat.grad, eager[0][1])
