"""esp_relpos_attn_probs in the window the block-staged kernel does not take (384 < T' <= 512): the per-wave
kernel relpos_attn_fwd16_kernel, every instantiation the default build still launches.

T' = 385 (25 key tiles, N = 28: the first T' past the LDS kernel), 449 (29 tiles, N = 32) and 512 (32 tiles,
N = 32, a full last tile), latest and legacy rel_shift.  The fp32 mode takes the <28 / 32, *, *> forms; the bf16
mode the <32, *, false, 1, 1> form (latest) and the two-waves-per-row-group form <16, *, true, 2, 1> (legacy,
the launcher recomputes its row-block count)."""
import functools
import math

import pytest
import torch

from oracle import espnet_cpu as O

pytestmark = pytest.mark.gpu

B, H, DK = 2, 4, 64
D, Z = H * DK, H * B
DROP_P, SEED = 0.1, 1234
# the kernels' inverted-dropout rescale: p on the 1/65536 grid (csrc/common.h, drop_threshold / drop_scale)
DROP_SCALE = 65536.0 / (65536.0 - int(DROP_P * 65536.0 + 0.5))

# bf16 mode against the fp64 softmax of bf16-rounded operands: 4x the largest error measured on the build
# before the launcher / path-table refactor -- 4.202e-9 (T' = 385 latest; 1.6e-9 .. 4.2e-9 over the six cases,
# the probabilities themselves are ~1/T').  The margin covers the fp32 accumulation order.
BF16_BOUND = 4 * 4.202e-9


@functools.lru_cache(maxsize=None)
def _inputs(T, legacy):
    P = T if legacy else 2 * T - 1
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * D, generator=g) * 0.5
    p = torch.randn(P, D, generator=g) * 0.5
    q_u = torch.randn(Z * T * DK, generator=g) * 0.5
    q_v = torch.randn(Z * T * DK, generator=g) * 0.5
    klen = torch.tensor([T, T - 7], dtype=torch.int32)
    return qkv, p, q_u, q_v, klen


@functools.lru_cache(maxsize=None)
def _ref_unfused(T, legacy):
    """The unfused fp32 path at the same seed: ac GEMM, bd GEMM, rel_shift + softmax pass -> (attn, pdrop)."""
    from espnet_slurp_amd import kernels as K
    dev = torch.device("cuda:0")
    qkv, p, q_u, q_v, klen = (t.to(dev) for t in _inputs(T, legacy))
    P = p.shape[0]
    Tp, Pp = K.pitch(T), K.pitch(P)
    ac = torch.empty(Z * T * Tp, device=dev)
    bd = torch.empty(Z * T * Pp, device=dev)
    pdrop = torch.empty(Z * T * Tp, device=dev)
    with K.gemm_compute("fp32"):
        K.gemm(T, T, DK, q_u, qkv, ac, mode_a=K.KC, lda=DK, mode_b=K.KC, ldb=3 * D, ldc=Tp, b_off=D,
               batch=Z, nb2=B, sa=(B * T * DK, T * DK), sb=(DK, T * 3 * D), sc=(B * T * Tp, T * Tp))
        K.gemm(T, P, DK, q_v, p, bd, mode_a=K.KC, lda=DK, mode_b=K.KC, ldb=D, ldc=Pp,
               batch=Z, nb2=B, sa=(B * T * DK, T * DK), sb=(DK, 0), sc=(B * T * Pp, T * Pp))
        K.attn_softmax_fwd(ac, bd, 2 if legacy else 1, P, math.sqrt(DK), klen, B, False, ac, pdrop, DROP_P, SEED, Z,
                           T, T, lds=Tp, ldp=Pp)
    torch.cuda.synchronize()
    return ac.view(Z, T, Tp)[:, :, :T].cpu(), pdrop.view(Z, T, Tp)[:, :, :T].cpu()


@functools.lru_cache(maxsize=None)
def _ref_bf16(T, legacy):
    """softmax((q_u k^T + rel_shift(q_v p^T)) / sqrt(d_k)) in fp64 from bf16-rounded operands, key mask applied."""
    qkv, p, q_u, q_v, klen = _inputs(T, legacy)
    r = lambda t: t.bfloat16().double()  # noqa: E731
    qu = r(q_u).view(H, B, T, DK)
    qv = r(q_v).view(H, B, T, DK)
    k = r(qkv[:, D:2 * D]).view(B, T, H, DK).permute(2, 0, 1, 3)
    ph = r(p).view(-1, H, DK).permute(1, 0, 2)
    ac = torch.einsum("hbid,hbjd->hbij", qu, k)
    bd = torch.einsum("hbid,hpd->hbip", qv, ph)
    bd = O.rel_shift_legacy(bd) if legacy else O.rel_shift_latest(bd)
    masked = torch.arange(T)[None, None, None, :] >= klen[None, :, None, None]
    s = ((ac + bd) / math.sqrt(DK)).masked_fill(masked, float("-inf"))
    return torch.softmax(s, -1).masked_fill(masked, 0.0).reshape(Z, T, T)


@pytest.mark.parametrize("T", [385, 449, 512])
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_relpos_probs_wave_window(dev, T, legacy, mode):
    from espnet_slurp_amd import kernels as K
    qkv, p, q_u, q_v, klen = (t.to(dev) for t in _inputs(T, legacy))
    Tp = K.pitch(T)
    ac = torch.empty(Z * T * Tp, device=dev)
    pdrop = torch.empty(Z * T * Tp, device=dev)
    with K.gemm_compute(mode):
        K.relpos_attn_probs(q_u, q_v, qkv, 3 * D, p, D, 2 if legacy else 1, B, H, math.sqrt(DK), klen, ac, pdrop,
                            DROP_P, SEED, T, Tp, k_off=D)
    torch.cuda.synchronize()
    a = ac.view(Z, T, Tp)[:, :, :T].cpu()  # the pitch columns are not compared
    pd = pdrop.view(Z, T, Tp)[:, :, :T].cpu()
    assert torch.isfinite(a).all() and torch.isfinite(pd).all()
    rowsum = float((a.sum(-1) - 1).abs().max())  # every row has keys (klen >= T - 7)
    print(f"T={T} legacy={legacy} {mode} max |row sum - 1|: {rowsum:.3e}")
    assert rowsum < 1e-5
    for b in range(B):  # z = h * B + b
        n = int(klen[b])
        assert not a.view(H, B, T, T)[:, b, :, n:].any() and not pd.view(H, B, T, T)[:, b, :, n:].any()
    # the dropout copy is 0 or p * drop_scale (one fp32 product)
    scaled = a * torch.tensor(DROP_SCALE, dtype=torch.float32)
    assert torch.allclose(torch.where(pd != 0, pd, scaled), scaled, rtol=1e-6, atol=1e-12)
    kept = float((pd != 0).sum()) / float((a != 0).sum())
    assert abs(kept - (1 - DROP_P)) < 0.01, kept
    if mode == "fp32":
        ra, rpd = _ref_unfused(T, legacy)
        err = float((a - ra).abs().max())
        print(f"T={T} legacy={legacy} fp32 vs unfused: {err:.3e}")
        assert err < 1e-6
        assert bool(((pd == 0) == (rpd == 0)).all())
    else:
        err = float((a.double() - _ref_bf16(T, legacy)).abs().max())
        print(f"T={T} legacy={legacy} bf16 vs fp64 of bf16 operands: {err:.3e}")
        assert err < BF16_BOUND
