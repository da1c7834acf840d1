"""esp_causal_attn_fwd / _bwd (csrc/causal_attn.hip) on the MI355X against an fp64 torch restatement of the masked
attention written here (key j visible to query i iff j <= i and j < klen[b]; query rows at or beyond klen[b] output
zeros).  Gate, as in test_gpu_cbt_kernels.py: at most twice the error of the same restatement run in fp32 on the CPU,
and never tighter than 1e-5 absolute; both errors are printed.  Outputs are prefilled with NaN, so an element the
kernels do not write fails."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, L, H, dk), klen: one token; several blocks' worth of ragged rows inside one 16-row tile; L no multiple of 16 and
# the 68 KiB backward (dk 64, L > 48); a full 64 x 64 tile beside a one-token row; three tiles with the diagonal
# inside a tile; dk = 128 at its Lmax (132 KiB of LDS in the backward)
CASES = [((3, 1, 1, 16), [1, 1, 1]),
         ((5, 10, 2, 16), [10, 7, 1, 3, 10]),
         ((2, 33, 2, 64), [33, 20]),
         ((2, 64, 1, 64), [64, 1]),
         ((2, 17, 4, 32), [17, 16]),
         ((2, 64, 2, 128), [64, 5])]


def _visible(klen, L):
    i = torch.arange(L)
    return (i[None, :] <= i[:, None])[None] & (i[None, None, :] < klen[:, None, None])  # (B, L, L)


def _heads(qkv, H, dk):
    B, L, _ = qkv.shape
    D = H * dk
    return (qkv[..., n * D:(n + 1) * D].reshape(B, L, H, dk).transpose(1, 2) for n in range(3))


def _attn(qkv, klen, H, dk):
    """qkv (B, L, 3*H*dk) -> ctx (B, L, H*dk) in qkv's dtype."""
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, dk)
    s = q @ k.transpose(-1, -2) / math.sqrt(dk)
    p = torch.softmax(s.masked_fill(~_visible(klen, L)[:, None], float("-inf")), dim=-1)
    live = (torch.arange(L)[None, :] < klen[:, None]).to(qkv.dtype)  # (B, L)
    return (p @ v).transpose(1, 2).reshape(B, L, H * dk) * live[..., None]


def _ref(qkv, cot, klen, H, dk, dtype):
    x = qkv.to(dtype).clone().requires_grad_(True)
    out = _attn(x, klen, H, dk)
    out.backward(cot.to(dtype))
    return out.detach(), x.grad


def _run(dev, qkv, cot, klen, H, dk):
    from espnet_slurp_amd import kernels as K
    B, L, _ = qkv.shape
    D = H * dk
    q = qkv.to(dev).contiguous().view(B * L, 3 * D)
    kl = klen.to(torch.int32).to(dev)
    ctx = torch.full((B * L, D), float("nan"), device=dev)
    lse = torch.full((B * H * L,), float("nan"), device=dev)
    K.causal_attn_fwd(q, kl, ctx, lse, B, L, H, dk)
    dqkv = torch.full((B * L, 3 * D), float("nan"), device=dev)
    K.causal_attn_bwd(q, kl, cot.to(dev).contiguous().view(B * L, D), lse, dqkv, B, L, H, dk)
    torch.cuda.synchronize()
    return ctx.cpu().view(B, L, D), dqkv.cpu().view(B, L, 3 * D), lse.cpu().view(B, H, L)


def _gate(what, got, ref32, want64):
    e_got = float((got.double() - want64).abs().max())
    e_ref = float((ref32.double() - want64).abs().max())
    gate = max(2 * e_ref, 1e-5)
    print(f"{what}: ours {e_got:.3e}, restatement fp32 {e_ref:.3e}, gate {gate:.3e}")
    assert e_got <= gate, (what, e_got, gate)


def _inputs(shape, seed):
    B, L, H, dk = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, 3 * H * dk, generator=g), torch.randn(B, L, H * dk, generator=g)


@pytest.mark.parametrize("shape,klen", CASES)
def test_causal_attn_vs_fp64(dev, shape, klen):
    from espnet_slurp_amd import kernels as K
    B, L, H, dk = shape
    assert K.causal_attn_ok(L, dk)
    D = H * dk
    klen = torch.tensor(klen)
    qkv, cot = _inputs(shape, 300 + L + dk)
    ctx, dqkv, lse = _run(dev, qkv, cot, klen, H, dk)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(lse).all())
    o64, g64 = _ref(qkv, cot, klen, H, dk, torch.float64)
    o32, g32 = _ref(qkv, cot, klen, H, dk, torch.float32)
    tag = f"causal_attn {shape}"
    _gate(tag + " ctx", ctx, o32, o64)
    for n, name in enumerate(("dq", "dk", "dv")):
        sl = slice(n * D, (n + 1) * D)
        _gate(f"{tag} {name}", dqkv[..., sl], g32[..., sl], g64[..., sl])
    # the saved statistic is the row log-sum-exp of the visible keys
    q, k, _ = _heads(qkv.double(), H, dk)
    s = (q @ k.transpose(-1, -2) / math.sqrt(dk)).masked_fill(~_visible(klen, L)[:, None], float("-inf"))
    want = torch.logsumexp(s, dim=-1)  # (B, H, L)
    for b in range(B):
        n = int(klen[b])
        assert float((lse[b, :, :n].double() - want[b, :, :n]).abs().max()) <= 1e-5
        # padding: exact zeros at the query rows and at the key / value rows beyond the length
        assert float(ctx[b, n:].abs().sum()) == 0.0 and float(lse[b, :, n:].abs().sum()) == 0.0
        assert float(dqkv[b, n:].abs().sum()) == 0.0
    # a second run repeats bit for bit
    ctx2, dqkv2, lse2 = _run(dev, qkv, cot, klen, H, dk)
    assert torch.equal(ctx, ctx2) and torch.equal(dqkv, dqkv2) and torch.equal(lse, lse2)


def test_causal_attn_rejects_unsupported_shapes(dev):
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd._native import NativeError
    kl = torch.ones(1, dtype=torch.int32, device=dev)
    for L, dk in ((65, 64), (10, 48), (0, 16)):
        assert not K.causal_attn_ok(L, dk)
        n = max(L, 1)  # (L = 0 is refused on its shape, not for an empty buffer)
        qkv, dqkv = torch.zeros(n, 3 * dk, device=dev), torch.zeros(n, 3 * dk, device=dev)
        ctx, lse = torch.zeros(n, dk, device=dev), torch.zeros(n, device=dev)
        with pytest.raises(NativeError):
            K._native.call("esp_causal_attn_fwd", qkv.data_ptr(), kl.data_ptr(), ctx.data_ptr(), lse.data_ptr(), 1, L,
                           1, dk, None)
        with pytest.raises(NativeError):
            K._native.call("esp_causal_attn_bwd", qkv.data_ptr(), kl.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                           dqkv.data_ptr(), 1, L, 1, dk, None)
    with pytest.raises(NativeError):  # through the wrapper as well
        K.causal_attn_fwd(torch.zeros(65, 192, device=dev), kl, torch.zeros(65, 64, device=dev),
                          torch.zeros(65, device=dev), 1, 65, 1, 64)
    assert K.causal_attn_ok(64, 64) and K.causal_attn_ok(1, 16) and K.causal_attn_ok(32, 128)
