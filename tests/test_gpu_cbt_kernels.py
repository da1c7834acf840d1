"""Kernels of the contextual block Transformer encoder (csrc/cbt.hip) on the MI355X.

Fused block attention against an fp64 torch restatement of the masked attention written here (key j valid iff
j <= S - 2, query row 0 outputs zeros).  Gate, as in test_gpu_lm.py: at most twice the error of the same restatement
run in fp32 on the CPU, and never tighter than 1e-5 absolute; both errors are printed.

chunk / ctx_shift / unchunk against the maps recorded from the reference (tests/golden/cbt_layout.json, the maps of
tests/test_cbt_cpu.py) and, backward, against torch autograd of an index_select / mean restatement: exact where every
sum is exact, else within 1 ulp per summand."""
import math

import numpy as np
import pytest
import torch

from tests import cbt_helpers as CH

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23  # 1 ulp of a float in [1, 2)


def _attn(qkv, S, H, dk, keep=None, dscale=1.0):
    """qkv (Z, S, 3*H*dk) -> ctx (Z, S, H*dk) in qkv's dtype; keep: (Z, H, S, S) 0 / 1 dropout mask."""
    Z = qkv.shape[0]
    D = H * dk
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(Z, S, H, dk).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(dk)
    dead = torch.zeros(S, S, dtype=torch.bool)
    dead[:, S - 1:] = True
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    if keep is not None:
        p = p * keep.to(p.dtype) * dscale
    rows = torch.ones(S, 1, dtype=qkv.dtype)
    rows[0] = 0
    return ((p @ v) * rows).transpose(1, 2).reshape(Z, S, D)


def _ref(qkv, cot, S, H, dk, dtype, keep=None, dscale=1.0):
    x = qkv.to(dtype).clone().requires_grad_(True)
    out = _attn(x, S, H, dk, keep, dscale)
    out.backward(cot.to(dtype))
    return out.detach(), x.grad


def _run(dev, qkv, cot, S, H, dk, p=0.0, seed=0):
    from espnet_slurp_amd import kernels as K
    Z = qkv.shape[0]
    D = H * dk
    q = qkv.to(dev).contiguous()
    ctx = torch.full((Z * S, D), float("nan"), device=dev)
    lse = torch.full((Z * H * S,), float("nan"), device=dev)
    K.block_attn_fwd(q.view(Z * S, 3 * D), ctx, lse, Z, S, H, dk, p, seed)
    dqkv = torch.full((Z * S, 3 * D), float("nan"), device=dev)
    K.block_attn_bwd(q.view(Z * S, 3 * D), cot.to(dev).contiguous().view(Z * S, D), lse, dqkv, Z, S, H, dk, p, seed)
    torch.cuda.synchronize()
    return ctx.cpu().view(Z, S, D), dqkv.cpu().view(Z, S, 3 * D), lse.cpu().view(Z, H, S)


def _gate(what, got, ref32, want64):
    e_got = float((got.double() - want64).abs().max())
    e_ref = float((ref32.double() - want64).abs().max())
    gate = max(2 * e_ref, 1e-5)
    print(f"{what}: ours {e_got:.3e}, restatement fp32 {e_ref:.3e}, gate {gate:.3e}")
    assert e_got <= gate, (what, e_got, gate)


def _gate_all(tag, ctx, dqkv, qkv, cot, S, H, dk, keep=None, dscale=1.0):
    D = H * dk
    o64, g64 = _ref(qkv, cot, S, H, dk, torch.float64, keep, dscale)
    o32, g32 = _ref(qkv, cot, S, H, dk, torch.float32, keep, dscale)
    _gate(tag + " ctx", ctx, o32, o64)
    for i, n in enumerate(("dq", "dk", "dv")):
        _gate(f"{tag} {n}", dqkv[..., i * D:(i + 1) * D], g32[..., i * D:(i + 1) * D], g64[..., i * D:(i + 1) * D])


def _inputs(S, dk, Z, H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Z, S, 3 * H * dk, generator=g), torch.randn(Z, S, H * dk, generator=g))


# (64, 64, 2, 1): the backward's LDS need above 64 KiB (not one of the three shapes the gate was set for, same gate)
@pytest.mark.parametrize("S,dk,Z,H", [(10, 16, 7, 2), (42, 64, 5, 2), (64, 32, 3, 1), (64, 64, 2, 1)])
def test_block_attn_vs_fp64(dev, S, dk, Z, H):
    qkv, cot = _inputs(S, dk, Z, H, 100 + S + dk)
    ctx, dqkv, lse = _run(dev, qkv, cot, S, H, dk)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dqkv).all())
    assert float(ctx[:, 0].abs().max()) == 0.0  # the dead query row
    assert float(dqkv[:, 0, :H * dk].abs().max()) == 0.0  # ... gets no gradient as a query
    assert float(dqkv[:, S - 1, H * dk:].abs().max()) == 0.0  # the last slot is no key and no value
    _gate_all(f"block_attn S={S} dk={dk}", ctx, dqkv, qkv, cot, S, H, dk)
    # the saved statistic is the row log-sum-exp of the valid keys
    D = H * dk
    q, k = (qkv[..., i * D:(i + 1) * D].double().reshape(Z, S, H, dk).transpose(1, 2) for i in range(2))
    want = torch.logsumexp((q @ k.transpose(-1, -2) / math.sqrt(dk))[..., :S - 1], dim=-1)
    assert float((lse[:, :, 1:].double() - want[:, :, 1:]).abs().max()) <= 1e-5


@pytest.mark.parametrize("S,dk,Z,H", [(10, 16, 7, 2), (42, 64, 5, 2)])
def test_block_attn_dropout(dev, S, dk, Z, H):
    p = 0.25
    D = H * dk
    qkv, cot = _inputs(S, dk, Z, H, 200 + S)
    # V = [I_S | 0]: ctx row i, head h holds the dropped probabilities of row i
    v = torch.zeros(Z, S, H, dk)
    v[:, :, :, :S] = torch.eye(S)[None, :, None, :]
    qkv[..., 2 * D:] = v.reshape(Z, S, D)
    ctx, dqkv, _ = _run(dev, qkv, cot, S, H, dk, p, seed=1234)
    ctx2, dqkv2, _ = _run(dev, qkv, cot, S, H, dk, p, seed=1234)
    assert torch.equal(ctx, ctx2) and torch.equal(dqkv, dqkv2)  # same seed: bit-equal
    ctx3, _, _ = _run(dev, qkv, cot, S, H, dk, p, seed=1235)
    assert not torch.equal(ctx, ctx3)
    pd = ctx.view(Z, S, H, dk)[..., :S].transpose(1, 2)  # (Z, H, S, S)
    keep = (pd != 0).float()
    assert float(keep[:, :, 0].sum()) == 0 and float(keep[..., S - 1].sum()) == 0
    n = Z * H * (S - 1) * (S - 1)
    frac = float(keep[:, :, 1:, :S - 1].sum()) / n
    sigma = math.sqrt(0.75 * 0.25 / n)
    print(f"dropout S={S}: kept {frac:.4f} of {n}, sigma {sigma:.4f}")
    assert abs(frac - 0.75) <= 4 * sigma
    keep[:, :, 0] = 1  # (rows the restatement zeroes itself)
    _gate_all(f"block_attn dropout S={S} dk={dk}", ctx, dqkv, qkv, cot, S, H, dk, keep, 1.0 / 0.75)


def test_block_attn_rejects_unsupported_shapes(dev):
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd._native import NativeError
    for S, dk in ((65, 64), (10, 48), (2, 16)):
        assert not K.block_attn_ok(S, dk)
        qkv = torch.zeros(S, 3 * dk, device=dev)
        with pytest.raises(NativeError):
            K.block_attn_fwd(qkv, torch.zeros(S, dk, device=dev), torch.zeros(S, device=dev), 1, S, 1, dk)
        with pytest.raises(NativeError):
            K.block_attn_bwd(qkv, torch.zeros(S, dk, device=dev), torch.zeros(S, device=dev), torch.zeros_like(qkv), 1,
                             S, 1, dk)
    assert K.block_attn_ok(42, 64) and K.block_attn_ok(64, 16) and K.block_attn_ok(3, 32)


# ------------------------------------------------------------------------------------------------ layout kernels
LAYOUTS = [("8/3/3", 9), ("8/3/3", 12), ("8/3/3", 13), ("40/16/16", 57)]
B, D = 2, 24


def _maps(key, T):
    bs, hop, la, _ = CH.LAYOUT_CASES[key]
    m = CH.load_json("cbt_layout")[key][str(T)]
    return bs, hop, la, m


def _chunk_ref(x, pe, m, bs, xscale, ctx_pe, mx=None, mc=None):
    """The chunked input from the recorded maps by index_select and mean (x (B, T, D), any dtype); mx / mc: frame
    and context dropout multipliers (B, T, D) / (B, nblk, D)."""
    nblk, S = m["nblk"], bs + 2
    fr = x * xscale + pe[:x.shape[1]].to(x.dtype)
    if mx is not None:
        fr = fr * mx.to(x.dtype)
    ctxv = torch.stack([x[:, lo:hi].mean(1) for lo, hi in m["ctx_window"]], 1)  # (B, nblk, D)
    if ctx_pe:
        ctxv = ctxv * xscale + pe[:nblk].to(x.dtype)
        if mc is not None:
            ctxv = ctxv * mc.to(x.dtype)
    zero = torch.zeros_like(x[:, :1])
    rows = []
    for k in range(nblk):
        for s in range(S):
            c = m["chunk_source"][k][s]
            rows.append(zero if c == -1 else (fr[:, c:c + 1] if c >= 0 else ctxv[:, -2 - c:-1 - c]))
    return torch.cat(rows, 1).reshape(x.shape[0], nblk, S, x.shape[2])


def _pe(n, dev=None, d=D):
    from espnet_slurp_amd.asr.encoder.abs_encoder import pos_table
    return pos_table("abs", n, d, dev if dev is not None else "cpu")


# D = 24: one partial pass of the 256 channel threads; 264 (40/16/16 only): a second, partial pass, as the recipe's
# D = 512 takes
@pytest.mark.parametrize("key,T,D", [(k, t, 24) for k, t in LAYOUTS] + [("40/16/16", 57, 264)])
@pytest.mark.parametrize("ctx_pe", [True, False])
def test_chunk_fwd_bwd(dev, key, T, ctx_pe, D):
    from espnet_slurp_amd import kernels as K
    bs, hop, la, m = _maps(key, T)
    nblk, S = m["nblk"], bs + 2
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, T, D, generator=g)
    cot = torch.randn(B, nblk, S, D, generator=g)
    xscale = math.sqrt(D)
    pe = _pe(T, d=D)
    xs = torch.full((B, nblk, S, D), float("nan"), device=dev)
    K.cbt_chunk_fwd(x.to(dev), pe.to(dev), xs, B, T, D, bs, hop, la, nblk, xscale, ctx_pe)
    dx = torch.full((B, T, D), float("nan"), device=dev)
    K.cbt_chunk_bwd(cot.to(dev), dx, B, T, D, bs, hop, la, nblk, xscale, ctx_pe)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    want = _chunk_ref(x64, pe.double(), m, bs, xscale, ctx_pe)
    want.backward(cot.double())
    scale = float(x.abs().max()) * xscale + 1.0
    # a frame slot is one fma (1 ulp); a mean is a sum of up to bs terms, a division and the fma
    e = float((xs.cpu().double() - want.detach()).abs().max())
    print(f"chunk_fwd {key} T={T}: {e:.3e} (bound {(bs + 2) * EPS * scale:.3e})")
    assert e <= (bs + 2) * EPS * scale
    for k in range(nblk):  # zero slots are exact zeros, frames in several blocks are the same bits
        for s in range(S):
            if m["chunk_source"][k][s] == -1:
                assert float(xs[:, k, s].abs().max()) == 0.0
    # a dx element sums at most ceil(bs / hop) frame terms and as many mean terms of three slots each
    nsum = 4 * -(-bs // hop) + 2
    gscale = float(cot.abs().max()) * xscale
    e = float((dx.cpu().double() - x64.grad).abs().max())
    print(f"chunk_bwd {key} T={T}: {e:.3e} (bound {nsum * EPS * gscale:.3e})")
    assert e <= nsum * EPS * gscale


@pytest.mark.parametrize("key,T", [("8/3/3", 13), ("40/16/16", 57)])
def test_chunk_dropout_is_shared_across_copies(dev, key, T):
    from espnet_slurp_amd import kernels as K
    bs, hop, la, m = _maps(key, T)
    nblk, S = m["nblk"], bs + 2
    g = torch.Generator().manual_seed(T + 1)
    x = torch.randn(B, T, D, generator=g)
    cot = torch.randn(B, nblk, S, D, generator=g)
    xscale, p = math.sqrt(D), 0.25
    pe = _pe(T)
    runs = []
    for _ in range(2):
        xs = torch.empty(B, nblk, S, D, device=dev)
        K.cbt_chunk_fwd(x.to(dev), pe.to(dev), xs, B, T, D, bs, hop, la, nblk, xscale, True, p, 77, 78)
        dx = torch.empty(B, T, D, device=dev)
        K.cbt_chunk_bwd(cot.to(dev), dx, B, T, D, bs, hop, la, nblk, xscale, True, p, 77, 78)
        torch.cuda.synchronize()
        runs.append((xs.cpu(), dx.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    xs, dx = runs[0]
    # the masks, read off the forward: keyed on (utterance, frame, channel) / (utterance, block, channel)
    mx = torch.zeros(B, T, D)
    seen = set()
    for k in range(nblk):
        for s in range(1, bs + 1):
            t = m["chunk_source"][k][s]
            if t < 0:
                continue
            mk = (xs[:, k, s] != 0).float()
            if t in seen:
                assert torch.equal(mk, mx[:, t]), (k, s, t)  # one mask in every block that holds the frame
            mx[:, t] = mk
            seen.add(t)
    assert len(seen) == T
    mc = (xs[:, :, S - 1] != 0).float()
    for k in range(nblk):  # slot 0 carries the very vector of the previous block's context slot
        assert torch.equal(xs[:, k, 0], xs[:, max(k - 1, 0), S - 1])
    n = mx.numel() + mc.numel()
    frac = float(mx.sum() + mc.sum()) / n
    assert abs(frac - 0.75) <= 4 * math.sqrt(0.75 * 0.25 / n), frac
    x64 = x.double().requires_grad_(True)
    want = _chunk_ref(x64, pe.double(), m, bs, xscale, True, mx / 0.75, mc / 0.75)
    want.backward(cot.double())
    scale = (float(x.abs().max()) * xscale + 1.0) / 0.75
    assert float((xs.double() - want.detach()).abs().max()) <= (bs + 3) * EPS * scale
    nsum = 4 * -(-bs // hop) + 4
    assert float((dx.double() - x64.grad).abs().max()) <= nsum * EPS * float(cot.abs().max()) * xscale / 0.75


def _ints(*shape, seed):
    """Small integers as floats: every sum of a few of them is exact in fp32."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("key,T", LAYOUTS)
def test_ctx_shift_fwd_bwd(dev, key, T):
    from espnet_slurp_amd import kernels as K
    bs, hop, la, m = _maps(key, T)
    nblk, S = m["nblk"], bs + 2
    x = _ints(B, nblk, S, D, seed=T)
    cot = _ints(B, nblk, S, D, seed=T + 1)
    prev = torch.tensor([max(k - 1, 0) for k in range(nblk)])
    xr = x.clone().requires_grad_(True)
    want = torch.cat([xr[:, prev, S - 1:S], xr[:, :, 1:]], 2)
    want.backward(cot)
    y = x.to(dev)
    K.cbt_ctx_shift(y, B, nblk, S, D)
    d = cot.to(dev)
    K.cbt_ctx_shift(d, B, nblk, S, D, backward=True)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want.detach())
    assert torch.equal(d.cpu(), xr.grad)
    assert float(d[:, :, 0].abs().max()) == 0.0


@pytest.mark.parametrize("key,T", LAYOUTS)
def test_unchunk_fwd_bwd(dev, key, T):
    from espnet_slurp_amd import kernels as K
    bs, hop, la, m = _maps(key, T)
    nblk, S = m["nblk"], bs + 2
    x = _ints(B, nblk, S, D, seed=T + 2)
    cot = _ints(B, T, D, seed=T + 3)
    flat = torch.tensor([k * S + s for k, s in m["output_source"]])
    xr = x.clone().requires_grad_(True)
    want = xr.view(B, nblk * S, D).index_select(1, flat)
    want.backward(cot)
    y = torch.full((B, T, D), float("nan"), device=dev)
    K.cbt_unchunk_fwd(x.to(dev), y, B, T, D, bs, hop, la, nblk)
    dxs = torch.full((B, nblk, S, D), float("nan"), device=dev)
    K.cbt_unchunk_bwd(cot.to(dev), dxs, B, T, D, bs, hop, la, nblk)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want.detach())
    assert torch.equal(dxs.cpu(), xr.grad)


def test_layout_kernels_reject_bad_layouts(dev):
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd._native import NativeError
    x = torch.zeros(1, 13, D, device=dev)
    xs = torch.zeros(1, 3, 10, D, device=dev)
    pe = _pe(13, dev)
    with pytest.raises(NativeError):  # a block count that is not the layout's
        K.cbt_chunk_fwd(x, pe, xs[:, :2].contiguous(), 1, 13, D, 8, 3, 3, 2, 1.0, True)
    with pytest.raises(NativeError):  # T' <= block_size has no blocks
        K.cbt_unchunk_fwd(xs[:, :1, :, :].contiguous(), x[:, :8].contiguous(), 1, 8, D, 8, 3, 3, 1)
    with pytest.raises(NativeError):  # the positional table is too short
        K.cbt_chunk_fwd(x, _pe(12, dev), xs, 1, 13, D, 8, 3, 3, 3, 1.0, True)


def test_layout_kernels_take_blocks_above_the_attention_limit(dev):
    """block_size 64 (66 slots, above esp_block_attn's 64) through chunk, ctx_shift and unchunk: against the host
    layout (BlockLayout, held to the reference's maps in tests/test_cbt_cpu.py), on integer data so every copy is
    exact; the chunk's context means against the restatement."""
    from espnet_slurp_amd import kernels as K
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import BlockLayout
    bs, hop, la, T = 64, 24, 24, 93
    L = BlockLayout(T, bs, hop, la)
    m = dict(nblk=L.nblk, chunk_source=L.chunk_source(), ctx_window=[list(L.window(k)) for k in range(L.nblk)],
             output_source=[list(p) for p in L.output_source()])
    nblk, S = L.nblk, L.S
    assert (nblk, S) == (3, 66)
    x = _ints(B, T, D, seed=5)
    pe = torch.zeros(T, D)
    xs = torch.full((B, nblk, S, D), float("nan"), device=dev)
    K.cbt_chunk_fwd(x.to(dev), pe.to(dev), xs, B, T, D, bs, hop, la, nblk, 2.0, True)
    want = _chunk_ref(x.double(), pe.double(), m, bs, 2.0, True)
    torch.cuda.synchronize()
    assert float((xs.cpu().double() - want).abs().max()) <= (bs + 2) * EPS * 16.0
    cot = _ints(B, nblk, S, D, seed=6)
    dx = torch.full((B, T, D), float("nan"), device=dev)
    K.cbt_chunk_bwd(cot.to(dev), dx, B, T, D, bs, hop, la, nblk, 2.0, True)
    x64 = x.double().requires_grad_(True)
    _chunk_ref(x64, pe.double(), m, bs, 2.0, True).backward(cot.double())
    assert float((dx.cpu().double() - x64.grad).abs().max()) <= 14 * EPS * 16.0
    ys = _ints(B, nblk, S, D, seed=7)
    y = torch.full((B, T, D), float("nan"), device=dev)
    K.cbt_unchunk_fwd(ys.to(dev), y, B, T, D, bs, hop, la, nblk)
    flat = torch.tensor([k * S + s for k, s in m["output_source"]])
    assert torch.equal(y.cpu(), ys.view(B, nblk * S, D).index_select(1, flat))
    dy = _ints(B, T, D, seed=8)
    dxs = torch.full((B, nblk, S, D), float("nan"), device=dev)
    K.cbt_unchunk_bwd(dy.to(dev), dxs, B, T, D, bs, hop, la, nblk)
    wantd = torch.zeros(B, nblk * S, D).index_copy(1, flat, dy).view(B, nblk, S, D)
    assert torch.equal(dxs.cpu(), wantd)
    sh = ys.to(dev)
    K.cbt_ctx_shift(sh, B, nblk, S, D)
    prev = torch.tensor([max(k - 1, 0) for k in range(nblk)])
    assert torch.equal(sh.cpu(), torch.cat([ys[:, prev, S - 1:S], ys[:, :, 1:]], 2))


# (B, T, F, D): T and F odd and even (a last input row / bin that no stride-2 patch reaches), D below, at and above
# the 64 lanes of the wave that sums the channels
@pytest.mark.parametrize("Bn,T,F,Dc", [(2, 11, 9, 96), (1, 12, 10, 32), (2, 7, 20, 130), (1, 3, 3, 64)])
def test_conv1_dgrad_vs_conv_transpose(dev, Bn, T, F, Dc):
    """esp_conv1_dgrad against torch's conv_transpose2d (the adjoint of the 3 x 3, stride-2 convolution) in fp64;
    gate as above: twice the fp32 restatement's error, never tighter than 1e-5."""
    from espnet_slurp_amd import kernels as K
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    g = torch.Generator().manual_seed(T * 100 + F)
    dz = torch.randn(Bn, T1, F1, Dc, generator=g)
    W = torch.randn(Dc, 1, 3, 3, generator=g) / 3.0

    def ref(dtype):
        y = torch.nn.functional.conv_transpose2d(dz.to(dtype).permute(0, 3, 1, 2), W.to(dtype), stride=2)[:, 0]
        out = torch.zeros(Bn, T, F, dtype=dtype)
        out[:, :y.shape[1], :y.shape[2]] = y
        return out

    dx = torch.full((Bn, T, F), float("nan"), device=dev)
    K.conv1_dgrad(dz.to(dev), W.to(dev), dx, Bn, T, F, Dc)
    torch.cuda.synchronize()
    _gate(f"conv1_dgrad T={T} F={F} D={Dc}", dx.cpu(), ref(torch.float32), ref(torch.float64))
