"""The cgMLP gating-unit kernels (csrc/cgmlp.hip) against a torch-CPU fp64 restatement of
espnet2/asr/layers/cgmlp.py:57-81 written here (F.gelu, F.layer_norm(eps=1e-12), F.conv1d(groups=C)).

Gate on every output and gradient: rel_err <= max(1e-5, 2 e32), e32 the same restatement run in fp32 on the
CPU against its fp64 run (1e-5: the floor of the fp32 elementwise kernel tests)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import keep_scale, rel_err

pytestmark = pytest.mark.gpu

# (B, T', C, k): T' < k with ragged utterance count; two 64-frame tiles with C not a multiple of 64; four channel
# tiles with the small kernel (the generic depthwise adjoint path); one utterance shorter than the half window, one
# float4 of channels
SHAPES = [(3, 29, 48, 31), (2, 74, 48, 31), (3, 74, 256, 7), (1, 5, 8, 31)]


def _inputs(B, T, C, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(v=1.5 * r(B * T, 2 * C), gamma=1.0 + 0.2 * r(C), beta=0.2 * r(C), W=r(C, 1, k) / np.sqrt(k),
                bias=1.0 + 0.2 * r(C), dout=r(B * T, C))


def _restatement(x, B, T, C, k, dtype):
    """(o, dv, dgamma, dbeta, dW, dbias) of the unit on the CPU in `dtype` (no dropout)."""
    p = {n: t.to(dtype).clone().requires_grad_(n != "dout") for n, t in x.items()}
    a = F.gelu(p["v"])
    a_r, a_g = a[:, :C], a[:, C:]
    n = F.layer_norm(a_g, (C,), p["gamma"], p["beta"], eps=1e-12)
    g = F.conv1d(n.view(B, T, C).transpose(1, 2), p["W"], p["bias"], padding=(k - 1) // 2, groups=C)
    o = a_r * g.transpose(1, 2).reshape(B * T, C)
    o.backward(p["dout"])
    return [o.detach()] + [p[n].grad for n in ("v", "gamma", "beta", "W", "bias")]


def _gpu(x, B, T, C, k, dev, drop_p=0.0, seed=0, tvalid=None, planes=0):
    from espnet_slurp_amd import kernels as K
    d = {n: t.float().to(dev).contiguous() for n, t in x.items()}
    M = B * T
    mean = torch.empty(M, device=dev)
    rstd = torch.empty(M, device=dev)
    K.csgu_stats(d["v"], mean, rstd, 1e-12)
    o = torch.full((M, C), float("nan"), device=dev)
    tv = None if tvalid is None else torch.tensor([tvalid], dtype=torch.int32, device=dev)
    K.csgu_fwd(d["v"], mean, rstd, d["gamma"], d["beta"], d["W"], d["bias"], o, B, T, k, drop_p=drop_p, seed=seed,
               tvalid=tv)
    dv = K.Planes(M, 2 * C, dev, planes) if planes else torch.full((M, 2 * C), float("nan"), device=dev)
    grads = [torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, 1, k, device=dev),
             torch.zeros(C, device=dev)]
    K.csgu_bwd(d["v"], mean, rstd, d["gamma"], d["beta"], d["W"], d["bias"], d["dout"], dv, grads[0], grads[1],
               grads[2], grads[3], B, T, k, drop_p=drop_p, seed=seed, tvalid=tv)
    torch.cuda.synchronize()
    return [o, dv.float() if planes else dv] + grads


NAMES = ("o", "dv", "dgamma", "dbeta", "dW", "dbias")


@pytest.mark.parametrize("B,T,C,k", SHAPES)
def test_csgu_fwd_bwd_vs_fp64_restatement(dev, B, T, C, k):
    x = _inputs(B, T, C, k, 11)
    r64 = _restatement(x, B, T, C, k, torch.float64)
    r32 = _restatement(x, B, T, C, k, torch.float32)
    got = _gpu(x, B, T, C, k, dev)
    bad = []
    for n, g, a64, a32 in zip(NAMES, got, r64, r32):
        e32 = rel_err(a32.numpy(), a64.numpy())
        e = rel_err(g.cpu().numpy(), a64.numpy())
        print(f"CSGU {B}x{T}x{C} k={k} {n}: e_gpu={e:.3e} e32={e32:.3e}")
        if not e <= max(1e-5, 2 * e32):
            bad.append((n, e, e32))
    assert not bad, bad


def test_window_never_crosses_an_utterance_boundary(dev):
    """Changing utterance 1 leaves utterance 0's and 2's outputs and input gradients bit-identical (zero padding
    applies outside each utterance's own rows), and changes utterance 1's."""
    B, T, C, k = 3, 29, 48, 31
    x = _inputs(B, T, C, k, 12)
    y = {n: t.clone() for n, t in x.items()}
    y["v"][T:2 * T] = 1.5 * torch.randn(T, 2 * C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a, b = _gpu(x, B, T, C, k, dev), _gpu(y, B, T, C, k, dev)
    for i in (0, 1):  # o, dv
        assert torch.equal(a[i][:T], b[i][:T]) and torch.equal(a[i][2 * T:], b[i][2 * T:])
        assert not torch.equal(a[i][T:2 * T], b[i][T:2 * T])


@pytest.mark.parametrize("B", [2, 1])
def test_tvalid_equals_the_unpadded_run(dev, B):
    """A buffer of T' frames per utterance whose frames at and after tvalid = T' - 9 hold garbage (NaN) equals the
    run on the tvalid frames alone, bit for bit: outputs, dv and the depthwise weight gradient (the new kernels and
    the depthwise kernels tile an utterance's own frames); the three column-sum gradients are reduced over all
    B * T' rows in 32-row groups whose composition moves with the padding when B > 1, so there they take the gate
    against the fp64 restatement, and the one-utterance run checks them bit for bit too.  Padded rows read 0."""
    T, C, k = 74, 48, 31
    Tv = T - 9
    x = _inputs(B, Tv, C, k, 13)
    pad = {n: t.clone() for n, t in x.items()}
    for n in ("v", "dout"):
        full = torch.full((B, T, x[n].shape[1]), float("nan"), dtype=torch.float64)
        full[:, :Tv] = x[n].view(B, Tv, -1)
        pad[n] = full.view(B * T, -1)
    ref = _gpu(x, B, Tv, C, k, dev)
    got = _gpu(pad, B, T, C, k, dev, tvalid=Tv)
    for i in (0, 1):
        g3 = got[i].view(B, T, -1)
        assert torch.equal(g3[:, :Tv].reshape(B * Tv, -1), ref[i]), NAMES[i]
        assert torch.equal(g3[:, Tv:], torch.zeros_like(g3[:, Tv:])), NAMES[i]
    assert torch.equal(got[4], ref[4]), "dW"
    if B == 1:
        for i in (2, 3, 5):
            assert torch.equal(got[i], ref[i]), NAMES[i]
    else:
        r64 = _restatement(x, B, Tv, C, k, torch.float64)
        r32 = _restatement(x, B, Tv, C, k, torch.float32)
        for i in (2, 3, 5):
            e32 = rel_err(r32[i].numpy(), r64[i].numpy())
            assert rel_err(got[i].cpu().numpy(), r64[i].numpy()) <= max(1e-5, 2 * e32), NAMES[i]


def test_dropout(dev):
    from espnet_slurp_amd import kernels as K
    B, T, C, k = 3, 74, 256, 7
    p, seed = 0.1, 0x1234567890ABCDEF
    x = _inputs(B, T, C, k, 14)
    base = _gpu(x, B, T, C, k, dev)
    a = _gpu(x, B, T, C, k, dev, drop_p=p, seed=seed)
    b = _gpu(x, B, T, C, k, dev, drop_p=p, seed=seed)
    for u, w in zip(a, b):  # one seed twice: bit-identical
        assert torch.equal(u, w)
    # the mask is esp_scale_dropout's for the same seed over the (M, C) output
    ones = torch.ones(B * T, C, device=dev)
    m = torch.empty_like(ones)
    K.scale_dropout(ones, m, drop_p=p, seed=seed)
    keep = m != 0
    N = keep.numel()
    assert N >= 4096
    kept = int(keep.sum())
    assert abs(kept - N * (1 - p)) <= 5 * np.sqrt(N * p * (1 - p)), (kept, N)
    scale = torch.tensor(keep_scale(p), dtype=torch.float32, device=dev)
    assert torch.equal(a[0][keep], (base[0] * scale)[keep])
    assert torch.equal(a[0][~keep], torch.zeros_like(a[0][~keep]))
    da_r = a[1][:, :C]
    assert torch.equal(da_r[~keep], torch.zeros_like(da_r[~keep]))
    assert int((da_r[keep] != 0).sum()) > 0.99 * kept
    other = _gpu(x, B, T, C, k, dev, drop_p=p, seed=seed + 1)
    assert not torch.equal(other[0], a[0])


@pytest.mark.parametrize("planes", [3, 1])
def test_dv_as_planes(dev, planes):
    """dv written as bf16 planes for channel_proj1's gradient GEMMs: n = 3 is the exact split of the fp32 dv,
    n = 1 its bf16 rounding (2^-9 relative)."""
    B, T, C, k = 2, 74, 48, 31
    x = _inputs(B, T, C, k, 15)
    f = _gpu(x, B, T, C, k, dev)
    g = _gpu(x, B, T, C, k, dev, planes=planes)
    if planes == 3:
        assert torch.equal(g[1], f[1])
    else:
        assert float(((g[1] - f[1]).abs() / f[1].abs().clamp_min(1e-30)).max()) <= 2.0 ** -8
    for i in (0, 2, 3, 4, 5):
        assert torch.equal(g[i], f[i])


def test_bad_arguments_are_rejected(dev):
    from espnet_slurp_amd import _native, kernels as K
    v = torch.zeros(8, 24, device=dev)
    s = torch.zeros(8, device=dev)
    o = torch.zeros(8, 12, device=dev)
    w = torch.zeros(12, 1, 4, device=dev)
    c = torch.zeros(12, device=dev)
    with pytest.raises(_native.NativeError, match="k odd"):
        K.csgu_fwd(v, s, s, c, c, w, c, o, 1, 8, 4)
    with pytest.raises(_native.NativeError, match="p must be < 1"):
        K.csgu_fwd(v, s, s, c, c, torch.zeros(12, 1, 3, device=dev), c, o, 1, 8, 3, drop_p=1.0)
