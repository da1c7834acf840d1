"""The E-Branchformer merge kernels (csrc/ebf_merge.hip) against torch.nn.functional.conv1d(groups=C) in fp64 on
the host, and its autograd.

Gate on u, d1 | d2, dW and dbias: rel_err(fused, fp64) <= max(1e-6, 2 e_composed), e_composed the error of the
composed path (kernels.EBF_MERGE_FUSED = False: esp_dwconv1d + add, esp_dwconv1d(flip), esp_dwconv1d_wgrad,
esp_colsum) on the same inputs.  1e-6 is a few fp32 roundings of a sum of at most 32 products of O(1) terms
relative to the tensor's maximum: both paths sit near it and differ only in summation order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

B = 3
# C = 128: two full channel tiles; 80: a guarded second tile.  T' = 1, 5 < pad of k 31; 29 (the model fixture's);
# 64 | 65: the frame-tile edge; 130: three frame tiles walked by one backward block; 300: five tiles, two backward
# blocks per utterance (4 + 1 tiles).
CS, TS, KS = (128, 80), (1, 5, 29, 64, 65, 130, 300), (1, 3, 7, 31)
NAMES = ("u", "d1|d2", "dW", "dbias")


def _inputs(T, C, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(xc=r(B * T, C), W=r(C, 1, k) / np.sqrt(k), bias=0.2 * r(C), du=r(B * T, C))


_TRUTH = {}


def _truth(T, C, k, seed=5, tv=None):
    """(inputs, [u, dxc, dW, dbias]) in fp64, computed once per case; with tv only the first tv frames of every
    utterance exist (the others: zero output, zero gradient)."""
    key = (T, C, k, seed, tv)
    if key not in _TRUTH:
        x = _inputs(T, C, k, seed)
        Tv = T if tv is None else tv
        xc = x["xc"].view(B, T, C)[:, :Tv].clone().requires_grad_()
        W, b = x["W"].clone().requires_grad_(), x["bias"].clone().requires_grad_()
        y = xc + F.conv1d(xc.transpose(1, 2), W, b, padding=(k - 1) // 2, groups=C).transpose(1, 2)
        y.backward(x["du"].view(B, T, C)[:, :Tv])
        u = torch.zeros(B, T, C, dtype=torch.float64)
        dx = torch.zeros(B, T, C, dtype=torch.float64)
        u[:, :Tv], dx[:, :Tv] = y.detach(), xc.grad
        _TRUTH[key] = (x, [u.view(B * T, C), dx.view(B * T, C), W.grad, b.grad])
    return _TRUTH[key]


def _gpu(x, T, C, k, dev, fused, tv=None, planes=0, prefill=None):
    from espnet_slurp_amd import kernels as K
    d = {n: t.float().to(dev).contiguous() for n, t in x.items()}
    tvd = None if tv is None else torch.tensor([tv], dtype=torch.int32, device=dev)
    dW = torch.zeros(C, 1, k, device=dev) if prefill is None else prefill[0].clone()
    db = torch.zeros(C, device=dev) if prefill is None else prefill[1].clone()
    prev = K.EBF_MERGE_FUSED
    K.EBF_MERGE_FUSED = fused
    try:
        u = K.ebf_merge_fwd(d["xc"], d["W"], d["bias"], B, T, k, tvalid=tvd, planes=planes)
        d1, d2 = K.ebf_merge_bwd(d["du"], d["xc"], d["W"], dW, db, B, T, k, tvalid=tvd)
    finally:
        K.EBF_MERGE_FUSED = prev
    torch.cuda.synchronize()
    return [u, torch.cat([d1, d2], dim=1), dW, db]


def _gate(tag, x, truth, T, C, k, dev, tv=None):
    fused = _gpu(x, T, C, k, dev, True, tv)
    comp = _gpu(x, T, C, k, dev, False, tv)
    bad = []
    for n, gf, gc, t in zip(NAMES, fused, comp, truth):
        ef, ec = rel_err(gf.cpu().numpy(), t.numpy()), rel_err(gc.cpu().numpy(), t.numpy())
        print(f"EBF_MERGE {tag} T'={T} C={C} k={k} {n}: e_fused={ef:.3e} e_composed={ec:.3e}")
        if not ef <= max(1e-6, 2 * ec):
            bad.append((k, n, ef, ec))
    return bad


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("T", TS)
def test_merge_fwd_bwd_vs_fp64_conv1d(dev, T, C):
    bad = []
    for k in KS:
        x, truth = _truth(T, C, k)
        bad += _gate("full", x, truth, T, C, k, dev)
    assert not bad, bad


def test_tvalid_cuts_the_window(dev):
    """A bucketed batch: 65 rows per utterance of which 40 exist.  The rows beyond hold finite garbage in xc and du;
    they are read as zero padding and written as 0."""
    T, C, k, tv = 65, 128, 31, 40
    x, truth = _truth(T, C, k, seed=6, tv=tv)
    assert float(x["xc"].view(B, T, C)[:, tv:].abs().min()) > 0.0
    bad = _gate("tvalid", x, truth, T, C, k, dev, tv=tv)
    assert not bad, bad
    u, dx, _, _ = _gpu(x, T, C, k, dev, True, tv)
    assert float(u.view(B, T, C)[:, tv:].abs().max()) == 0.0 and float(dx.view(B, T, C)[:, tv:].abs().max()) == 0.0


@pytest.mark.parametrize("T,C,k", [(65, 80, 31), (5, 128, 31), (130, 128, 7)])
def test_planes_output_is_the_fp32_output(dev, T, C, k):
    """The 3-plane u summed in fp32 equals the fp32 u bit for bit; the 1-plane u is its bf16 rounding."""
    x, _ = _truth(T, C, k)
    u32 = _gpu(x, T, C, k, dev, True)[0]
    u3 = _gpu(x, T, C, k, dev, True, planes=3)[0]
    u1 = _gpu(x, T, C, k, dev, True, planes=1)[0]
    assert u3.n == 3 and u3.ld == C and torch.equal(u3.float(), u32)
    p = u3.buf.view(3, B * T, C).float()
    assert torch.equal((p[0] + p[1]) + p[2], u32)
    assert torch.equal(u1.float(), u32.bfloat16().float())


def test_two_launches_give_equal_gradients_and_accumulation_is_honoured(dev):
    T, C, k = 130, 80, 31
    x, truth = _truth(T, C, k)
    a = _gpu(x, T, C, k, dev, True)
    b = _gpu(x, T, C, k, dev, True)
    for n, ga, gb in zip(NAMES, a, b):
        assert torch.equal(ga, gb), n
    g = torch.Generator().manual_seed(9)
    pre = (torch.randn(C, 1, k, generator=g).to(dev), torch.randn(C, generator=g).to(dev))
    c = _gpu(x, T, C, k, dev, True, prefill=pre)
    # dW += s is one fp32 add of the reduced sum: the pre-filled result is that add exactly
    assert torch.equal(c[2], pre[0] + a[2]) and torch.equal(c[3], pre[1] + a[3])
    assert rel_err((c[2] - pre[0]).cpu().numpy(), truth[2].numpy()) < 1e-5


@pytest.mark.parametrize("T,C,k", [(5, 128, 33), (5, 128, 4), (5, 12, 3), (0, 128, 3)])
def test_unsupported_arguments_fail_the_argument_check(dev, T, C, k):
    from espnet_slurp_amd import _native
    from espnet_slurp_amd import kernels as K
    n = B * max(T, 1)
    xc = torch.zeros(n, C, device=dev)
    W, bias = torch.zeros(C, 1, k, device=dev), torch.zeros(C, device=dev)
    u = torch.zeros(n, C, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_native.NativeError, match="esp_ebf_merge_fwd: bad shape"):
        _native.call("esp_ebf_merge_fwd", xc.data_ptr(), W.data_ptr(), bias.data_ptr(), u.data_ptr(), 0, 0, B, T, C, k,
                     None, st)
    d1 = torch.zeros(n, C // 2, device=dev)
    with pytest.raises(_native.NativeError, match="esp_ebf_merge_bwd: bad shape"):
        _native.call("esp_ebf_merge_bwd", u.data_ptr(), xc.data_ptr(), W.data_ptr(), d1.data_ptr(), d1.data_ptr(),
                     W.data_ptr(), bias.data_ptr(), B, T, C, k, None, 0, None, st)
    assert K.EBF_MERGE_KMAX == 31
