"""gemm_fwd_ws_kernel (csrc/gemm_fwd_ws.hip): the forward GEMMs on B planes with A gathered and split once per block
on producer waves -- the conv2 forward (I2C_KC x KC, bias + ReLU) and the Linear forward with the bias + dropout +
alpha + beta R epilogue (KC x KC, EPI_BDR: FFN w_2) -- against the LDS-DMA kernel it replaces (esp_set_fwd_ws(0)) on
the same inputs.  esp_set_fwd_ws(2) takes the new kernel for every eligible launch.

Both kernels issue the same MFMAs per accumulator, so every case requires torch.equal between the modes, and
agreement with an fp64 reference to 1e-5 of sum |a| |b| so that a bit-identical wrong answer cannot pass.

The new kernel takes unsplit launches only, and at these small shapes the host would split K (one or two tiles
cannot fill the chip: an unsplit and a split sum differ in their last bits, whichever kernel runs).  The cases
therefore run both modes with a zero-byte split-K workspace (_unsplit), which leaves every launch unsplit; the
launch counter (K.fwd_ws_launches) then shows that mode 2 ran the new kernel in every case and mode 0 never."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

# conv2 forward, z1 (Bn, T1, F1, C), 3 x 3 stride 2, bias + ReLU:
#  a  M = 4, one partial tile; N = 32; K = 288: nine slabs, the ring wraps
#  b  M = 231: two row tiles, the second partial; pixels cross map rows and utterances
#  c  even F1: the last input column is never read
#  d  N = 256, the full-width tile, and the workload's K = 2304
#  e  269 row tiles, more than one per block: blocks hand over to a next tile
#  f  N = 512: two column tiles
CONV = {"a": (1, 5, 5, 32), "b": (3, 23, 15, 64), "c": (2, 21, 14, 32), "d": (2, 9, 9, 256), "e": (16, 131, 67, 32),
        "f": (1, 7, 7, 512)}
# Linear EPI_BDR (M, N, K): bias, dropout p = 0.1, alpha = 0.5, beta = 1 with R aliasing C
#  a  partial third row tile   b  partial second column tile   c  K tail: 31 slabs + 8   d  one slab
LIN = {"a": (300, 256, 1024), "b": (130, 264, 96), "c": (128, 256, 1000), "d": (40, 32, 32)}
ALPHA, P_DROP, SEED = 0.5, 0.1, 1234


def _out(n):
    return (n - 3) // 2 + 1


@contextlib.contextmanager
def _unsplit():
    """K.gemm with a zero-byte split-K workspace: the host plans every launch unsplit."""
    prev = K._GEMM_WS_BYTES
    K._GEMM_WS_BYTES = 0
    try:
        yield
    finally:
        K._GEMM_WS_BYTES = prev


@contextlib.contextmanager
def _mode(mode, expect=None):
    """esp_set_fwd_ws(mode) around the body; expect: the launches of the new kernel the body must add."""
    prev = K.set_fwd_ws(mode)
    n0 = K.fwd_ws_launches()
    try:
        yield
    finally:
        K.set_fwd_ws(prev)
    if expect is not None:
        assert K.fwd_ws_launches() - n0 == expect, (mode, K.fwd_ws_launches() - n0, expect)


def _cols(z1):
    """im2col(z1) in fp64: (Bn T2 F2, 9 C), columns ordered (kt, kf, c)."""
    Bn, T1, F1, C = z1.shape
    cols = F.unfold(z1.double().permute(0, 3, 1, 2), 3, stride=2)  # (Bn, C * 9, L) ordered (c, kt, kf)
    return cols.view(Bn, C, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(-1, 9 * C)


def _conv_inputs(name):
    Bn, T1, F1, C = CONV[name]
    gen = torch.Generator().manual_seed(11 + ord(name))
    z1 = torch.randn(Bn, T1, F1, C, generator=gen)
    W = torch.randn(C, 9 * C, generator=gen) / math.sqrt(9 * C)
    b = torch.randn(C, generator=gen)
    return z1, W, b


def _run_conv(mode, z1, W, b, dev, expect=None):
    Bn, T1, F1, C = z1.shape
    T2, F2 = _out(T1), _out(F1)
    M = Bn * T2 * F2
    z1d, Wd, bd = z1.to(dev).contiguous(), W.to(dev), b.to(dev)
    z2 = torch.full((M, C), float("nan"), device=dev)
    with _unsplit(), _mode(mode, expect):
        K.gemm(M, C, 9 * C, z1d, Wd, z2, mode_a=K.I2C_KC, lda=0, mode_b=K.KC, ldb=9 * C, ldc=C, bias=bd, act=K.ACT_RELU,
               ic_a=(T1, F1, C, T2, F2), b_weight=True)
        torch.cuda.synchronize()
    return z2.cpu()


def _lin_inputs(name):
    M, N, Kd = LIN[name]
    gen = torch.Generator().manual_seed(31 + ord(name))
    A = torch.randn(M, Kd, generator=gen)
    W = torch.randn(N, Kd, generator=gen) / math.sqrt(Kd)
    b = torch.randn(N, generator=gen)
    R = torch.randn(M, N, generator=gen)
    return A, W, b, R


def _run_lin(mode, A, W, b, R, dev, expect=None, p=P_DROP, beta=1.0):
    """alpha * drop(A W^T + b) + beta * R written over R's buffer (R aliases C); beta = 0: no residual."""
    M, Kd = A.shape
    N = W.shape[0]
    Ad, Wd, bd = A.to(dev), W.to(dev), b.to(dev)
    C = R.to(dev).clone()
    key = torch.tensor([0x5EED1234], dtype=torch.int64, device=dev)
    K.set_rng_key(key)
    try:
        with _unsplit(), _mode(mode, expect):
            K.gemm(M, N, Kd, Ad, Wd, C, mode_a=K.KC, lda=Kd, mode_b=K.KC, ldb=Kd, ldc=N, bias=bd, alpha=ALPHA, beta=beta,
                   R=C if beta else None, drop_p=p, seed=SEED, b_weight=True)
            torch.cuda.synchronize()
    finally:
        K.set_rng_key(None)
    return C.cpu()


_CACHE = {}


def _conv_case(name, dev):
    if ("conv", name) not in _CACHE:
        z1, W, b = _conv_inputs(name)
        _CACHE["conv", name] = (z1, W, b, _run_conv(0, z1, W, b, dev, 0), _run_conv(2, z1, W, b, dev, 1),
                                _run_conv(2, z1, W, b, dev, 1))
    return _CACHE["conv", name]


def _lin_case(name, dev):
    if ("lin", name) not in _CACHE:
        A, W, b, R = _lin_inputs(name)
        _CACHE["lin", name] = (A, W, b, R, _run_lin(0, A, W, b, R, dev, 0), _run_lin(2, A, W, b, R, dev, 1),
                               _run_lin(2, A, W, b, R, dev, 1))
    return _CACHE["lin", name]


@pytest.mark.parametrize("name", list(CONV))
def test_fwd_ws_conv2_matches_old_kernel(dev, name):
    z1, W, b, old, new, _ = _conv_case(name, dev)
    assert torch.equal(new, old)
    cols = _cols(z1)
    ref = torch.relu(cols @ W.double().t() + b.double())
    den = cols.abs() @ W.double().abs().t() + b.double().abs()
    assert ((new.double() - ref).abs() / den).max().item() < 1e-5


@pytest.mark.parametrize("name", list(LIN))
def test_fwd_ws_linear_bdr_matches_old_kernel(dev, name):
    A, W, b, R, old, new, _ = _lin_case(name, dev)
    assert torch.equal(new, old)
    # the dropout mask and scale, read off the kernel the new one replaces: drop(0 + 1) with the same seed and key
    # (the dropout index depends on (m, n) alone)
    keep = _run_lin(0, torch.zeros_like(A), W, torch.ones_like(b), R, dev, p=P_DROP, beta=0.0).double() / ALPHA
    frac = (keep == 0).double().mean().item()
    assert 0.05 < frac < 0.15 and keep.max().item() == pytest.approx(1.0 / (1.0 - P_DROP), rel=1e-3), frac
    pre = A.double() @ W.double().t() + b.double()
    ref = ALPHA * keep * pre + R.double()
    den = ALPHA * keep * (A.double().abs() @ W.double().abs().t() + b.double().abs()) + R.double().abs()
    assert ((new.double() - ref).abs() / den).max().item() < 1e-5


@pytest.mark.parametrize("p,with_r,new_kernel", [(0.0, False, 0), (0.0, True, 0), (P_DROP, True, 1)],
                         ids=["p0-beta0", "p0-beta0-R", "p.1-beta0-R"])
def test_fwd_ws_linear_beta0(dev, p, with_r, new_kernel):
    """beta = 0.  Without dropout the epilogue resolves to another kind (bias alone, or the generic one when R is
    given), so p = 0 stays on the old kernel in every mode; with dropout and R given at beta = 0 the new kernel runs
    (the counter says which) and R contributes nothing."""
    A, W, b, R = _lin_inputs("a")
    M, Kd = A.shape
    N = W.shape[0]
    outs = []
    for mode in (0, 2):
        C = torch.full((M, N), float("nan"), device=dev)
        with _unsplit(), _mode(mode, new_kernel if mode else 0):
            K.gemm(M, N, Kd, A.to(dev), W.to(dev), C, mode_a=K.KC, lda=Kd, mode_b=K.KC, ldb=Kd, ldc=N, bias=b.to(dev),
                   alpha=ALPHA, beta=0.0, R=R.to(dev) if with_r else None, drop_p=p, seed=SEED, b_weight=True)
            torch.cuda.synchronize()
        outs.append(C.cpu())
    assert torch.equal(outs[1], outs[0])
    if not p:  # (with dropout: the fp64 check under the kernel's own mask is test_fwd_ws_linear_bdr_matches_old_kernel's)
        ref = ALPHA * (A.double() @ W.double().t() + b.double())
        den = ALPHA * (A.double().abs() @ W.double().abs().t() + b.double().abs())
        assert ((outs[1].double() - ref).abs() / den).max().item() < 1e-5


def _same_bits(new, old):
    """Equal bit for bit where finite, NaN in the same places."""
    assert torch.equal(torch.isnan(new), torch.isnan(old))
    assert torch.equal(torch.nan_to_num(new, nan=0.0), torch.nan_to_num(old, nan=0.0))


def test_fwd_ws_nonfinite_a_conv(dev):
    """One inf and one NaN in the conv1 map: the output equals the old kernel's, and only the output pixels whose
    receptive field holds one of them may be affected (their rows: ReLU turns a NaN sum into 0)."""
    z1, W, b = _conv_inputs("b")
    z1 = z1.clone()
    Bn, T1, F1, C = z1.shape
    T2, F2 = _out(T1), _out(F1)
    z1[0, 4, 6, 5] = float("inf")      # rows 1-2 x columns 2-3 of utterance 0's output grid
    z1[2, 22, 14, 9] = float("nan")    # the last pixel of the last utterance only
    old, new = _run_conv(0, z1, W, b, dev, 0), _run_conv(2, z1, W, b, dev, 1)
    _same_bits(new, old)
    clean = _conv_case("b", dev)[4]
    hit = torch.zeros(Bn, T2, F2, dtype=torch.bool)
    hit[0, 1:3, 2:4] = True
    hit[2, T2 - 1, F2 - 1] = True
    hit = hit.view(-1)
    assert torch.isfinite(new[~hit]).all()
    assert torch.equal(new[~hit], clean[~hit])


def test_fwd_ws_nonfinite_a_linear(dev):
    """One inf and one NaN in A: the output equals the old kernel's, NaNs in the same places, and the rows that do not
    read them stay finite and unchanged."""
    A, W, b, R = _lin_inputs("a")
    A = A.clone()
    A[7, 33] = float("inf")
    A[299, 1023] = float("nan")
    old, new = _run_lin(0, A, W, b, R, dev, 0), _run_lin(2, A, W, b, R, dev, 1)
    _same_bits(new, old)
    # (a dropped element of those rows is 0 + R: finite)
    assert torch.isnan(new[7]).sum().item() > 128 and torch.isnan(new[299]).sum().item() > 128
    rows = torch.ones(A.shape[0], dtype=torch.bool)
    rows[7] = rows[299] = False
    assert torch.isfinite(new[rows]).all()
    assert torch.equal(new[rows], _lin_case("a", dev)[5][rows])


@pytest.mark.parametrize("kind,name", [("conv", n) for n in CONV] + [("lin", n) for n in LIN])
def test_fwd_ws_deterministic(dev, kind, name):
    *_, new, new2 = _conv_case(name, dev) if kind == "conv" else _lin_case(name, dev)
    assert torch.equal(new, new2)


def test_fwd_ws_auto_keeps_small_shapes_on_the_old_kernel(dev):
    """Eligible shapes below the auto rule's thresholds (K of nine slabs; one round of tiles): mode 1 launches the old
    kernel (the counter stays) and gives its result."""
    z1, W, b, old, *_ = _conv_case("e", dev)
    assert torch.equal(_run_conv(1, z1, W, b, dev, 0), old)
    A, Wl, bl, R, oldl, *_ = _lin_case("a", dev)
    assert torch.equal(_run_lin(1, A, Wl, bl, R, dev, 0), oldl)


def test_fwd_ws_subsampling_block(dev):
    """Conv2dSubsampling forward + backward (D = 64, B = 2, 67 frames) under modes 0 and 2: equal output and equal
    gradients; mode 2 ran the conv2 forward on the new kernel."""
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
    res = {}
    for mode in (0, 2):
        flat.grad.zero_()
        with _unsplit(), _mode(mode, 1 if mode else 0):
            out, c = mod.fwd(x.to(dev), math.sqrt(D), 0.0, Seeds(3), True)
            dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
            mod.bwd(c, dout.to(dev))
            torch.cuda.synchronize()
        res[mode] = (out.cpu().clone(), flat.grad.cpu().clone())
    assert torch.isfinite(res[2][0]).all() and res[2][1].abs().sum().item() > 0
    assert torch.equal(res[2][0], res[0][0]) and torch.equal(res[2][1], res[0][1])


def test_fwd_ws_ffn_block(dev):
    """One encoder FFN (256 -> 1024 -> 256, Swish, dropout 0.1, residual dropout 0.1, alpha 0.5) forward + backward under
    modes 0 and 2: equal output, input gradient and parameter gradients; mode 2 ran w_2's forward on the new kernel."""
    from espnet_slurp_amd.blocks import PositionwiseFeedForward, Seeds
    from espnet_slurp_amd.flat import FlatParams

    torch.manual_seed(3)
    ff = PositionwiseFeedForward(256, 1024, 0.1, K.ACT_SWISH).to(dev)
    with torch.no_grad():
        for p in ff.parameters():
            p.copy_(torch.randn_like(p) * 0.05)
    flat = FlatParams(ff, dev)
    gen = torch.Generator().manual_seed(121)
    x, dout = torch.randn(300, 256, generator=gen).to(dev), torch.randn(300, 256, generator=gen).to(dev)
    res = {}
    for mode in (0, 2):
        flat.grad.zero_()
        with _unsplit(), _mode(mode, 1 if mode else 0), K.param_cast_scope():
            out, c = ff.fwd(x, x, 0.5, 0.1, Seeds(5), True)
            dx = ff.bwd(c, dout)
            torch.cuda.synchronize()
        res[mode] = (out.cpu().clone(), dx.cpu().clone(), flat.grad.cpu().clone())
    assert torch.isfinite(res[2][0]).all()
    for a, b in zip(res[2], res[0]):
        assert torch.equal(a, b)
