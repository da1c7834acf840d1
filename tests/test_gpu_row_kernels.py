"""Row kernels that pick a template instantiation from the row length, at every instantiation.

LayerNorm (csrc/norm.hip, through the kernels.py wrappers): ln_fwd_kernel<4|8|32> by ceil(D / 64),
ln_fwd_planes_kernel<1|2|8> (planes and dual) and ln_bwd_kernel<1|2|8> by ceil(D / 256), up to MAXD = 2048; the
backward at M = 1, 5, 33, 77 rows (LN_RB = 4 rows per wave pass, 32 rows per block: less than one pass, a partial
pass, one row into the second and the third block), accumulated dw / db and the accumulate form of dx.

Materialised softmax family (csrc/attention.hip): esp_attn_softmax_fwd / _bwd at PER 1, 2, 4, 8, 16 (both edges of
each step) and in the loop kernels (rows past 1024), Tq != Tk, causal, an utterance of length 0, in place, with
dropout (forward and backward masks tied through the element index); esp_attn_softmax_bwd_relpos latest and legacy
in softmax_bwd_relpos_kernel<PER, REL> (row pitch no multiple of 4), softmax_bwd_relpos4_kernel<Q, REL, pow2>
(16-B aligned rows) and softmax_bwd_loop_kernel<REL> (T = 1025); esp_attn_softmax_bwd_relpos_band; esp_relshift_bwd.

Gate of every floating-point comparison: the reference is plain torch on the CPU in fp64, the yardstick the same
torch code in fp32; per output tensor, e(a) = max|a - ref64| / max|ref64|, e(ours) <= max(2 e(torch fp32), 1e-5).
Both figures are printed (GATE lines).  Every output buffer is NaN (or a stated sentinel) on entry.
"""
import functools
import math

import pytest
import torch

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd._native import NativeError
from oracle import espnet_cpu as O

pytestmark = pytest.mark.gpu

FLOOR = 1e-5
EPS = 1e-12
NAN = float("nan")


def _gate(what, ours, ref64, ref32):
    ours, ref64, ref32 = ours.detach().cpu(), ref64.detach().cpu(), ref32.detach().cpu()
    assert ours.shape == ref64.shape, (what, ours.shape, ref64.shape)
    assert not torch.isnan(ours).any(), (what, "NaN (an element was not written)")
    m = float(ref64.abs().max()) or 1.0  # (a reference that is identically 0: the absolute error)
    e = float((ours.double() - ref64).abs().max()) / m
    r = float((ref32.double() - ref64).abs().max()) / m
    gate = max(2 * r, FLOOR)
    print(f"GATE {what}: ours {e:.3e} torch_fp32 {r:.3e} gate {gate:.3e}")
    assert e <= gate, (what, e, r, gate)


def _nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


# ----------------------------------------------------------------------------------------------- LayerNorm
@functools.lru_cache(maxsize=None)
def _ln_inputs(M, D, kind):
    g = torch.Generator().manual_seed(7000 + 131 * M + D)
    x = torch.randn(M, D, generator=g)
    x = 100.0 + 0.5 * x if kind == "offset" else 3.0 * x + 1.5
    w = 1.0 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    dx0, dw0, db0 = torch.randn(M, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    return x, w, b, dy, dx0, dw0, db0


@functools.lru_cache(maxsize=None)
def _ln_ref(M, D, kind, dtype):
    """y, mean, rstd, dx, dw, db of F.layer_norm's kernel and its autograd on the CPU in dtype."""
    x, w, b, dy = (t.to(dtype).clone() for t in _ln_inputs(M, D, kind)[:4])  # (the inputs are shared: copies)
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(x, (D,), w, b, EPS)
    y.backward(dy)
    return y.detach(), mean.detach().reshape(M), rstd.detach().reshape(M), x.grad, w.grad, b.grad


def _ln_fwd(dev, M, D, kind):
    x, w, b = (t.to(dev) for t in _ln_inputs(M, D, kind)[:3])
    y, mean, rstd = _nan(M, D, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev)
    K.layernorm_fwd(x, w, b, y, mean, rstd, EPS)
    torch.cuda.synchronize()
    return y, mean, rstd


def _gate_ln_fwd(what, M, D, kind, y, mean, rstd):
    r64, r32 = _ln_ref(M, D, kind, torch.float64), _ln_ref(M, D, kind, torch.float32)
    for i, (name, t) in enumerate((("y", y), ("mean", mean), ("rstd", rstd))):
        _gate(f"{what} M={M} D={D} {kind} {name}", t, r64[i], r32[i])


@pytest.mark.parametrize("D", [1, 3, 64, 255, 256, 257, 320, 512, 513, 1024, 2047, 2048])
def test_layernorm_fwd_every_instantiation(dev, D):
    """ln_fwd_kernel<4> (D <= 256), <8> (<= 512), <32> (<= 2048); M = 5: one full block of 4 rows plus one."""
    M = 5
    _gate_ln_fwd("layernorm_fwd", M, D, "plain", *_ln_fwd(dev, M, D, "plain"))


def test_layernorm_fwd_rejects_rows_past_maxd(dev):
    M, D = 5, 2049
    x, w, b = torch.zeros(M, D, device=dev), torch.ones(D, device=dev), torch.zeros(D, device=dev)
    with pytest.raises(NativeError):
        K.layernorm_fwd(x, w, b, _nan(M, D, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev), EPS)


def _planes(M, D, dev, n, ld):
    """Planes at row pitch ld, every bf16 element NaN on entry."""
    p = K.Planes(M, D, dev, n, buf=torch.full((n * M * ld,), NAN, dtype=torch.bfloat16, device=dev))
    p.ld, p.ps = ld, M * ld
    return p


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("D", [4, 252, 256, 260, 512, 516, 2048])
def test_layernorm_planes_and_dual_every_instantiation(dev, D, pad):
    """ln_fwd_planes_kernel<1> (D <= 256), <2> (<= 512), <8> (<= 2048) at row pitch D and D + 8: the three planes sum
    to the dual form's fp32 y bit for bit (hi = bf16(y)), the one-plane form is to_bf16(y), mean and rstd are the
    same in all three, the pitch's padding columns stay untouched."""
    M, ld = 5, D + pad
    x, w, b = (t.to(dev) for t in _ln_inputs(M, D, "plain")[:3])
    p3, p1 = _planes(M, D, dev, 3, ld), _planes(M, D, dev, 1, ld)
    m3, r3, m1, r1, md, rd = (_nan(M, dev=dev) for _ in range(6))
    K.layernorm_fwd_planes(x, w, b, p3, m3, r3, EPS)
    K.layernorm_fwd_planes(x, w, b, p1, m1, r1, EPS)
    y = _nan(M, D, dev=dev)
    K.layernorm_fwd_dual(x, w, b, y, md, rd, EPS)
    torch.cuda.synchronize()
    _gate_ln_fwd(f"layernorm_fwd_dual ld={ld}", M, D, "plain", y, md, rd)
    tw = K.twin_planes(y)
    assert tw is not None and tw.n == 3 and torch.equal(tw.float(), y)
    assert torch.equal(p3.float(), y)
    assert torch.equal(p3.buf.view(3, M, ld)[0, :, :D], y.to(torch.bfloat16))
    assert torch.equal(p1.buf.view(M, ld)[:, :D], K.to_bf16(y, M, D, D))
    for m, r in ((m3, r3), (m1, r1)):
        assert torch.equal(m, md) and torch.equal(r, rd)
    if pad:
        assert torch.isnan(p3.buf.view(3, M, ld)[:, :, D:].float()).all()
        assert torch.isnan(p1.buf.view(M, ld)[:, D:].float()).all()


@pytest.mark.parametrize("D", [258, 2052])
def test_layernorm_planes_and_dual_reject_bad_rows(dev, D):
    M = 5
    x, w, b = torch.zeros(M, D, device=dev), torch.ones(D, device=dev), torch.zeros(D, device=dev)
    planes = _planes(M, D, dev, 3, (D + 7) // 8 * 8)
    with pytest.raises(NativeError):
        K.layernorm_fwd_planes(x, w, b, planes, _nan(M, dev=dev), _nan(M, dev=dev), EPS)
    with pytest.raises(NativeError):
        K.layernorm_fwd_dual(x, w, b, _nan(M, D, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev), EPS)


def _ln_bwd_case(dev, M, D, kind, accumulate):
    x, w, b, dy, dx0, dw0, db0 = _ln_inputs(M, D, kind)
    r64, r32 = _ln_ref(M, D, kind, torch.float64), _ln_ref(M, D, kind, torch.float32)
    y, mean, rstd = _ln_fwd(dev, M, D, kind)
    dx = dx0.to(dev) if accumulate else _nan(M, D, dev=dev)
    dw, db = dw0.to(dev), db0.to(dev)  # dw / db are accumulated: non-zero on entry
    K.layernorm_bwd(dy.to(dev), x.to(dev), w.to(dev), mean, rstd, dx, dw, db, accumulate=accumulate)
    torch.cuda.synchronize()
    what = f"layernorm_bwd M={M} D={D} {kind} acc={int(accumulate)}"
    base = dx0 if accumulate else torch.zeros(M, D)
    _gate(what + " dx", dx, base.double() + r64[3], base + r32[3])
    _gate(what + " dw", dw, dw0.double() + r64[4], dw0 + r32[4])
    _gate(what + " db", db, db0.double() + r64[5], db0 + r32[5])


@pytest.mark.parametrize("M", [1, 5, 33, 77])
@pytest.mark.parametrize("D", [4, 80, 252, 256, 260, 512, 516, 1024, 2048])
def test_layernorm_bwd_every_instantiation(dev, D, M):
    """ln_bwd_kernel<1> (D <= 256), <2> (<= 512), <8> (<= 2048), partial quad tails (D = 80, 252, 260, 516)."""
    _ln_bwd_case(dev, M, D, "plain", False)


@pytest.mark.parametrize("M", [1, 5, 33, 77])
@pytest.mark.parametrize("D", [260, 2048])
def test_layernorm_bwd_accumulates_into_dx(dev, D, M):
    _ln_bwd_case(dev, M, D, "plain", True)


def test_layernorm_rows_with_a_large_mean(dev):
    """x = 100 + 0.5 randn: the variance is 4e4 times smaller than the squared mean."""
    M, D = 77, 516
    _gate_ln_fwd("layernorm_fwd", M, D, "offset", *_ln_fwd(dev, M, D, "offset"))
    _ln_bwd_case(dev, M, D, "offset", False)


@pytest.mark.parametrize("D", [3, 257, 2048])
def test_layernorm_constant_rows(dev, D):
    """Rows of 2.0: every partial sum is exact in fp32 (an integer multiple of 2 up to 4096), so mean == 2, the
    deviations are 0, rstd = 1 / sqrt(eps) is finite and y == bias bit for bit."""
    M = 5
    w, b = (t.to(dev) for t in _ln_inputs(M, D, "plain")[1:3])
    x = torch.full((M, D), 2.0, device=dev)
    y, mean, rstd = _nan(M, D, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev)
    K.layernorm_fwd(x, w, b, y, mean, rstd, EPS)
    torch.cuda.synchronize()
    assert (mean == 2.0).all() and torch.isfinite(rstd).all() and (rstd > 0).all()
    assert torch.equal(y, b.expand(M, D))


# ----------------------------------------------------------------------------------------------- softmax family
def _put(x, pitch, dev):
    """x on the device with its last dimension at a row pitch, the padding NaN."""
    buf = torch.full((*x.shape[:-1], pitch), NAN)
    buf[..., : x.shape[-1]] = x
    return buf.to(dev).contiguous()


@functools.lru_cache(maxsize=None)
def _sm_inputs(relpos, Z, Tq, Tk):
    g = torch.Generator().manual_seed(9000 + 7 * Tk + 3 * Tq + relpos)
    ac = 3.0 * torch.randn(Z, Tq, Tk, generator=g)
    P = (0, 2 * Tq - 1, Tq)[relpos]
    bd = 3.0 * torch.randn(Z, Tq, P, generator=g) if relpos else None
    dP = torch.randn(Z, Tq, Tk, generator=g)
    return ac, bd, dP


def _sm_torch(dtype, relpos, Z, Tq, Tk, nb, klen, dk, causal, keep=None, scale=1.0):
    """attn, d ac, d bd of the masked softmax of (ac + rel_shift(bd)) / sqrt(d_k) under the upstream gradient dP of
    the (dropped) probabilities; keep: the dropout mask, scale its rescale."""
    ac, bd, dP = _sm_inputs(relpos, Z, Tq, Tk)
    act = ac.to(dtype).clone().requires_grad_(True)  # (the inputs are shared: copies)
    sc, bdt = act, None
    if relpos:
        bdt = bd.to(dtype).clone().requires_grad_(True)
        shift = O.rel_shift_latest if relpos == 1 else O.rel_shift_legacy
        sc = act + shift(bdt.view(1, Z, Tq, -1))[0]
    sc = sc / math.sqrt(dk)
    kl = torch.tensor(klen)[torch.arange(Z) % nb]  # z = h * nb + b
    mask = (torch.arange(Tk)[None, None, :] < kl[:, None, None]).expand(Z, Tq, Tk)
    if causal:
        mask = mask & (torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None])[None]
    attn = torch.softmax(sc.masked_fill(~mask, torch.finfo(dtype).min), -1).masked_fill(~mask, 0.0)
    out = attn if keep is None else attn * keep.to(dtype) * scale
    out.backward(dP.to(dtype))
    return attn.detach(), act.grad, None if bdt is None else bdt.grad


@functools.lru_cache(maxsize=None)
def _sm_ref(dtype, relpos, Z, Tq, Tk, nb, klen, dk, causal):
    return _sm_torch(dtype, relpos, Z, Tq, Tk, nb, klen, dk, causal)


def _sm_fwd(dev, relpos, Z, Tq, Tk, nb, klen, dk, causal, lds=None, ldp=None, drop_p=0.0, seed=0):
    """esp_attn_softmax_fwd into NaN buffers; attn (and pdrop) as flat device buffers at pitch lds."""
    ac, bd, _ = _sm_inputs(relpos, Z, Tq, Tk)
    lds = lds or Tk
    P = bd.shape[-1] if relpos else 0
    attn = _nan(Z * Tq * lds, dev=dev)
    pdrop = _nan(Z * Tq * lds, dev=dev) if drop_p else None
    K.attn_softmax_fwd(_put(ac, lds, dev), _put(bd, ldp or P, dev) if relpos else None, relpos, P, math.sqrt(dk),
                       torch.tensor(klen, dtype=torch.int32).to(dev), nb, causal, attn, pdrop, drop_p, seed, Z, Tq, Tk,
                       lds=lds, ldp=ldp or P)
    torch.cuda.synchronize()
    return attn, pdrop


def _rows(buf, Z, Tq, pitch, n):
    return buf.view(Z, Tq, pitch)[:, :, :n]


def _plain_case(dev, Z, Tq, Tk, nb, klen, dk, causal):
    cfg = (0, Z, Tq, Tk, nb, klen, dk, causal)
    a64, ds64, _ = _sm_ref(torch.float64, *cfg)
    a32, ds32, _ = _sm_ref(torch.float32, *cfg)
    attn, _ = _sm_fwd(dev, *cfg)
    what = f"softmax Tq={Tq} Tk={Tk} klen={klen} causal={int(causal)}"
    _gate(what + " attn", attn.view(Z, Tq, Tk), a64, a32)
    dS = _nan(Z * Tq * Tk, dev=dev)
    K.attn_softmax_bwd(attn, _sm_inputs(0, Z, Tq, Tk)[2].to(dev).contiguous(), dS, 0.0, 0, math.sqrt(dk), Z * Tq, Tk)
    torch.cuda.synchronize()
    _gate(what + " dS", dS.view(Z, Tq, Tk), ds64, ds32)
    return attn.view(Z, Tq, Tk).cpu(), dS.view(Z, Tq, Tk).cpu()


@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 128, 129, 257, 513, 1024, 1025, 1100])
def test_softmax_cross_attention_every_per(dev, Tk):
    """Tq = 7 != Tk: softmax_fwd_kernel / softmax_bwd_kernel<1, 2, 4, 8, 16> at both edges of each step, and the
    loop kernels past 1024; H = 2, nb = 2 (z = h * nb + b picks the utterance's length)."""
    _plain_case(dev, 4, 7, Tk, 2, (Tk, max(1, Tk // 3)), 64, False)


def test_softmax_utterance_of_length_zero(dev):
    Z, Tq, Tk, nb = 4, 7, 130, 2
    attn, dS = _plain_case(dev, Z, Tq, Tk, nb, (Tk, 0), 64, False)
    assert (attn[1::nb] == 0).all() and (dS[1::nb] == 0).all()  # exactly 0, not NaN


@pytest.mark.parametrize("T", [65, 130])
def test_softmax_causal(dev, T):
    _plain_case(dev, 4, T, T, 2, (T, T - 23), 64, True)


@pytest.mark.parametrize("Tk", [130, 1100])
def test_softmax_in_place(dev, Tk):
    """attn may alias ac in the forward and dS may alias dP in the backward: bit-equal to the out-of-place run."""
    Z, Tq, nb, klen, dk = 4, 7, 2, (Tk, Tk // 3), 64
    ac, _, dP = _sm_inputs(0, Z, Tq, Tk)
    attn, _ = _sm_fwd(dev, 0, Z, Tq, Tk, nb, klen, dk, False)
    buf = ac.to(dev).contiguous()
    K.attn_softmax_fwd(buf, None, 0, 0, math.sqrt(dk), torch.tensor(klen, dtype=torch.int32).to(dev), nb, False, buf,
                       None, 0.0, 0, Z, Tq, Tk)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(-1), attn)
    dS = _nan(Z * Tq * Tk, dev=dev)
    K.attn_softmax_bwd(attn, dP.to(dev).contiguous(), dS, 0.0, 0, math.sqrt(dk), Z * Tq, Tk)
    g = dP.to(dev).contiguous()
    K.attn_softmax_bwd(attn, g, g, 0.0, 0, math.sqrt(dk), Z * Tq, Tk)
    torch.cuda.synchronize()
    assert not torch.isnan(dS).any() and torch.equal(g.view(-1), dS)


@pytest.mark.parametrize("Tk", [130, 513, 1100])
def test_softmax_dropout_masks_of_forward_and_backward_agree(dev, Tk):
    """p = 0.5 (exact on the kernels' 1/65536 grid: rescale 2): the kept elements of pdrop are attn * 2, about half
    are kept, and the backward with the same seed is the fp64 backward under the mask read back from the forward --
    both draw element row * Tk + j, at PER 4, 16 and in the loop kernels.  The rows lie at a pitch of Tk + 5 (padding
    NaN), so an index taken from the pitch instead of the row length would show."""
    Z, Tq, nb, klen, dk, p, seed = 4, 7, 2, (Tk, Tk), 64, 0.5, 4242
    cfg = (0, Z, Tq, Tk, nb, klen, dk, False)
    lds = Tk + 5
    attn, pdrop = _sm_fwd(dev, *cfg, lds=lds, drop_p=p, seed=seed)
    a, pd = _rows(attn, Z, Tq, lds, Tk).cpu(), _rows(pdrop, Z, Tq, lds, Tk).cpu()
    assert not torch.isnan(pd).any() and (a > 0).all()
    assert torch.isnan(attn.view(Z, Tq, lds)[:, :, Tk:]).all() and torch.isnan(pdrop.view(Z, Tq, lds)[:, :, Tk:]).all()
    keep = pd != 0
    assert torch.equal(pd[keep], a[keep] * 2.0)
    n = keep.numel()
    assert abs(int(keep.sum()) - n / 2) <= 5 * math.sqrt(n) / 2, (int(keep.sum()), n)
    dS = _nan(Z * Tq * lds, dev=dev)
    K.attn_softmax_bwd(attn, _put(_sm_inputs(*cfg[:4])[2], lds, dev), dS, p, seed, math.sqrt(dk), Z * Tq, Tk, lds=lds)
    torch.cuda.synchronize()
    _, ds64, _ = _sm_torch(torch.float64, *cfg, keep=keep, scale=2.0)
    _, ds32, _ = _sm_torch(torch.float32, *cfg, keep=keep, scale=2.0)
    _gate(f"softmax dropout Tk={Tk} dS", _rows(dS, Z, Tq, lds, Tk), ds64, ds32)
    assert torch.isnan(dS.view(Z, Tq, lds)[:, :, Tk:]).all()


def _relpos_case(dev, T, legacy, padded, dk):
    Z, nb = 2, 2
    relpos = 2 if legacy else 1
    P = T if legacy else 2 * T - 1
    klen = (T, max(1, T // 3))
    cfg = (relpos, Z, T, T, nb, klen, dk, False)
    a64, ds64, dbd64 = _sm_ref(torch.float64, *cfg)
    a32, ds32, dbd32 = _sm_ref(torch.float32, *cfg)
    Tp, Pp = (K.pitch(T) + 4, K.pitch(P) + 4) if padded else (T, P)
    what = f"relpos {'legacy' if legacy else 'latest'} T={T} pitch={Tp}/{Pp} dk={dk}"
    attn, _ = _sm_fwd(dev, *cfg, lds=Tp, ldp=Pp)
    _gate(what + " attn", _rows(attn, Z, T, Tp, T), a64, a32)
    dP = _put(_sm_inputs(relpos, Z, T, T)[2], Tp, dev)
    dS, dbd = _nan(Z * T * Tp, dev=dev), _nan(Z * T * Pp, dev=dev)
    K.attn_softmax_bwd_relpos(attn, dP, dS, dbd, Pp, 0.0, 0, math.sqrt(dk), Z * T, T, Tp, relpos=relpos)
    torch.cuda.synchronize()
    _gate(what + " dS", _rows(dS, Z, T, Tp, T), ds64, ds32)
    got = _rows(dbd, Z, T, Pp, P).cpu()
    _gate(what + " dbd", got, dbd64, dbd32)
    assert (got[dbd64 == 0] == 0).all(), (what, "the zeros of the rel_shift adjoint")
    if padded:
        assert torch.isnan(dbd.view(Z, T, Pp)[:, :, P:]).all(), (what, "dbd's padding columns were written")
    dbd2 = _nan(Z * T * Pp, dev=dev)
    K.relshift_bwd(dS, dbd2, relpos, Z, T, P, lds=Tp, ldp=Pp)
    torch.cuda.synchronize()
    assert torch.equal(_rows(dbd2, Z, T, Pp, P), _rows(dbd, Z, T, Pp, P)), (what, "relshift_bwd on the same dS")


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("legacy", [False, True], ids=["latest", "legacy"])
@pytest.mark.parametrize("T", [65, 129, 257, 513, 1024, 1025])
def test_softmax_bwd_relpos_every_instantiation(dev, T, legacy, padded):
    """Tight pitch (lds = T, ldp = P): softmax_bwd_relpos_kernel<2, 4, 8, 16, REL> for the odd T (T = 1024 is a
    multiple of 4: the aligned kernel); padded pitch: softmax_bwd_relpos4_kernel<1, 2, 4, REL, pow2>, T = 1024 its
    last length; T = 1025: softmax_bwd_loop_kernel<REL> in both layouts."""
    _relpos_case(dev, T, legacy, padded, 64)


@pytest.mark.parametrize("legacy", [False, True], ids=["latest", "legacy"])
@pytest.mark.parametrize("T", [65, 257, 1024])
def test_softmax_bwd_relpos_sqrt_dk_not_a_power_of_two(dev, T, legacy):
    """d_k = 20: softmax_bwd_relpos4_kernel<1, 2, 4, REL, false> divides by sqrt(d_k) instead of multiplying by its
    exact reciprocal."""
    _relpos_case(dev, T, legacy, True, 20)


@pytest.mark.parametrize("dk", [64, 20])
@pytest.mark.parametrize("T", [65, 257, 513, 1024])
def test_softmax_bwd_relpos_band_writes_the_band_only(dev, T, dk):
    """softmax_bwd_relpos4_kernel<1, 2, 4, 3, pow2>: into a buffer of 7.0 the band (row i: columns T-1-i .. 2T-2-i)
    becomes the fp64 gradient and every other element, padding included, is still exactly 7.0."""
    Z, nb, P = 2, 2, 2 * T - 1
    cfg = (1, Z, T, T, nb, (T, max(1, T // 3)), dk, False)
    _, ds64, dbd64 = _sm_ref(torch.float64, *cfg)
    _, ds32, dbd32 = _sm_ref(torch.float32, *cfg)
    Tp, Pp = K.pitch(T) + 4, K.pitch(P) + 4
    attn, _ = _sm_fwd(dev, *cfg, lds=Tp, ldp=Pp)
    dP = _put(_sm_inputs(1, Z, T, T)[2], Tp, dev)
    dS = _nan(Z * T * Tp, dev=dev)
    dbd = torch.full((Z * T * Pp,), 7.0, device=dev)
    K.attn_softmax_bwd_relpos_band(attn, dP, dS, dbd, Pp, 0.0, 0, math.sqrt(dk), Z * T, T, Tp)
    torch.cuda.synchronize()
    what = f"relpos band T={T} dk={dk}"
    _gate(what + " dS", _rows(dS, Z, T, Tp, T), ds64, ds32)
    k = torch.arange(Pp)[None, :] - (T - 1 - torch.arange(T))[:, None]
    band = ((k >= 0) & (k < T))[None].expand(Z, T, Pp)
    got = dbd.view(Z, T, Pp).cpu()
    assert (got[~band] == 7.0).all(), (what, "an element outside the band was written")
    full = torch.zeros(Z, T, Pp, dtype=torch.float64)
    full[:, :, :P] = dbd64
    full32 = torch.zeros(Z, T, Pp)
    full32[:, :, :P] = dbd32
    _gate(what + " dbd band", got[band], full[band], full32[band])
