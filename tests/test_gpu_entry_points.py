"""First direct tests of ten exported entry points that were reached only through module and model tests:
esp_bn_swish_eval, esp_heads_split, esp_heads_split2, esp_add2d, esp_im2col_nhwc, esp_col2im_relu_nhwc, esp_embed_fwd,
esp_cache_gather, esp_scale_by_dev, esp_ctc_prefix_score_batch -- at pitches and column offsets, float4 tails,
out-of-range indices that must be skipped, padding that must stay untouched, ragged lengths.  And of seven more that
tests/test_kernel_coverage_cpu.py found beside them: esp_adam_amsgrad, esp_adam_dev, esp_adam_dev_amsgrad,
esp_opt_hyper, esp_opt_advance, esp_rng_advance, esp_global_mvn.

Floating-point results: reference plain torch on the CPU in fp64, yardstick the same code in fp32; per output tensor,
e(a) = max|a - ref64| / max|ref64|, e(ours) <= max(2 e(torch fp32), 1e-5), both printed (GATE lines).  Pure data
movement (copies, gathers, a single add or multiply) is torch.equal with torch fp32.  Output buffers are NaN or a
stated sentinel on entry (esp_ctc_prefix_score_batch's are allocated by its wrapper: every element is compared).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd._native import NativeError
from oracle import ctc_np
from tests.helpers import keep_scale

pytestmark = pytest.mark.gpu

FLOOR = 1e-5
NAN = float("nan")
SENTINEL = 7.0


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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------- bn_swish_eval
@pytest.mark.parametrize("D", [1, 30, 64, 257])
@pytest.mark.parametrize("M", [0, 1, 37])
def test_bn_swish_eval(dev, M, D):
    """s = z sigmoid(z), z = (y - rm) / sqrt(rv + eps) gamma + beta; D = 257: a second block of bn_running_kernel;
    M = 0 writes mean and rstd and leaves s untouched."""
    g, eps = _gen(100 + D), 1e-5
    y = 2.0 * torch.randn(M, D, generator=g) + 0.5
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    rm, rv = 0.5 * torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
    s = torch.full((max(M, 3), D), NAN, device=dev)
    mean, rstd = torch.full((D,), NAN, device=dev), torch.full((D,), NAN, device=dev)
    K.bn_swish_eval(y.to(dev), gamma.to(dev), beta.to(dev), s, rm.to(dev), rv.to(dev), mean, rstd, eps=eps)
    torch.cuda.synchronize()

    def ref(dt):
        rs = 1.0 / torch.sqrt(rv.to(dt) + eps)
        z = (y.to(dt) - rm.to(dt)) * rs * gamma.to(dt) + beta.to(dt)
        return z * torch.sigmoid(z), rs
    (s64, r64), (s32, r32) = ref(torch.float64), ref(torch.float32)
    assert torch.equal(mean.cpu(), rm)
    _gate(f"bn_swish_eval M={M} D={D} rstd", rstd, r64, r32)
    if M:
        _gate(f"bn_swish_eval M={M} D={D} s", s[:M], s64, s32)
    assert torch.isnan(s[M:]).all()


# ----------------------------------------------------------------------------------------------- heads_split
def _heads_src(B, T, H, dk, seed):
    ld = 3 * H * dk + 8
    g = _gen(seed)
    return torch.randn(B * T, ld, generator=g), torch.randn(H * dk, generator=g), torch.randn(H * dk, generator=g), ld


def _heads_ref(src, col0, B, T, H, dk, bias):
    v = src[:, col0:col0 + H * dk].reshape(B, T, H, dk).permute(2, 0, 1, 3)
    return (v + bias.view(H, 1, 1, dk) if bias is not None else v).contiguous()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dk", [7, 20, 64])
@pytest.mark.parametrize("part", [0, 1, 2])
def test_heads_split(dev, part, dk, with_bias):
    B, T, H = 3, 5, 3
    src, bias, _, ld = _heads_src(B, T, H, dk, 200 + dk)
    col0 = part * H * dk
    dst = torch.full((H, B, T, dk), NAN, device=dev)
    K.heads_split(src.to(dev), ld, col0, B, T, H, dk, bias.to(dev) if with_bias else None, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), _heads_ref(src, col0, B, T, H, dk, bias if with_bias else None))


@pytest.mark.parametrize("dk", [4, 20, 64])
@pytest.mark.parametrize("part", [0, 1, 2])
def test_heads_split2(dev, part, dk):
    B, T, H = 3, 5, 3
    src, ba, bb, ld = _heads_src(B, T, H, dk, 300 + dk)
    col0 = part * H * dk
    da, db = torch.full((H, B, T, dk), NAN, device=dev), torch.full((H, B, T, dk), NAN, device=dev)
    K.heads_split2(src.to(dev), ld, col0, B, T, H, dk, ba.to(dev), da, bb.to(dev), db)
    torch.cuda.synchronize()
    assert torch.equal(da.cpu(), _heads_ref(src, col0, B, T, H, dk, ba))
    assert torch.equal(db.cpu(), _heads_ref(src, col0, B, T, H, dk, bb))


@pytest.mark.parametrize("dk,col0,ldpad", [(6, 0, 8), (4, 2, 8), (4, 0, 6)],
                         ids=["dk_not_x4", "col0_not_x4", "ld_not_x4"])
def test_heads_split2_rejects_unaligned(dev, dk, col0, ldpad):
    B, T, H = 3, 5, 3
    ld = 3 * H * dk + ldpad
    src = torch.zeros(B * T, ld, device=dev)
    b = torch.zeros(H * dk, device=dev)
    da, db = torch.full((H, B, T, dk), NAN, device=dev), torch.full((H, B, T, dk), NAN, device=dev)
    with pytest.raises(NativeError):
        K.heads_split2(src, ld, col0, B, T, H, dk, b, da, b, db)
    torch.cuda.synchronize()
    assert torch.isnan(da).all() and torch.isnan(db).all()


# ----------------------------------------------------------------------------------------------- add2d
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("M,N,ldx,ldy", [(1, 1, 1, 1), (37, 30, 33, 40), (300, 256, 256, 768)])
def test_add2d(dev, M, N, ldx, ldy, shifted):
    """y[:, c0:c0+N] += x[:, x0:x0+N] on pitched rows: column 0 (the q block of a fused qkv gradient, as the rel-pos
    attention backward adds dq_v) or the last N columns; every other column of y keeps its sentinel."""
    g = _gen(400 + M)
    x_off, y_off = (ldx - N, ldy - N) if shifted else (0, 0)
    x = torch.randn(M, ldx, generator=g)
    y = torch.full((M, ldy), SENTINEL)
    y[:, y_off:y_off + N] = torch.randn(M, N, generator=g)
    want = y.clone()
    want[:, y_off:y_off + N] += x[:, x_off:x_off + N]
    yd = y.to(dev)
    K.add2d(x.to(dev), ldx, yd, ldy, M, N, x_off=x_off, y_off=y_off)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), want)


# ----------------------------------------------------------------------------------------------- NHWC columns
def _unfold_rows(x_nhwc, k, s):
    """F.unfold of the NCHW image, rows (b, t2, f2), columns reordered from (c, kt, kf) to (kt, kf, c)."""
    B, T1, F1, C = x_nhwc.shape
    T2, F2 = (T1 - k) // s + 1, (F1 - k) // s + 1
    u = F.unfold(x_nhwc.permute(0, 3, 1, 2), k, stride=s)  # (B, C k k, T2 F2)
    return u.view(B, C, k, k, T2, F2).permute(0, 4, 5, 2, 3, 1).reshape(B * T2 * F2, k * k * C).contiguous()


def _fold_rows(dcol, B, T1, F1, C, k, s):
    """The adjoint of _unfold_rows (F.fold), as an NHWC image."""
    T2, F2 = (T1 - k) // s + 1, (F1 - k) // s + 1
    u = dcol.view(B, T2, F2, k, k, C).permute(0, 5, 3, 4, 1, 2).reshape(B, C * k * k, T2 * F2)
    return F.fold(u, (T1, F1), k, stride=s).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("size", ["kernel", (17, 13), (20, 16)], ids=["k_x_k", "17x13", "20x16"])
@pytest.mark.parametrize("C", [4, 12, 64])
@pytest.mark.parametrize("k,s", [(5, 3), (3, 2)])
def test_im2col_and_col2im_relu_nhwc(dev, k, s, C, size):
    """(T1 - k) % s != 0 in some: trailing rows / columns belong to no window (their dx is exactly 0)."""
    B = 2
    T1, F1 = (k, k) if size == "kernel" else size
    T2, F2 = (T1 - k) // s + 1, (F1 - k) // s + 1
    g = _gen(500 + 10 * k + C + T1)
    x = torch.randn(B, T1, F1, C, generator=g)
    col = torch.full((B * T2 * F2, k * k * C), NAN, device=dev)
    K.im2col_nhwc(x.to(dev), col, B, T1, F1, C, k, s)
    torch.cuda.synchronize()
    assert torch.equal(col.cpu(), _unfold_rows(x, k, s))

    dcol = torch.randn(B * T2 * F2, k * k * C, generator=g)
    z = torch.randn(B, T1, F1, C, generator=g)
    z.view(-1)[::7] = 0.0  # z == 0: no gradient
    dx = torch.full((B, T1, F1, C), NAN, device=dev)
    K.col2im_relu_nhwc(dcol.to(dev), z.to(dev), dx, B, T1, F1, C, k, s)
    torch.cuda.synchronize()
    r64 = _fold_rows(dcol.double(), B, T1, F1, C, k, s) * (z > 0)
    r32 = _fold_rows(dcol, B, T1, F1, C, k, s) * (z > 0)
    _gate(f"col2im_relu_nhwc k={k} s={s} C={C} {T1}x{F1}", dx, r64, r32)
    got = dx.cpu()
    assert (got[z <= 0] == 0).all()
    tr, fr = s * (T2 - 1) + k, s * (F2 - 1) + k  # rows / columns from here on belong to no window
    assert (got[:, tr:] == 0).all() and (got[:, :, fr:] == 0).all()


def test_nhwc_columns_reject_channels_not_x4(dev):
    B, T1, F1, C, k, s = 2, 8, 8, 6, 3, 2
    x = torch.zeros(B, T1, F1, C, device=dev)
    col = torch.full((B * 3 * 3, k * k * C), NAN, device=dev)
    with pytest.raises(NativeError):
        K.im2col_nhwc(x, col, B, T1, F1, C, k, s)
    dx = torch.full((B, T1, F1, C), NAN, device=dev)
    with pytest.raises(NativeError):
        K.col2im_relu_nhwc(torch.zeros_like(col), x, dx, B, T1, F1, C, k, s)
    torch.cuda.synchronize()
    assert torch.isnan(col).all() and torch.isnan(dx).all()


# ----------------------------------------------------------------------------------------------- embed_fwd
def _embed_inputs(D, L, seed):
    B, V = 3, 40  # more tokens than rows: some embedding rows are never looked up
    g = _gen(seed)
    tok = torch.randint(0, V, (B * L,), generator=g)
    tok[0], tok[-1] = 0, V - 1
    if B * L > 3:
        tok[1] = tok[2] = V - 1  # repeats
    E = torch.randn(V, D, generator=g)
    E = torch.where(E.abs() < 0.05, torch.full_like(E, 0.05), E)  # no zeros
    pe = torch.randn(L, D, generator=g)
    return tok, E, pe, V


@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("D", [5, 256, 1024])
def test_embed_fwd(dev, D, L):
    tok, E, pe, V = _embed_inputs(D, L, 600 + D + L)
    n, xscale = tok.numel(), math.sqrt(D)
    y = torch.full((n, D), NAN, device=dev)
    K.embed_fwd(tok.to(dev), E.to(dev), pe.to(dev), y, L, xscale, 0.0, 0)
    torch.cuda.synchronize()
    pos = torch.arange(n) % L
    _gate(f"embed_fwd D={D} L={L}", y, E.double()[tok] * xscale + pe.double()[pos],
          E[tok] * torch.tensor(xscale, dtype=torch.float32) + pe[pos])


@pytest.mark.parametrize("D", [5, 256, 1024])
def test_embed_dropout_mask_of_forward_and_backward_agree(dev, D):
    """p = 0.3, pe = 0, E without zeros: the forward's mask is y != 0; esp_embed_bwd with the same seed on dy = 1 must
    give, per (v, d), xscale * scale * (the kept rows with tok == v) under that mask -- both draw element
    row * D + d.  scale is read from a kept element of y; dE is accumulated (non-zero on entry)."""
    L, p, seed = 7, 0.3, 777
    tok, E, _, V = _embed_inputs(D, L, 650 + D)
    n, xscale = tok.numel(), math.sqrt(D)
    y = torch.full((n, D), NAN, device=dev)
    K.embed_fwd(tok.to(dev), E.to(dev), torch.zeros(L, D, device=dev), y, L, xscale, p, seed)
    torch.cuda.synchronize()
    yc = y.cpu()
    assert not torch.isnan(yc).any()
    keep = yc != 0
    assert 0 < int(keep.sum()) < keep.numel()
    r, d = [int(i) for i in keep.nonzero()[0]]
    scale = float(yc[r, d].double() / (E[tok[r], d].double() * xscale))
    assert abs(scale - keep_scale(p)) <= 1e-6 * keep_scale(p)
    _gate(f"embed_fwd dropout D={D} y", y, E.double()[tok] * xscale * scale * keep,
          E[tok] * torch.tensor(xscale, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32) * keep)
    dE0 = torch.randn(V, D, generator=_gen(660 + D))
    dE = dE0.to(dev)
    K.embed_bwd(tok.to(dev), torch.ones(n, D, device=dev), dE, xscale, p, seed)
    torch.cuda.synchronize()
    count = torch.zeros(V, D, dtype=torch.float64).index_add_(0, tok, keep.double())
    want64 = dE0.double() + xscale * scale * count
    want32 = dE0 + (torch.tensor(xscale * scale, dtype=torch.float32) * count.float())
    _gate(f"embed_bwd dropout D={D} dE", dE, want64, want32)
    unused = torch.ones(V, dtype=torch.bool)
    unused[tok] = False
    assert unused.any() and torch.equal(dE.cpu()[unused], dE0[unused])


# ----------------------------------------------------------------------------------------------- cache_gather
def _cache(W, dev, seed):
    NL = 2
    src = torch.randn(NL, 6, 9, W, generator=_gen(seed))
    return src, torch.full((NL, 5, 11, W), SENTINEL, device=dev)


@pytest.mark.parametrize("n", [5, 3])
@pytest.mark.parametrize("length", [0, 1, 9])
@pytest.mark.parametrize("W", [4, 128])
def test_cache_gather(dev, W, length, n):
    """index holds a repeat and two entries outside [0, src_n): their rows, the positions >= length and the
    destination rows >= n (n = 3) keep the sentinel."""
    src, dst = _cache(W, dev, 700 + W)
    index, src_n = [3, 0, 3, -1, 4][:n], 4
    K.cache_gather(src.to(dev), dst, torch.tensor(index, dtype=torch.int64, device=dev), n, length, src_n)
    torch.cuda.synchronize()
    want = torch.full((2, 5, 11, W), SENTINEL)
    for i, s in enumerate(index):
        if 0 <= s < src_n:
            want[:, i, :length] = src[:, s, :length]
    assert torch.equal(dst.cpu(), want)


def test_cache_gather_rejects_bad_arguments(dev):
    index = torch.tensor([3, 0, 3, -1, 4], dtype=torch.int64, device=dev)
    src, dst = _cache(6, dev, 1)  # W no multiple of 4
    with pytest.raises(NativeError):
        K.cache_gather(src.to(dev), dst, index, 5, 1, 4)
    src, dst = _cache(4, dev, 2)
    srcd = src.to(dev)
    with pytest.raises(NativeError):  # src is dst
        K.cache_gather(srcd, srcd, index, 5, 1, 4)
    with pytest.raises(NativeError):  # more rows than dst holds
        K.cache_gather(srcd, dst, torch.zeros(6, dtype=torch.int64, device=dev), 6, 1, 4)
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all() and torch.equal(srcd.cpu(), src)


# ----------------------------------------------------------------------------------------------- scale_by_dev
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_scale_by_dev(dev, n):
    x = torch.randn(n, generator=_gen(800 + n))
    s = torch.tensor([0.37], dtype=torch.float32)
    xd = x.to(dev)
    K.scale_by_dev(xd, s.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x * s)


# ----------------------------------------------------------------------------------------------- CTC prefix scores
LOGZERO = float(ctc_np.LOGZERO)


def _oracle_step(lp, y, cs, r_prev, blank, eos):
    """ctc_np.ctc_prefix_score_np on one utterance's frames.  Past its domain -- a prefix with more labels than the
    utterance has frames, whose recursion would start beyond the last frame -- the recursion runs over no frame:
    the states are logzero, psi is logzero but for <eos> (the prefix's own total, r_sum[-1]) and blank."""
    T, n_out, cs = lp.shape[0], len(y) - 1, np.asarray(cs)
    if max(n_out, 1) - 1 < T:
        return ctc_np.ctc_prefix_score_np(lp, y, cs, r_prev, blank, eos)
    psi = np.full(len(cs), ctc_np.LOGZERO, dtype=np.float32)
    psi[cs == eos] = np.logaddexp(r_prev[-1, 0], r_prev[-1, 1])
    psi[cs == blank] = ctc_np.LOGZERO
    return psi, np.full((len(cs), T, 2), ctc_np.LOGZERO, dtype=np.float32)


@pytest.mark.parametrize("out_len", [0, 1, 4])
def test_ctc_prefix_score_batch_ragged(dev, out_len):
    """U = 3 utterances of 57, 23 and 1 frames (frames at and past the length are NaN: they must not be read),
    NH = 7 hypotheses x C = 11 candidates (77 threads: two blocks, the last partial); prefixes of out_len labels,
    their states by successive oracle calls."""
    rng = np.random.RandomState(11 + out_len)
    U, Tmax, V, NH, C, blank = 3, 57, 20, 7, 11, 0
    eos = V - 1
    tlen = [57, 23, 1]
    lps = [torch.log_softmax(torch.tensor(rng.randn(t, V) * 3, dtype=torch.float32), -1).numpy() for t in tlen]
    lp = np.full((U, Tmax, V), np.nan, dtype=np.float32)
    for u in range(U):
        lp[u, :tlen[u]] = lps[u]
    utt = [h % U for h in range(NH)]
    prefixes = [[eos] + [int(v) for v in rng.randint(1, V - 1, out_len)] for _ in range(NH)]
    if out_len >= 2:
        prefixes[1][-1] = prefixes[1][-2]  # a repeated label
    states = []
    for h, y in enumerate(prefixes):
        r = ctc_np.ctc_prefix_init_np(lps[utt[h]], blank)
        for k in range(1, len(y)):
            _, rs = _oracle_step(lps[utt[h]], y[:k], [y[k]], r, blank, eos)
            r = rs[0]
        states.append(r)
    r_prev = np.full((NH, Tmax, 2), ctc_np.LOGZERO, dtype=np.float32)
    for h in range(NH):
        r_prev[h, :tlen[utt[h]]] = states[h]
    cands = np.stack([rng.choice(V, C, replace=False) for _ in range(NH)]).astype(np.int64)
    cands[:, 0], cands[:, 1] = blank, eos
    cands[:, 2] = [y[-1] for y in prefixes]  # the hypothesis's last label
    last = torch.tensor([y[-1] for y in prefixes], dtype=torch.int64, device=dev)
    lpd, rpd = torch.tensor(lp, device=dev), torch.tensor(r_prev, device=dev)
    tld = torch.tensor(tlen, dtype=torch.int32, device=dev)

    def run(utt_, cands_):
        psi, rs = K.ctc_prefix_score_batch(lpd, tld, torch.tensor(utt_, dtype=torch.int32, device=dev), rpd, last,
                                           out_len, torch.tensor(cands_, device=dev), blank, eos)
        torch.cuda.synchronize()
        return psi.cpu().numpy(), rs.cpu().numpy()
    psi, rs = run(utt, cands)
    assert not np.isnan(psi).any() and not np.isnan(rs).any()
    start = max(out_len, 1) - 1
    for h, y in enumerate(prefixes):
        tl = tlen[utt[h]]
        want_psi, want_r = _oracle_step(lps[utt[h]], y, cands[h], states[h], blank, eos)
        np.testing.assert_allclose(psi[h], want_psi, rtol=0, atol=1e-4, err_msg=f"psi of hypothesis {h}")
        if start < tl:
            np.testing.assert_allclose(rs[h, :, start:tl], want_r[:, start:tl], rtol=0, atol=1e-4,
                                       err_msg=f"states of hypothesis {h}")
        assert (rs[h, :, tl:] == LOGZERO).all(), f"hypothesis {h}: state rows past the utterance's length"
        if out_len <= tl:  # esp_ctc_prefix_score on the utterance's own frames: the same recursion
            one, _ = K.ctc_prefix_score(torch.tensor(lps[utt[h]], device=dev), rpd[h:h + 1, :tl].contiguous(),
                                        last[h:h + 1], out_len, torch.tensor(cands[h:h + 1], device=dev), blank, eos)
            assert np.array_equal(one.cpu().numpy()[0], psi[h]), f"hypothesis {h} vs esp_ctc_prefix_score"

    # labels and utterance indices out of range score logzero and read nothing; the others are unchanged
    cands2, utt2 = cands.copy(), list(utt)
    cands2[0, 3], cands2[1, 4] = -1, V
    utt2[3], utt2[4] = -1, U
    psi2, rs2 = run(utt2, cands2)
    assert not np.isnan(psi2).any() and not np.isnan(rs2).any()
    dead = np.zeros((NH, C), dtype=bool)
    dead[0, 3] = dead[1, 4] = True
    dead[3], dead[4] = True, True
    assert (psi2[dead] == LOGZERO).all() and (rs2[dead] == LOGZERO).all()
    assert np.array_equal(psi2[~dead], psi[~dead]) and np.array_equal(rs2[~dead], rs[~dead])


# ----------------------------------------------------------------------------------------------- optimizer, RNG, MVN
# (found by tests/test_kernel_coverage_cpu.py beside the ten above: reached only through FusedAdam, the trainer and
# GlobalMVN until now)
def _adam_torch(dt, p, g, m, v, vmax, coef, lr, b1, b2, eps, wd, step):
    """One torch.optim.Adam step (L2 weight decay in the gradient) on the clipped gradient, in dt."""
    p, g, m, v = p.to(dt), g.to(dt) * coef, m.to(dt), v.to(dt)
    if wd:
        g = g + wd * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    vd = v
    if vmax is not None:
        vd = vmax = torch.maximum(vmax.to(dt), v)
    denom = vd.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * (m / denom), m, v, vmax


@pytest.mark.parametrize("n", [1, 1023, 70001])
@pytest.mark.parametrize("form", ["amsgrad", "dev", "dev_amsgrad"])
def test_adam_forms(dev, form, n):
    """esp_adam_amsgrad (host step count), esp_adam_dev / esp_adam_dev_amsgrad (lr and bias corrections from
    esp_opt_hyper's device triple) at step 3, clip coefficient 0.5, weight decay; a zero finite flag leaves every
    buffer as it was."""
    g_ = _gen(900 + n)
    p, g, m = torch.randn(n, generator=g_), torch.randn(n, generator=g_), 0.1 * torch.randn(n, generator=g_)
    v = 0.01 * torch.rand(n, generator=g_)
    ams = form.endswith("amsgrad")
    vmax = 0.01 * torch.rand(n, generator=g_) if ams else None  # above v in places, below in others
    lr, b1, b2, eps, wd, step, coef = 2e-3, 0.9, 0.98, 1e-9, 1e-2, 3, 0.5

    def run(flag):
        bufs = [t.to(dev) for t in (p, g, m, v)] + ([vmax.to(dev)] if ams else [])
        clip = torch.tensor([1.0, coef, flag], device=dev)
        if form == "amsgrad":
            K.adam_amsgrad(*bufs, clip, lr, b1, b2, eps, wd, step)
        else:
            hyper = torch.full((3,), NAN, device=dev)
            K.opt_hyper(torch.tensor([step - 1.0, 0.0], dtype=torch.float64, device=dev), lr, 0.0, b1, b2, hyper)
            if ams:
                K.adam_dev_amsgrad(*bufs, clip, hyper, b1, b2, eps, wd)
            else:
                K.adam_dev(*bufs, clip, hyper, b1, b2, eps, wd)
        torch.cuda.synchronize()
        return [t.cpu() for t in bufs]
    same = run(0.0)
    for got, was in zip(same, (p, g, m, v, vmax)):
        assert torch.equal(got, was)
    out = run(1.0)
    r64 = _adam_torch(torch.float64, p, g, m, v, vmax, coef, lr, b1, b2, eps, wd, step)
    r32 = _adam_torch(torch.float32, p, g, m, v, vmax, coef, lr, b1, b2, eps, wd, step)
    assert torch.equal(out[1], g)
    for name, got, a, b in zip(("p", "m", "v", "vmax"), [out[0]] + out[2:], r64, r32):
        _gate(f"adam {form} n={n} {name}", got, a, b)


@pytest.mark.parametrize("warmup", [0.0, 25000.0])
@pytest.mark.parametrize("steps", [(0.0, 0.0), (6.0, 4.0), (30000.0, 29990.0)])
def test_opt_hyper_and_advance(dev, steps, warmup):
    """esp_opt_hyper: {lr of WarmupLR at scheduler step s + 1, 1 - b1^(t+1), sqrt(1 - b2^(t+1))} from the device
    state (t, s), each the fp32 rounding of a double (1 ulp of fp32 allowed: the device's pow is not libm's);
    esp_opt_advance: both counters + 1 unless the step was skipped (finite flag 0)."""
    base, b1, b2 = 2e-3, 0.9, 0.98
    state = torch.tensor(steps, dtype=torch.float64, device=dev)
    hyper = torch.full((3,), NAN, device=dev)
    K.opt_hyper(state, base, warmup, b1, b2, hyper)
    torch.cuda.synchronize()
    t, s = steps[0] + 1, steps[1] + 1
    lr = base * math.sqrt(warmup) * min(1 / math.sqrt(s), s * warmup ** -1.5) if warmup else base
    want = np.array([lr, 1 - b1 ** t, math.sqrt(1 - b2 ** t)])
    np.testing.assert_allclose(hyper.cpu().numpy().astype(np.float64), want, rtol=2.0 ** -23, atol=0)
    K.opt_advance(state, torch.tensor([1.0, 1.0, 0.0], device=dev))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == list(steps)
    K.opt_advance(state, torch.tensor([1.0, 1.0, 1.0], device=dev))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [t, s]


def test_rng_advance_is_splitmix64(dev):
    M = (1 << 64) - 1
    for k0 in (0, 1, 0x0123456789ABCDEF, (1 << 62) - 1):
        key = torch.tensor([k0], dtype=torch.int64, device=dev)
        want = k0
        for _ in range(3):
            K.rng_advance(key)
            z = (want + 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            want = z ^ (z >> 31)
        torch.cuda.synchronize()
        assert int(key.cpu().item()) & M == want


@pytest.mark.parametrize("norm_means,norm_vars", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("B,T,Fd", [(1, 1, 1), (3, 37, 80), (2, 300, 83)])
def test_global_mvn(dev, B, T, Fd, norm_means, norm_vars):
    """In place ((x - mean), frames t >= len zeroed) / std, ragged lengths including 0 and T."""
    g = _gen(950 + T)
    x = 3.0 * torch.randn(B, T, Fd, generator=g) + 1.0
    mean, std = torch.randn(Fd, generator=g), 0.5 + torch.rand(Fd, generator=g)
    lens = torch.tensor([T, T // 3, 0][:B], dtype=torch.int32)
    xd = x.to(dev)
    K.global_mvn(xd, lens.to(dev), mean.to(dev), std.to(dev), norm_means, norm_vars)
    torch.cuda.synchronize()

    def ref(dt):
        y = x.to(dt) - mean.to(dt) if norm_means else x.to(dt)
        y = y * (torch.arange(T)[None, :, None] < lens[:, None, None])
        return y / std.to(dt) if norm_vars else y
    _gate(f"global_mvn {B}x{T}x{Fd} means={int(norm_means)} vars={int(norm_vars)}", xd, ref(torch.float64),
          ref(torch.float32))
    pad = (torch.arange(T)[None, :] >= lens[:, None])
    assert (xd.cpu()[pad] == 0).all()
