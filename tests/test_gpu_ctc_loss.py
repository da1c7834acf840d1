"""The CTC loss kernels and their neighbours in a training step, each against torch on the CPU in fp64.

K.log_softmax + K.ctc_loss (as asr/ctc.py calls them) against torch.nn.functional.ctc_loss (reduction none,
zero_infinity, blank 0) differentiated through log_softmax with the cotangent gscale per utterance, at the
shapes the model fixtures never reach: more than 256 CTC states (several states per thread), the 1023-state
limit, targets that fit their frames without slack, T = 1, empty targets and inputs, V at the shared-memory
limit, log-probabilities hundreds of nats apart, and repeat runs.  The gate is the project's usual one:
err(ours vs fp64) <= max(2 * err(fp32 torch vs fp64), floor), floors 1e-4 on nll and 1e-5 on the gradient
(those of test_ctc_against_golden_and_numpy).  log_softmax, label_smoothing and reduce_losses follow.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd._native import NativeError
from oracle import espnet_cpu as O
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

NLL_FLOOR, GRAD_FLOOR = 1e-4, 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pad(rows, Umax):
    y = torch.zeros(len(rows), max(Umax, 1), dtype=torch.int64)
    for b, r in enumerate(rows):
        y[b, : len(r)] = torch.as_tensor(r, dtype=torch.int64)
    return y


def _feasible(rows, ilens):
    """ilen >= U + adjacent repeats, per row"""
    return [il >= len(r) + sum(1 for a, b in zip(r[:-1], r[1:]) if a == b) for r, il in zip(rows, ilens)]


def _ref(x, rows, ilens, gscale, dtype):
    """(nll with inf kept, gradient w.r.t. the logits) of torch's CPU ctc_loss in `dtype`; x (B, T, V)"""
    B = x.shape[0]
    Umax = max(len(r) for r in rows)
    y, il, tl = _pad(rows, Umax), torch.tensor(ilens), torch.tensor([len(r) for r in rows])
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    lp = torch.log_softmax(xx, -1).transpose(0, 1)  # (T, B, V)
    loss = F.ctc_loss(lp, y, il, tl, blank=0, reduction="none", zero_infinity=True)
    loss.backward(torch.full((B,), gscale, dtype=dtype))
    with torch.no_grad():
        raw = F.ctc_loss(lp, y, il, tl, blank=0, reduction="none", zero_infinity=False)
    return raw.detach(), xx.grad


def _ours(dev, x, rows, ilens, gscale, want_grad=True, Umax=None):
    B, T, V = x.shape
    Umax = max(len(r) for r in rows) if Umax is None else Umax
    y = _pad(rows, Umax).to(dev)
    lp = torch.empty(B * T, V, device=dev)
    K.log_softmax(x.reshape(B * T, V).contiguous().to(dev), lp, B * T, V)
    nll = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    grad = torch.full((B * T, V), float("nan"), device=dev) if want_grad else None
    K.ctc_loss(lp, y, Umax, torch.tensor(ilens, dtype=torch.int32).to(dev),
               torch.tensor([len(r) for r in rows], dtype=torch.int32).to(dev), B, T, V, 0, gscale, True, nll, grad)
    torch.cuda.synchronize()
    return nll.cpu(), grad.cpu().view(B, T, V) if want_grad else None


def _check(what, x, rows, ilens, gscale, nll, grad, refs=None):
    """The checks every case shares; returns (nll64, grad64, nll gate, gradient gate)."""
    n64, g64 = refs[0] if refs else _ref(x, rows, ilens, gscale, torch.float64)
    n32, g32 = refs[1] if refs else _ref(x, rows, ilens, gscale, torch.float32)
    inf = torch.isinf(n64)
    assert not torch.isnan(nll).any() and not torch.isnan(grad).any(), what
    assert torch.equal(torch.isinf(nll), inf), (what, nll, n64)
    assert torch.equal(torch.isinf(n32), inf) and torch.isfinite(g32).all(), what  # the yardstick itself is sound
    fin = ~inf
    e_n = float((nll[fin] - n64[fin]).abs().max()) if fin.any() else 0.0
    r_n = float((n32[fin].double() - n64[fin]).abs().max()) if fin.any() else 0.0
    gate_n = max(2 * r_n, NLL_FLOOR)
    e_g = float((grad.double() - g64).abs().max())
    r_g = float((g32.double() - g64).abs().max())
    gate_g = max(2 * r_g, GRAD_FLOOR)
    print(f"{what}: nll ours {e_n:.3e}, torch fp32 {r_n:.3e}, gate {gate_n:.3e}; "
          f"grad ours {e_g:.3e}, torch fp32 {r_g:.3e}, gate {gate_g:.3e}")
    assert e_n <= gate_n, (what, "nll", e_n, gate_n)
    assert e_g <= gate_g, (what, "grad", e_g, gate_g)
    for b, il in enumerate(ilens):
        assert (grad[b, il:] == 0).all(), (what, b, "frames past ilen")
        if inf[b]:
            assert (grad[b] == 0).all(), (what, b, "infeasible utterance")
    return n64, g64, gate_n, gate_g


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _case_strided():
    """S = 261, 257, 255, 3, 1: two trips of the strided state loops, the 256/257 edge, and the short rows"""
    B, T, V = 5, 150, 16
    g = _gen(101)
    tlens, ilens = [130, 128, 127, 1, 0], [150, 150, 140, 150, 37]
    rows = [torch.randint(1, V, (u,), generator=g).tolist() for u in tlens]
    rows[0][60:63] = [7, 7, 7]  # a run of three equal labels
    assert all(_feasible(rows, ilens))
    x = torch.randn(B, T, V, generator=g)
    return x, rows, ilens


@functools.lru_cache(maxsize=None)
def _case_limit():
    """S = 1023, the most the kernels take, and a 601-state row beside it"""
    B, T, V = 2, 520, 8
    g = _gen(102)
    rows = [[1 + (i % 7) for i in range(511)], torch.randint(1, V, (300,), generator=g).tolist()]
    ilens = [520, 520]
    assert all(_feasible(rows, ilens))
    x = torch.randn(B, T, V, generator=g)
    return x, rows, ilens


@functools.lru_cache(maxsize=None)
def _refs(case, gscale):
    x, rows, ilens = case()
    return _ref(x, rows, ilens, gscale, torch.float64), _ref(x, rows, ilens, gscale, torch.float32)


def _wide(gap):
    """T = 3, V = 4, target [1]: the label's logit far below the others, further still on the last two frames"""
    x = torch.zeros(1, 3, 4)
    x[0, :, 1] = torch.tensor([-gap, -gap - 20.0, -gap - 20.0])
    return x, [[1]], [3]


# ------------------------------------------------------------------------------------------------ CTC cases
@pytest.mark.parametrize("gmul", [1.0, 0.3])
def test_ctc_strided_states(dev, gmul):
    x, rows, ilens = _case_strided()
    gs = gmul / x.shape[0]
    nll, grad = _ours(dev, x, rows, ilens, gs)
    _check(f"strided gscale {gmul}/B", x, rows, ilens, gs, nll, grad, _refs(_case_strided, gs))
    if gmul == 1.0:  # without a gradient: the same nll, bit for bit
        nll2, _ = _ours(dev, x, rows, ilens, gs, want_grad=False)
        assert torch.equal(nll, nll2)


def test_ctc_state_limit(dev):
    x, rows, ilens = _case_limit()
    gs = 1.0 / x.shape[0]
    nll, grad = _ours(dev, x, rows, ilens, gs)
    _check("limit S=1023", x, rows, ilens, gs, nll, grad, _refs(_case_limit, gs))
    with pytest.raises(NativeError):
        _ours(dev, torch.zeros(1, 2, 8), [[1, 2]], [2], 1.0, Umax=512)


def test_ctc_no_slack(dev):
    B, T, V = 3, 12, 6
    g = _gen(103)
    x = torch.randn(B, T, V, generator=g) * 2.0
    y0 = [1 + (i % 5) for i in range(12)]
    rows, ilens = [y0, [2, 2, 3], [2, 2, 3]], [12, 4, 3]
    assert _feasible(rows, ilens) == [True, True, False]
    gs = 1.0 / B
    nll, grad = _ours(dev, x, rows, ilens, gs)
    n64, _, gate_n, gate_g = _check("no slack", x, rows, ilens, gs, nll, grad)
    assert torch.isinf(nll[2]) and torch.isfinite(nll[:2]).all()
    # row 0 has exactly one path: frame t emits y_t
    lp0 = torch.log_softmax(x[0].double(), -1)
    idx = torch.tensor(y0)
    direct = -lp0[torch.arange(T), idx].sum()
    e = abs(float(nll[0] - direct))
    print(f"no slack, one path: nll ours vs -sum lp {e:.3e}, gate {gate_n:.3e}")
    assert e <= gate_n
    want = (lp0.exp() - F.one_hot(idx, V)) * gs
    e = float((grad[0].double() - want).abs().max())
    print(f"no slack, one path: grad ours vs softmax - onehot {e:.3e}, gate {gate_g:.3e}")
    assert e <= gate_g


def test_ctc_tiny(dev):
    g = _gen(104)
    x = torch.randn(4, 1, 5, generator=g)  # T = 1: U = 0, 1, 2 (infeasible), and no input frame at all
    rows, ilens = [[], [3], [3, 4], [2]], [1, 1, 1, 0]
    nll, grad = _ours(dev, x, rows, ilens, 0.25)
    _check("tiny T=1", x, rows, ilens, 0.25, nll, grad)
    assert torch.isinf(nll).tolist() == [False, False, True, True]
    x = torch.randn(2, 3, 1, generator=g)  # V = 1: the blank alone
    rows, ilens = [[], []], [3, 1]
    nll, grad = _ours(dev, x, rows, ilens, 0.5, Umax=1)
    _check("tiny V=1", x, rows, ilens, 0.5, nll, grad)
    assert (nll == 0).all() and (grad == 0).all()


@pytest.mark.parametrize("V", [257, 8192])
def test_ctc_vocabulary(dev, V):
    x = torch.randn(1, 4, V, generator=_gen(105)) * 3.0
    rows, ilens = [[V - 1, 1]], [4]
    nll, grad = _ours(dev, x, rows, ilens, 1.0)
    _check(f"V={V}", x, rows, ilens, 1.0, nll, grad)


def test_ctc_vocabulary_limit_raises(dev):
    with pytest.raises(NativeError):
        _ours(dev, torch.zeros(1, 4, 8193), [[1, 2]], [4], 1.0)


def _wide_condition(x, rows, ilens, gs):
    """what the wide-range inputs were chosen for: torch's fp32 stays finite and near fp64, so the gate is tight"""
    r64, r32 = _ref(x, rows, ilens, gs, torch.float64), _ref(x, rows, ilens, gs, torch.float32)
    assert torch.isfinite(r32[0]).all() and torch.isfinite(r32[1]).all()
    e = float((r32[1].double() - r64[1]).abs().max())
    print(f"wide-range condition: torch fp32 gradient within {e:.3e} of fp64")
    assert e <= 1e-4
    return r64, r32


@pytest.mark.parametrize("gap", [20, 60, 110, 140, 250])
def test_ctc_wide_range(dev, gap):
    """Measured on the MI355X with the occupancy as exp(v - max v) * exp(max v + nll - lp): gap 110 gave inf and
    NaN in frame 0 (a denormal sum times an overflowed factor), gap 140 and 250 a gradient error of 1.0 (the sum
    underflowed and the occupancy term dropped).  Formed per state as exp(v + nll - lp): 3.8e-8 at every gap."""
    x, rows, ilens = _wide(float(gap))
    refs = _wide_condition(x, rows, ilens, 1.0)
    nll, grad = _ours(dev, x, rows, ilens, 1.0)
    _check(f"wide g={gap}", x, rows, ilens, 1.0, nll, grad, refs)


def test_ctc_wide_range_random(dev):
    B, T, V = 3, 30, 12
    g = _gen(106)
    x = torch.randn(B, T, V, generator=g) * 40.0
    rows = [torch.randint(1, V, (u,), generator=g).tolist() for u in (6, 4, 1)]
    ilens = [30, 25, 30]
    assert all(_feasible(rows, ilens))
    gs = 1.0 / B
    refs = _wide_condition(x, rows, ilens, gs)
    nll, grad = _ours(dev, x, rows, ilens, gs)
    _check("wide random x40", x, rows, ilens, gs, nll, grad, refs)


@pytest.mark.parametrize("case", [_case_strided, _case_limit], ids=["strided", "limit"])
def test_ctc_repeats_bit_for_bit(dev, case):
    x, rows, ilens = case()
    gs = 1.0 / x.shape[0]
    n1, g1 = _ours(dev, x, rows, ilens, gs)
    n2, g2 = _ours(dev, x, rows, ilens, gs)
    assert torch.isfinite(g1).all()
    assert torch.equal(n1, n2) and torch.equal(g1, g2)


# ------------------------------------------------------------------------------------------------ neighbours
def _gate(what, got, ref32, want64, floor):
    e_got = float((got.double() - want64).abs().max())
    e_ref = float((ref32.double() - want64).abs().max())
    gate = max(2 * e_ref, floor)
    print(f"{what}: ours {e_got:.3e}, torch fp32 {e_ref:.3e}, gate {gate:.3e}")
    assert e_got <= gate, (what, e_got, gate)


@pytest.mark.parametrize("V", [1, 255, 257, 8192])
def test_log_softmax(dev, V):
    """Floor 1e-5: outputs of the unit-scale rows are below 32 in magnitude, where fp32 resolves 2e-6."""
    g = _gen(107)
    x = torch.randn(6, V, generator=g) * 3.0
    x[4] = torch.randn(V, generator=g) * 1e4
    if V > 1:
        x[2, V // 2] = float("-inf")
    y = torch.empty(6, V, device=dev)
    K.log_softmax(x.to(dev), y, 6, V)
    y = y.cpu()
    want, ref32 = torch.log_softmax(x.double(), -1), torch.log_softmax(x, -1)
    ninf = torch.isinf(want)
    assert torch.equal(torch.isinf(y) & (y < 0), ninf) and not torch.isnan(y).any()
    y, want, ref32 = (t.masked_fill(ninf, 0.0) for t in (y, want, ref32))
    small = [0, 1, 2, 3, 5]
    _gate(f"log_softmax V={V} unit rows", y[small], ref32[small], want[small], 1e-5)
    _gate(f"log_softmax V={V} 1e4 row", y[4], ref32[4], want[4], 1e-5)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_label_smoothing_many_rows_and_ties(dev, smoothing):
    R, V = 300, 5000
    g = _gen(108)
    x = torch.randn(R, V, generator=g) * 3.0
    tgt = torch.randint(0, V, (R,), generator=g)
    tgt[::3] = x.argmax(-1)[::3]  # a third right, so the accuracy is neither 0 nor 1
    tgt[::7] = -1
    # tied maxima; a column c belongs to thread c % 256, wave (c % 256) // 64.  (first, second): the first in a
    # later wave than the second; both in one wave; one thread's two trips; the last column against the first
    ties = [(70, 778), (5, 200), (300, 556), (0, V - 1), (130, 4100), (255, 256)]
    for i, (c1, c2) in enumerate(ties):
        for r, t in ((20 + 2 * i, c1), (21 + 2 * i, c2)):  # the target on the first, then on the second
            x[r, c1] = x[r, c2] = 50.0
            tgt[r] = t
    xt = x.double().requires_grad_(True)
    ref = O.label_smoothing_loss(xt.view(1, R, V), tgt.view(1, R), V, -1, smoothing)
    ref.backward()
    acc = O.th_accuracy(x, tgt.view(1, R), -1)
    assert 0.2 < acc < 0.8
    grad = torch.full((R, V), float("nan"), device=dev)
    rl = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    rs = torch.full((2 * R,), -7, dtype=torch.int32, device=dev)
    K.label_smoothing(x.to(dev), tgt.to(dev), V, -1, smoothing, 1.0, grad, rl, rs)
    out4 = torch.full((4,), float("nan"), device=dev)
    K.reduce_losses(None, 1, True, rl, rs, R, 1.0, 0.0, out4)
    rs = rs.cpu().view(R, 2)
    pred_ok = (x.argmax(-1) == tgt) & (tgt != -1)
    assert torch.equal(rs[:, 0].bool(), pred_ok), "first index must win a tie, as in torch.argmax"
    assert torch.equal(rs[:, 1].bool(), tgt != -1)
    print(f"label smoothing {smoothing}: loss {out4[1].item():.6f} vs {ref.item():.6f}, acc {out4[2].item():.6f} vs "
          f"{acc:.6f}, grad rel {rel_err(grad.cpu(), xt.grad):.3e}")
    assert abs(out4[1].item() - ref.item()) < 1e-4 * max(1, abs(ref.item()))
    assert abs(out4[2].item() - acc) < 1e-6
    assert rel_err(grad.cpu(), xt.grad) < 1e-5
    assert (grad.cpu()[tgt == -1] == 0).all()


def test_reduce_losses_many_utterances_length_normalised(dev):
    """One fp32 rounding of an fp64 sum: relative 2^-24, gated at 2^-23."""
    B = R = 300
    g = _gen(109)
    nll = torch.rand(B, generator=g, dtype=torch.float64) * 200.0
    nll[::11] = float("inf")
    rl = torch.rand(R, generator=g, dtype=torch.float64) * 9.0
    counted = torch.rand(R, generator=g) < 0.8
    right = (torch.rand(R, generator=g) < 0.5) & counted
    rl[~counted] = 0.0
    rs = torch.stack([right, counted], 1).to(torch.int32).contiguous()
    n = int(counted.sum())
    w = 0.3
    out5 = torch.full((5,), float("nan"), device=dev)
    K.reduce_losses(nll.to(dev), B, True, rl.to(dev), rs.view(-1).to(dev), R, 0.0, w, out5)
    out5 = out5.cpu()
    lc = float(nll[torch.isfinite(nll)].sum()) / B
    lat = float(rl.sum()) / n
    w32 = float(torch.tensor(w, dtype=torch.float32))
    want = [lc, lat, float(right.sum()) / n, w32 * lc + (1.0 - w32) * lat]
    for i, wv in enumerate(want):
        print(f"reduce_losses out[{i}] {out5[i].item():.8f} vs {wv:.8f}")
        assert abs(out5[i].item() - wv) <= 2.0 ** -23 * abs(wv), i
    assert out5[4].item() == torch.tensor(1.0 / n, dtype=torch.float64).float().item()
