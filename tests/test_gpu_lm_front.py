"""esp_lm_front_fwd / _bwd (csrc/lm_step.hip) on the MI355X: the LM input layer's LayerNorm -> Dropout -> ReLU ->
positional step in training form, against a torch restatement in fp64.  Gate, as in test_gpu_cbt_kernels.py: at most
twice the error of the same restatement run in fp32 on the CPU, never tighter than 1e-5 absolute; both are printed.

With dropout the keep masks are read back from the output (as test_block_attn_dropout does) and handed to the
restatement: beta is large enough that every LayerNorm output is positive, so without a table a zero is a
first-dropout drop; with a table (random, no zero entry) a zero is a second-dropout drop and a value equal to
pe * scale2 a first-dropout drop."""
import math

import pytest
import torch

from tests.helpers import keep_scale

pytestmark = pytest.mark.gpu

EPS_LN = 1e-5
SHAPES = [(7, 64, 7), (33, 128, 11), (130, 256, 13)]  # rows, D, L (rows wrap around the table: r % L)


def _inputs(rows, D, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) * 1.5 + 0.3
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 6.0 + 0.1 * torch.randn(D, generator=g)  # LN(x) > 0 everywhere (|xhat| stays far below 5)
    pe = torch.randn(L, D, generator=g)
    cot = torch.randn(rows, D, generator=g)
    return x, gamma, beta, pe, cot


def _front(x, gamma, beta, pe, L, xscale, m1, m2):
    """m1 / m2: dropout multipliers (keep * scale) or None; pe None: no scale, no table, no second dropout."""
    v = torch.nn.functional.layer_norm(x, x.shape[1:], gamma, beta, EPS_LN)
    if m1 is not None:
        v = v * m1.to(x.dtype)
    v = torch.relu(v)
    if pe is not None:
        v = v * xscale + pe.to(x.dtype)[torch.arange(x.shape[0]) % L]
        if m2 is not None:
            v = v * m2.to(x.dtype)
    return v


def _ref(x, gamma, beta, pe, L, xscale, m1, m2, cot, dtype):
    xs, gs, bs = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = _front(xs, gs, bs, pe, L, xscale, m1, m2)
    y.backward(cot.to(dtype))
    return y.detach(), xs.grad, gs.grad, bs.grad


def _run(dev, x, gamma, beta, pe, L, xscale, p, seeds, cot):
    from espnet_slurp_amd import kernels as K
    rows, D = x.shape
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    ped = pe.to(dev).contiguous() if pe is not None else None
    y = torch.full((rows, D), float("nan"), device=dev)
    mean, rstd = torch.full((rows,), float("nan"), device=dev), torch.full((rows,), float("nan"), device=dev)
    kw = dict(xscale=xscale, p1=p, seed1=seeds[0], p2=p, seed2=seeds[1])
    K.lm_front_fwd(xd, gd, bd, EPS_LN, y, mean, rstd, pe=ped, L=L, **kw)
    dx = torch.full((rows, D), float("nan"), device=dev)
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    K.lm_front_bwd(cot.to(dev), xd, gd, bd, mean, rstd, dx, dg, db, has_pe=pe is not None, **kw)
    dg1, db1 = dg.clone(), db.clone()
    K.lm_front_bwd(cot.to(dev), xd, gd, bd, mean, rstd, dx, dg, db, has_pe=pe is not None, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dg, 2 * dg1) and torch.equal(db, 2 * db1)  # dgamma / dbeta are accumulated, dx overwritten
    want_mean = x.double().mean(1)
    assert float((mean.cpu().double() - want_mean).abs().max()) <= 1e-5
    return y.cpu(), dx.cpu(), dg1.cpu(), db1.cpu()


def _gate(what, got, ref32, want64):
    e_got = float((got.double() - want64).abs().max())
    e_ref = float((ref32.double() - want64).abs().max())
    gate = max(2 * e_ref, 1e-5)
    print(f"{what}: ours {e_got:.3e}, restatement fp32 {e_ref:.3e}, gate {gate:.3e}")
    assert bool(torch.isfinite(got).all()) and e_got <= gate, (what, e_got, gate)


def _gate_all(tag, got, x, gamma, beta, pe, L, xscale, m1, m2, cot):
    r64 = _ref(x, gamma, beta, pe, L, xscale, m1, m2, cot, torch.float64)
    r32 = _ref(x, gamma, beta, pe, L, xscale, m1, m2, cot, torch.float32)
    for name, a, b, c in zip(("y", "dx", "dgamma", "dbeta"), got, r32, r64):
        _gate(f"{tag} {name}", a, b, c)


@pytest.mark.parametrize("with_pe", [True, False])
@pytest.mark.parametrize("rows,D,L", SHAPES)
def test_front_without_dropout(dev, rows, D, L, with_pe):
    from espnet_slurp_amd import kernels as K
    x, gamma, beta, pe, cot = _inputs(rows, D, L, 400 + rows)
    pe = pe if with_pe else None
    xscale = math.sqrt(D)
    got = _run(dev, x, gamma, beta, pe, L, xscale, 0.0, (0, 0), cot)
    _gate_all(f"lm_front {rows}x{D} pe={with_pe} p=0", got, x, gamma, beta, pe, L, xscale, None, None, cot)
    # the inference kernel computes the same values bit for bit
    y2 = torch.full((rows, D), float("nan"), device=dev)
    K.step_ln_act(x.to(dev), gamma.to(dev), beta.to(dev), EPS_LN, y2, pe=pe.to(dev) if with_pe else None,
                  xscale=xscale, L=L)
    assert torch.equal(y2.cpu(), got[0])


@pytest.mark.parametrize("with_pe", [True, False])
@pytest.mark.parametrize("rows,D,L", SHAPES)
def test_front_with_dropout(dev, rows, D, L, with_pe):
    p = 0.25
    sc = float(torch.tensor(keep_scale(p), dtype=torch.float32))  # the scale as the kernels hold it (an fp32 value)
    x, gamma, beta, pe, cot = _inputs(rows, D, L, 500 + rows)
    pe = pe if with_pe else None
    xscale = math.sqrt(D)
    got = _run(dev, x, gamma, beta, pe, L, xscale, p, (1234, 99), cot)
    again = _run(dev, x, gamma, beta, pe, L, xscale, p, (1234, 99), cot)
    assert all(torch.equal(a, b) for a, b in zip(got, again))  # same seeds: bit-equal
    other = _run(dev, x, gamma, beta, pe, L, xscale, p, (1235, 98), cot)
    assert not torch.equal(got[0], other[0]) and not torch.equal(got[1], other[1])
    y = got[0]
    n = rows * D
    if with_pe:
        k2 = y != 0
        dropped1 = y == pe[torch.arange(rows) % L] * torch.tensor(sc, dtype=torch.float32)
        k1 = ~dropped1  # (where k2 is 0 the first mask cannot be read and does not matter: y and every gradient are 0)
        n1 = int(k2.sum())
        fracs = [("second", float(k2.sum()) / n, n), ("first", float((k1 & k2).sum()) / n1, n1)]
        m1, m2 = k1.double() * sc, k2.double() * sc
    else:
        k1 = y != 0
        fracs = [("first", float(k1.sum()) / n, n)]
        m1, m2 = k1.double() * sc, None
    for which, frac, cnt in fracs:
        sigma = math.sqrt(p * (1 - p) / cnt)
        print(f"lm_front {rows}x{D} pe={with_pe}: {which} dropout kept {frac:.4f} of {cnt}, sigma {sigma:.4f}")
        assert abs(frac - (1 - p)) <= 4 * sigma, (which, frac)
    _gate_all(f"lm_front {rows}x{D} pe={with_pe} p={p}", got, x, gamma, beta, pe, L, xscale, m1, m2, cot)
