"""The RNN-Transducer kernels (csrc/rnnt.hip), each against plain torch on the CPU in fp64, with the same
computation in fp32 as the yardstick: err(ours vs fp64) <= max(2 * err(fp32 torch vs fp64), floor), floors 1e-4 on
nll and 1e-5 of the tensor's fp64 maximum on gradients.

Lattice (esp_rnnt_logprobs / _alpha_beta / _grad against tests/rnnt_helpers.py): one batch of (T_b, U_b) = (1, 0),
(1, 3), (5, 0), (3, 70), (130, 2), (40, 40) padded to T = 133, Umax = 72, at V = 5, 37, 130 and at two logit scales
(ordinary; x 60, log-probabilities hundreds of nats apart), and one of (2, 300), (4, 257): more than 256 cells on a
diagonal, several per thread.  nll from alpha equals -beta[0, 0]; padded cells hold exactly zero; padded logits are
NaN on entry (they must not be read); every output buffer is NaN on entry; a repeat run is bit-equal.

Joint (esp_rnnt_joint_fwd / _bwd against autograd): J = 20, 64, 200 x T = 1, 70 x U1 = 1, 9, ragged lengths.
"""
import functools

import pytest
import torch

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd._native import NativeError
from tests.rnnt_helpers import lattice, rnnt_nll

pytestmark = pytest.mark.gpu

NLL_FLOOR, GRAD_FLOOR = 1e-4, 1e-5
MIXED = dict(lens=[(1, 0), (1, 3), (5, 0), (3, 70), (130, 2), (40, 40)], T=133, Umax=72)
WIDE = dict(lens=[(2, 300), (4, 257)], T=5, Umax=301)
GSCALE = 1.0 / 3.0


@functools.lru_cache(maxsize=None)
def _inputs(which, V, scale):
    spec = MIXED if which == "mixed" else WIDE
    g = torch.Generator().manual_seed(1000 + V)
    B, T, Umax = len(spec["lens"]), spec["T"], spec["Umax"]
    x = torch.randn(B, T, Umax + 1, V, generator=g) * scale
    ys = torch.full((B, Umax), -1, dtype=torch.int64)
    for b, (_, u) in enumerate(spec["lens"]):
        ys[b, :u] = torch.randint(1, V, (u,), generator=g)
    return x, ys, [t for t, _ in spec["lens"]], [u for _, u in spec["lens"]]


@functools.lru_cache(maxsize=None)
def _ref(which, V, scale, dtype):
    """(nll, gradient of GSCALE * sum nll w.r.t. the logits) on the CPU in dtype."""
    x, ys, tl, ul = _inputs(which, V, scale)
    xx = x.to(dtype).requires_grad_(True)
    nll = rnnt_nll(xx, ys, tl, ul)
    (GSCALE * nll.sum()).backward()
    return nll.detach(), xx.grad


def _ours(dev, which, V, scale, gdev=None):
    x, ys, tl, ul = _inputs(which, V, scale)
    B, T, U1, _ = x.shape
    valid = torch.zeros(B, T, U1, dtype=torch.bool)
    for b in range(B):
        valid[b, :tl[b], :ul[b] + 1] = True
    xin = torch.where(valid[..., None], x, torch.full_like(x, float("nan")))  # padded logits must not be read
    logits = xin.reshape(B * T * U1, V).contiguous().to(dev)
    hl, tlen = torch.tensor(tl, dtype=torch.int32).to(dev), torch.tensor(ul, dtype=torch.int32).to(dev)
    ysd = ys.to(dev)
    work = K.rnnt_workspace(B, T, U1, dev)
    work.fill_(float("nan"))
    nll = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    K.rnnt_logprobs(logits, ysd, hl, tlen, B, T, U1, V, work)
    K.rnnt_alpha_beta(hl, tlen, B, T, U1, work, nll)
    K.rnnt_grad(logits, ysd, hl, tlen, B, T, U1, V, GSCALE, nll, work, gdev=gdev)
    torch.cuda.synchronize()
    return nll.cpu(), logits.cpu().view(B, T, U1, V), work.cpu().view(5, B, T, U1), valid


@pytest.mark.parametrize("scale", [1.0, 60.0], ids=["plain", "wide_range"])
@pytest.mark.parametrize("V", [5, 37, 130])
def test_lattice_mixed_lengths(dev, V, scale):
    _lattice_case(dev, "mixed", V, scale)


def test_lattice_more_cells_than_threads(dev):
    _lattice_case(dev, "wide", 5, 1.0)


def _lattice_case(dev, which, V, scale):
    n64, g64 = _ref(which, V, scale, torch.float64)
    n32, g32 = _ref(which, V, scale, torch.float32)
    nll, grad, work, valid = _ours(dev, which, V, scale)
    what = f"{which} V={V} scale={scale}"
    assert not torch.isnan(nll).any() and not torch.isnan(grad).any() and not torch.isnan(work).any(), what
    e_n, r_n = float((nll - n64).abs().max()), float((n32.double() - n64).abs().max())
    gate_n = max(2 * r_n, NLL_FLOOR)
    gm = float(g64.abs().max())
    e_g, r_g = float((grad.double() - g64).abs().max()) / gm, float((g32.double() - g64).abs().max()) / gm
    gate_g = max(2 * r_g, GRAD_FLOOR)
    beta00 = work[4][:, 0, 0]
    e_b = float((nll + beta00).abs().max())
    print(f"{what}: nll ours {e_n:.3e}, torch fp32 {r_n:.3e}, gate {gate_n:.3e}; nll + beta00 {e_b:.3e}; "
          f"grad/max ours {e_g:.3e}, torch fp32 {r_g:.3e}, gate {gate_g:.3e}; nll range {float(n64.min()):.1f} .. "
          f"{float(n64.max()):.1f}")
    assert e_n <= gate_n, (what, "nll", e_n, gate_n)
    assert e_b <= gate_n, (what, "nll vs -beta[0,0]", e_b, gate_n)
    assert e_g <= gate_g, (what, "grad", e_g, gate_g)
    assert (grad[~valid] == 0).all(), (what, "gradient in padded cells")
    assert (work[:, ~valid] == 0).all(), (what, "workspace in padded cells")
    if scale > 1.0:  # the log-probabilities of a cell do lie hundreds of nats apart
        x = _inputs(which, V, scale)[0]
        assert float((x.max(-1)[0] - x.min(-1)[0]).max()) > 200.0
    # alpha and beta themselves, on the longest lattice
    x, ys, tl, ul = _inputs(which, V, scale)
    b = max(range(len(tl)), key=lambda i: tl[i] * (ul[i] + 1))
    lp = torch.log_softmax(x[b, :tl[b], :ul[b] + 1].double(), -1)
    al, be = lattice(lp, ys[b, :ul[b]].tolist())
    assert float((work[3][b, :tl[b], :ul[b] + 1] - al).abs().max()) <= gate_n, what
    assert float((work[4][b, :tl[b], :ul[b] + 1] - be).abs().max()) <= gate_n, what


def test_repeat_run_is_bit_equal_and_gdev_scales(dev):
    a = _ours(dev, "mixed", 37, 1.0)
    b = _ours(dev, "mixed", 37, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    two = torch.tensor([2.0], device=dev)
    c = _ours(dev, "mixed", 37, 1.0, gdev=two)
    g64 = _ref("mixed", 37, 1.0, torch.float64)[1]
    assert float((c[1].double() - 2 * g64).abs().max()) <= 2 * GRAD_FLOOR * float(g64.abs().max())


def test_limits_raise(dev):
    hl = torch.ones(1, dtype=torch.int32, device=dev)
    work = K.rnnt_workspace(1, 1, 4, dev)
    with pytest.raises(NativeError, match="U1=1025"):
        K.rnnt_alpha_beta(hl, hl, 1, 1, 1025, torch.empty(8, dtype=torch.float64, device=dev),
                          torch.empty(1, dtype=torch.float64, device=dev))
    with pytest.raises(NativeError, match="workspace"):
        K.rnnt_alpha_beta(hl, hl, 1, 2, 4, work, torch.empty(1, dtype=torch.float64, device=dev))
    with pytest.raises(NotImplementedError, match="swish"):
        K.rnnt_act("swish")


# ------------------------------------------------------------------------------------------------ joint
def _joint_ref(pe, pd, dz, tl, ul, act, dtype):
    pe, pd = pe.to(dtype).requires_grad_(True), pd.to(dtype).requires_grad_(True)
    z = pe[:, :, None, :] + pd[:, None, :, :]
    z = torch.tanh(z) if act == "tanh" else torch.relu(z)
    mask = torch.zeros(z.shape[:3], dtype=torch.bool)
    for b in range(len(tl)):
        mask[b, :tl[b], :ul[b] + 1] = True
    (z * dz.to(dtype) * mask[..., None]).sum().backward()
    return z.detach(), pe.grad, pd.grad


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("U1", [1, 9])
@pytest.mark.parametrize("T", [1, 70])
@pytest.mark.parametrize("J", [20, 64, 200])
def test_joint_and_its_two_reductions(dev, J, T, U1, act):
    B = 3
    g = torch.Generator().manual_seed(J * 1000 + T * 10 + U1)
    pe, pd = torch.randn(B, T, J, generator=g), torch.randn(B, U1, J, generator=g)
    dz = torch.randn(B, T, U1, J, generator=g)
    tl = [T, max(1, T // 2), max(1, T - 3)]
    ul = [U1 - 1, 0, max(0, U1 - 4)]
    z64, dpe64, dpd64 = _joint_ref(pe, pd, dz, tl, ul, act, torch.float64)
    z32, dpe32, dpd32 = _joint_ref(pe, pd, dz, tl, ul, act, torch.float32)
    code = K.rnnt_act(act)
    z = torch.full((B * T * U1, J), float("nan"), device=dev)
    K.rnnt_joint_fwd(pe.reshape(B * T, J).to(dev), pd.reshape(B * U1, J).to(dev), z, B, T, U1, J, code)
    dpe = torch.full((B * T, J), float("nan"), device=dev)
    dpd = torch.full((B * U1, J), float("nan"), device=dev)
    hl, tlen = torch.tensor(tl, dtype=torch.int32).to(dev), torch.tensor(ul, dtype=torch.int32).to(dev)
    # padded cells of dz are NaN: they must not be read
    mask = torch.zeros(B, T, U1, dtype=torch.bool)
    for b in range(B):
        mask[b, :tl[b], :ul[b] + 1] = True
    dzin = torch.where(mask[..., None], dz, torch.full_like(dz, float("nan"))).reshape(B * T * U1, J).to(dev)
    outs = []
    for _ in range(2):
        K.rnnt_joint_bwd(dzin, z, hl, tlen, dpe, dpd, B, T, U1, J, code)
        torch.cuda.synchronize()
        outs.append((dpe.cpu().clone(), dpd.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # fixed order, no atomics
    zc = z.cpu().view(B, T, U1, J)
    assert float((zc.double() - z64).abs().max()) <= max(2 * float((z32.double() - z64).abs().max()), 1e-6)
    for name, got, r64, r32 in (("dpe", outs[0][0].view(B, T, J), dpe64, dpe32),
                                ("dpd", outs[0][1].view(B, U1, J), dpd64, dpd32)):
        assert not torch.isnan(got).any(), name
        gm = float(r64.abs().max())
        e, r = float((got.double() - r64).abs().max()) / gm, float((r32.double() - r64).abs().max()) / gm
        print(f"joint J={J} T={T} U1={U1} {act} {name}: ours {e:.3e}, torch fp32 {r:.3e}")
        assert e <= max(2 * r, GRAD_FLOOR), (name, e, r)
    for b in range(B):  # frames / labels past the lengths get exactly zero
        assert (outs[0][0].view(B, T, J)[b, tl[b]:] == 0).all() and (outs[0][1].view(B, U1, J)[b, ul[b] + 1:] == 0).all()
