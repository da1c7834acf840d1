"""gemm_dgrad_ws_kernel (csrc/gemm_dgrad_ws.hip): the conv2 input gradient's four parity-class GEMMs with dz2 gathered
and split once per block on producer waves, against the LDS-DMA kernel it replaces (esp_set_dgrad_ws(0)) on the same
inputs.  esp_set_dgrad_ws(2) takes the new kernel for every eligible class launch; the launch counter
(K.dgrad_ws_launches) shows which kernel ran.

dz1 (esp_conv2_dgrad_bits): both kernels issue the same MFMAs per accumulator and share the store, so the masked dz1
must be torch.equal between the modes; an fp64 restatement (transposed convolution, mask) guards against a
bit-identical wrong answer.

dW / db of conv1 (esp_conv2_dgrad_c1fold): the per-tile sums are the same, their summation order over tiles and blocks
differs, so the gate is on the error against fp64: the new kernel's worst relative error (max |got - ref| / max |ref|,
the larger of dW's and db's) is at most 2 x the larger of mode 0's and a plain torch fp32 run's on the same inputs.
The three figures are printed (FIGURES lines; recorded in profiles/r30a_test_conv2_dgrad_ws_figures.txt)."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

# (B, T1, F1, D): a every class smaller than one tile; b several tiles with a partial last one; c even T1 and F1 (the
# class grids differ in size, the last map row / column lies outside the transposed convolution's reach); d two column
# tiles
SHAPES = {"a": (2, 13, 7, 256), "b": (3, 37, 11, 256), "c": (2, 12, 8, 256), "d": (1, 13, 7, 512)}
# the auto rule (mode 1): the shape of >= 4 rounds of tiles per class, and the classes it admits there (by K)
AUTO_SHAPE = (24, 749, 39, 256)
AUTO_CLASSES = 4
# the fold over more tiles than CUs (every class > 256 tiles of 128 rows): a block's sums carried across its tiles, the
# producers' LDS image of a tile's rows re-used tile after tile; at D = 512 a block also returns to a column tile
# (the records' read-modify-write)
FOLD_MULTI = [(16, 261, 39, 256), (16, 261, 39, 512)]


def _out(n):
    return (n - 3) // 2 + 1


@contextlib.contextmanager
def _mode(mode, expect=None):
    """esp_set_dgrad_ws(mode) around the body; expect: the launches of the new kernel the body must add."""
    prev = K.set_dgrad_ws(mode)
    n0 = K.dgrad_ws_launches()
    try:
        yield
    finally:
        K.set_dgrad_ws(prev)
    if expect is not None:
        assert K.dgrad_ws_launches() - n0 == expect, (mode, K.dgrad_ws_launches() - n0, expect)


def _inputs(name, bits="rand"):
    B, T1, F1, D = SHAPES[name]
    T2, F2 = _out(T1), _out(F1)
    T, Fd = 2 * T1 + 2, 2 * F1 + 1  # a conv1 input with (T - 3) // 2 + 1 == T1
    gen = torch.Generator().manual_seed(7 + ord(name))
    dz2 = torch.randn(B * T2 * F2, D, generator=gen)
    W = torch.randn(D, D, 3, 3, generator=gen) / math.sqrt(9 * D)
    x = torch.randn(B, T, Fd, generator=gen)
    nw = B * T1 * F1 * D // 32
    if bits == "rand":  # ~50 % density
        zb = torch.randint(-2**31, 2**31, (nw,), generator=gen, dtype=torch.int64).to(torch.int32)
    else:
        zb = torch.full((nw,), -1 if bits == "ones" else 0, dtype=torch.int32)
    return dz2, W, x, zb


def _mask(zb, B, T1, F1, D):
    """The bit map as a (B, D, T1, F1) 0/1 tensor: bit c % 32 of word pixel * (D / 32) + c / 32."""
    m = (zb.view(-1, D // 32, 1).to(torch.int64) >> torch.arange(32)) & 1
    return m.view(B, T1, F1, D).permute(0, 3, 1, 2)


def _ref(name, dz2, W, x, zb, dtype):
    """dz1 (B, T1, F1, D), dW (D, 9), db (D) restated with torch in `dtype`."""
    B, T1, F1, D = SHAPES[name]
    T2, F2 = _out(T1), _out(F1)
    g = dz2.to(dtype).view(B, T2, F2, D).permute(0, 3, 1, 2)
    d = F.conv_transpose2d(g, W.to(dtype), stride=2)  # (B, D, 2 T2 + 1, 2 F2 + 1)
    d = F.pad(d, (0, F1 - d.shape[3], 0, T1 - d.shape[2])) * _mask(zb, B, T1, F1, D).to(dtype)
    patches = F.unfold(x.to(dtype)[:, None], 3, stride=2)  # (B, 9, T1 * F1)
    dW = torch.einsum("bcl,bkl->ck", d.reshape(B, D, -1), patches)
    return d.permute(0, 2, 3, 1).contiguous(), dW, d.sum(dim=(0, 2, 3))


def _run_bits(name, mode, dz2, W, zb, dev, expect=None):
    B, T1, F1, D = SHAPES[name]
    dz1 = torch.full((B * T1 * F1 * D,), float("nan"), device=dev)
    with _mode(mode, expect):
        K.conv2_dgrad(dz2.to(dev), W.to(dev), None, dz1, B, T1, F1, D, z1bits=zb.to(dev))
        torch.cuda.synchronize()
    return dz1.cpu().view(B, T1, F1, D)


def _run_fold(name, mode, dz2, W, x, zb, dev, expect=None, init=None):
    B, T1, F1, D = SHAPES[name]
    dW = torch.zeros(D, 9) if init is None else init[0].clone()
    db = torch.zeros(D) if init is None else init[1].clone()
    dW, db = dW.to(dev), db.to(dev)
    with _mode(mode, expect):
        K.conv2_dgrad_c1fold(dz2.to(dev), W.to(dev), zb.to(dev), x.to(dev), x.shape[1], x.shape[2], dW, db, B, T1, F1, D)
        torch.cuda.synchronize()
    return dW.cpu(), db.cpu()


_CACHE = {}


def _case(name, dev):
    """Inputs (random bit map) and, computed once: dz1 in mode 0 and twice in mode 2, the fold in mode 0 and twice in
    mode 2, the fp64 reference."""
    if name not in _CACHE:
        dz2, W, x, zb = _inputs(name)
        _CACHE[name] = dict(
            inp=(dz2, W, x, zb), ref=_ref(name, dz2, W, x, zb, torch.float64),
            old=_run_bits(name, 0, dz2, W, zb, dev, 0), new=_run_bits(name, 2, dz2, W, zb, dev, 4),
            new2=_run_bits(name, 2, dz2, W, zb, dev, 4),
            fold_old=_run_fold(name, 0, dz2, W, x, zb, dev, 0), fold_new=_run_fold(name, 2, dz2, W, x, zb, dev, 4),
            fold_new2=_run_fold(name, 2, dz2, W, x, zb, dev, 4))
    return _CACHE[name]


def _err(got, ref):
    return max(((g.double() - r).abs().max() / r.abs().max()).item() for g, r in zip(got, ref))


@pytest.mark.parametrize("name", list(SHAPES))
def test_dgrad_ws_dz1_bit_identical(dev, name):
    """Mode 2 (4 launches of the new kernel) against mode 0 (none): torch.equal, and both right against fp64."""
    c = _case(name, dev)
    assert torch.isfinite(c["new"]).all()
    assert torch.equal(c["new"], c["old"])
    ref = c["ref"][0]
    # fp32 on split products: ~2^-22 per product, K <= 4 D terms of |dz2| |W| ~ 1 / sqrt(9 D) each
    assert (c["new"].double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert c["new"].abs().sum().item() > 0


@pytest.mark.parametrize("bits", ["zeros", "ones"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_dgrad_ws_dz1_constant_masks(dev, name, bits):
    dz2, W, x, zb = _inputs(name, bits)
    old, new = _run_bits(name, 0, dz2, W, zb, dev, 0), _run_bits(name, 2, dz2, W, zb, dev, 4)
    assert torch.equal(new, old)
    if bits == "zeros":
        assert not new.any()
    else:
        ref = _ref(name, dz2, W, x, zb, torch.float64)[0]
        assert (new.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("name", list(SHAPES))
def test_dgrad_ws_fold_gradient(dev, name):
    """dW / db of the fold against fp64: new <= 2 x max(mode 0, torch fp32); only the summation order over tiles and
    blocks differs between the kernels."""
    c = _case(name, dev)
    dz2, W, x, zb = c["inp"]
    ref = c["ref"][1:]
    e_new, e_old = _err(c["fold_new"], ref), _err(c["fold_old"], ref)
    e_t32 = _err(_ref(name, dz2, W, x, zb, torch.float32)[1:], ref)
    print(f"FIGURES fold {name} {SHAPES[name]}: new {e_new:.3e}  mode 0 {e_old:.3e}  torch fp32 {e_t32:.3e}")
    assert all(torch.isfinite(t).all() for t in c["fold_new"])
    assert e_new <= 2.0 * max(e_old, e_t32), (e_new, e_old, e_t32)


def test_dgrad_ws_fold_accumulates_and_zero_mask(dev):
    """dW / db are accumulated into (one fp32 addition of the reduced sum to the start); an all-zero mask adds
    exactly 0."""
    name = "b"
    c = _case(name, dev)
    dz2, W, x, zb = c["inp"]
    B, T1, F1, D = SHAPES[name]
    gen = torch.Generator().manual_seed(3)
    init = (torch.randn(D, 9, generator=gen), torch.randn(D, generator=gen))
    dW, db = _run_fold(name, 2, dz2, W, x, zb, dev, 4, init=init)
    # the finalize kernel adds the reduced sum to the start in one fp32 addition
    assert torch.equal(dW, init[0] + (c["fold_new"][0])) and torch.equal(db, init[1] + c["fold_new"][1])
    zero = torch.zeros_like(zb)
    dW0, db0 = _run_fold(name, 2, dz2, W, x, zero, dev, 4)
    assert not dW0.any() and not db0.any()
    dW1, db1 = _run_fold(name, 2, dz2, W, x, zero, dev, 4, init=init)
    assert torch.equal(dW1, init[0]) and torch.equal(db1, init[1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_dgrad_ws_deterministic(dev, name):
    c = _case(name, dev)
    assert torch.equal(c["new"], c["new2"])
    assert torch.equal(c["fold_new"][0], c["fold_new2"][0]) and torch.equal(c["fold_new"][1], c["fold_new2"][1])


def test_dgrad_ws_nonfinite_dz2(dev):
    """One inf and one NaN in dz2: the non-finite set of dz1 equals mode 0's, the finite values are bit-equal."""
    name = "b"
    dz2, W, x, zb = _inputs(name, "ones")
    dz2 = dz2.clone()
    dz2[5, 17] = float("inf")
    dz2[dz2.shape[0] - 3, 200] = float("nan")
    old, new = _run_bits(name, 0, dz2, W, zb, dev, 0), _run_bits(name, 2, dz2, W, zb, dev, 4)
    fo, fn = torch.isfinite(old), torch.isfinite(new)
    assert torch.equal(fo, fn)
    assert 0 < (~fn).sum().item() < fn.numel()
    assert torch.equal(old[fo], new[fn])


def test_dgrad_ws_auto_rule(dev):
    """Mode 1: at the shape of >= 4 rounds of tiles per class the admitted classes run the new kernel and dz1 equals
    mode 0's; at shape a (one tile per class) none does."""
    c = _case("a", dev)
    dz2, W, x, zb = c["inp"]
    assert torch.equal(_run_bits("a", 1, dz2, W, zb, dev, 0), c["old"])
    B, T1, F1, D = AUTO_SHAPE
    T2, F2 = _out(T1), _out(F1)
    gen = torch.Generator(device=dev).manual_seed(1)
    dz2 = torch.randn(B * T2 * F2, D, device=dev, generator=gen)
    W = torch.randn(D, D, 3, 3, device=dev, generator=gen) / math.sqrt(9 * D)
    zb = torch.randint(-2**31, 2**31, (B * T1 * F1 * D // 32,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    res = []
    for mode, expect in ((0, 0), (1, AUTO_CLASSES)):
        dz1 = torch.full((B * T1 * F1 * D,), float("nan"), device=dev)
        with _mode(mode, expect):
            K.conv2_dgrad(dz2, W, None, dz1, B, T1, F1, D, z1bits=zb)
            torch.cuda.synchronize()
        res.append(dz1)
    assert torch.equal(res[0], res[1])
    assert torch.isfinite(res[1]).all()


@pytest.mark.parametrize("shape", FOLD_MULTI, ids=lambda v: "x".join(map(str, v)))
def test_dgrad_ws_fold_many_tiles(dev, shape):
    """The fold at more than one tile per block, modes 0 and 2 (twice: bit-equal), under the fold's gate.  The
    reference is the fp64 sum, on the device, of the stored dz1 (which the two kernels give bit for bit, checked here
    too) times the conv1-input patches; the torch fp32 figure is the same sum in fp32."""
    B, T1, F1, D = shape
    T2, F2 = _out(T1), _out(F1)
    T, Fd = 2 * T1 + 2, 2 * F1 + 1
    gen = torch.Generator(device=dev).manual_seed(2)
    dz2 = torch.randn(B * T2 * F2, D, device=dev, generator=gen)
    W = torch.randn(D, D, 3, 3, device=dev, generator=gen) / math.sqrt(9 * D)
    x = torch.randn(B, T, Fd, device=dev, generator=gen)
    zb = torch.randint(-2**31, 2**31, (B * T1 * F1 * D // 32,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    assert min((B * ((T1 - ph + 1) // 2) * ((F1 - pw + 1) // 2) + 127) // 128 for ph in (0, 1) for pw in (0, 1)) > 256
    dz1 = {}
    for mode in (0, 2):
        dz1[mode] = torch.full((B * T1 * F1 * D,), float("nan"), device=dev)
        with _mode(mode, 4 if mode else 0):
            K.conv2_dgrad(dz2, W, None, dz1[mode], B, T1, F1, D, z1bits=zb)
            torch.cuda.synchronize()
    assert torch.equal(dz1[0], dz1[2]) and torch.isfinite(dz1[2]).all()
    d = dz1.pop(0).view(B, T1 * F1, D)
    dz1.clear()
    patches = F.unfold(x[:, None], 3, stride=2)  # (B, 9, T1 * F1)
    ref = (torch.einsum("bld,bkl->dk", d.double(), patches.double()).cpu(), d.double().sum(dim=(0, 1)).cpu())
    t32 = (torch.einsum("bld,bkl->dk", d, patches).cpu(), d.sum(dim=(0, 1)).cpu())
    del d, patches

    def fold(mode):
        dW, db = torch.zeros(D, 9, device=dev), torch.zeros(D, device=dev)
        with _mode(mode, 4 if mode else 0):
            K.conv2_dgrad_c1fold(dz2, W, zb, x, T, Fd, dW, db, B, T1, F1, D)
            torch.cuda.synchronize()
        return dW.cpu(), db.cpu()

    old, new, new2 = fold(0), fold(2), fold(2)
    assert torch.equal(new[0], new2[0]) and torch.equal(new[1], new2[1])
    e_new, e_old, e_t32 = _err(new, ref), _err(old, ref), _err(t32, ref)
    print(f"FIGURES fold many tiles {shape}: new {e_new:.3e}  mode 0 {e_old:.3e}  torch fp32 {e_t32:.3e}")
    assert e_new <= 2.0 * max(e_old, e_t32), (e_new, e_old, e_t32)


def test_dgrad_ws_subsampling_block(dev):
    """Conv2dSubsampling forward + backward (D = 256, B = 2, 67 frames) under modes 0 and 2: every gradient but conv1's
    is bit-equal; conv1's (through the fold) passes the fold's gate against a torch fp64 run of the same module."""
    from espnet_slurp_amd.blocks import Conv2dSubsampling, Seeds
    from espnet_slurp_amd.flat import FlatParams

    torch.manual_seed(5)
    B, T, Fd, D = 2, 67, 80, 256
    mod = Conv2dSubsampling(Fd, D)
    with torch.no_grad():
        for p in mod.parameters():
            p.normal_(0, 0.05)
    x = torch.randn(B, T, Fd)
    dout = torch.randn(B, mod.out_frames(T), D, generator=torch.Generator().manual_seed(6))

    def torch_grads(dtype):  # the module as plain torch (dropout 0): conv + ReLU twice, the Linear, x sqrt(D)
        m = Conv2dSubsampling(Fd, D).to(dtype)
        m.load_state_dict(mod.state_dict())
        y = m.conv(x.to(dtype)[:, None])
        b, c, t, f = y.shape
        y = F.linear(y.transpose(1, 2).contiguous().view(b, t, c * f), m.out[0].weight, m.out[0].bias) * math.sqrt(D)
        y.backward(dout.to(dtype).view_as(y))
        return m.conv[0].weight.grad.view(D, 9), m.conv[0].bias.grad

    ref, t32 = torch_grads(torch.float64), torch_grads(torch.float32)
    mod = mod.to(dev)
    flat = FlatParams(mod, dev)
    res = {}
    for mode in (0, 2):
        flat.grad.zero_()
        with _mode(mode, 4 if mode else 0):
            out, c = mod.fwd(x.to(dev), math.sqrt(D), 0.0, Seeds(3), True)
            mod.bwd(c, dout.to(dev).view_as(out))
            torch.cuda.synchronize()
        res[mode] = {n: p.grad.detach().cpu().clone() for n, p in mod.named_parameters()}
    for n in res[0]:
        if not n.startswith("conv.0."):
            assert torch.equal(res[2][n], res[0][n]), n
    got = {m: (res[m]["conv.0.weight"].view(D, 9), res[m]["conv.0.bias"]) for m in (0, 2)}
    e_new, e_old, e_t32 = _err(got[2], ref), _err(got[0], ref), _err(t32, ref)
    print(f"FIGURES block conv1 grads: new {e_new:.3e}  mode 0 {e_old:.3e}  torch fp32 {e_t32:.3e}")
    assert e_new <= 2.0 * max(e_old, e_t32), (e_new, e_old, e_t32)
