"""esp_decode_attn_masked (csrc/decode_attn.hip): single-query attention with a per-row key-validity byte mask,
against an fp64 numpy restatement on unit-normal inputs.

N = 3 rows over one cache-like K|V buffer (rows, TK, 2W), d_k 16 / 32 / 64, klen in {1, 63, 64, 65, 130}.  Masks: all
ones (must equal esp_decode_attn bit for bit), only key 0 valid, keys 64..127 all masked (a whole chunk masked after
valid ones), the first chunk masked except its last key (an all-masked chunk cannot come first under the contract of
one valid key per row, but 63 masked lanes beside one live lane can), and a random mask (key 0 kept).  Masked keys
hold NaN in K and V, so a read of a masked key, or an exp(-inf - -inf), shows up as a non-finite output.

Gate: twice the unmasked kernel's own error against fp64 on the all-ones case of the same d_k and klen (same
arithmetic over at most as many keys), floor 1e-6."""
import functools

import numpy as np
import pytest
import torch

from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

H, N, TK = 2, 3, 136
KLENS = (1, 63, 64, 65, 130)
MASKS = ("ones", "key0", "chunk1_off", "chunk0_last", "random")


def _mask(kind, klen, seed):
    m = np.ones((N, klen), dtype=np.uint8)
    if kind == "key0":
        m[:, 1:] = 0
    elif kind == "chunk1_off":
        m[:, 64:128] = 0
    elif kind == "chunk0_last":
        m[:, : min(klen, 64) - 1] = 0
    elif kind == "random":
        m = (np.random.RandomState(seed).rand(N, klen) < 0.5).astype(np.uint8)
        m[:, 0] = 1
    return m


@functools.lru_cache(maxsize=None)
def _inputs(dk):
    rng = np.random.RandomState(dk)
    W = H * dk
    return rng.randn(N, W).astype(np.float32), rng.randn(N, TK, 2 * W).astype(np.float32)


def _reference(q, kv, mask, dk):
    W = H * dk
    out = np.zeros((N, W))
    for n in range(N):
        keep = mask[n].astype(bool)
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            k = kv[n, : mask.shape[1], :W][keep][:, c].astype(np.float64)
            v = kv[n, : mask.shape[1], W:][keep][:, c].astype(np.float64)
            s = k @ q[n, c].astype(np.float64) / np.sqrt(dk)
            p = np.exp(s - s.max())
            out[n, c] = (p / p.sum()) @ v
    return out


def _launch(dev, dk, klen, mask, masked=True, poison=True):
    q, kv = _inputs(dk)
    W = H * dk
    kvp = kv.copy()
    if poison:
        kvp[:, klen:] = np.nan
        kvp[:, :klen][~mask.astype(bool)] = np.nan
    qd, kvd = torch.tensor(q, device=dev), torch.tensor(kvp, device=dev)
    out = torch.full((N, W), 7.0, dtype=torch.float32, device=dev)
    idx = K.DecodeIndex(np.arange(N), klen, dev)
    args = (qd, W, 0, kvd, 2 * W, TK * 2 * W, 0, kvd, 2 * W, TK * 2 * W, W, out, W, 0, idx)
    if masked:
        K.decode_attn_masked(*args, torch.tensor(mask, device=dev), H, dk, N, TK)
    else:
        K.decode_attn(*args, H, dk, N, TK)
    return out.cpu().numpy()


@pytest.mark.parametrize("dk", [16, 32, 64])
@pytest.mark.parametrize("klen", KLENS)
def test_masked_decode_attn(dev, dk, klen):
    q, kv = _inputs(dk)
    ones = _mask("ones", klen, 0)
    plain = _launch(dev, dk, klen, ones, masked=False)
    base = float(np.abs(plain - _reference(q, kv, ones, dk)).max())
    gate = max(2 * base, 1e-6)
    for i, kind in enumerate(MASKS):
        if kind == "chunk1_off" and klen <= 64:
            continue  # no second chunk
        mask = _mask(kind, klen, 100 * dk + klen + i)
        assert mask.any(axis=1).all()
        got = _launch(dev, dk, klen, mask)
        assert np.isfinite(got).all(), (kind, "NaN / Inf: a masked key was read, or exp(-inf - -inf) formed")
        if kind == "ones":
            assert np.array_equal(got, plain), "an all-ones mask must equal esp_decode_attn bit for bit"
            assert torch.equal(torch.tensor(got), torch.tensor(plain))
        err = float(np.abs(got - _reference(q, kv, mask, dk)).max())
        print(f"dk={dk} klen={klen} {kind}: max abs err {err:.3e} (unmasked kernel {base:.3e}, gate {gate:.3e})")
        assert err <= gate, (kind, err, gate)


def test_mask_rows_may_be_wider_than_klen(dev):
    """The mask of a longer prefix, read through its row pitch (the LM's catch-up steps)."""
    dk, klen = 16, 65
    q, kv = _inputs(dk)
    wide = _mask("random", 130, 5)
    W = H * dk
    kvp = kv.copy()
    kvp[:, klen:] = np.nan
    qd, kvd = torch.tensor(q, device=dev), torch.tensor(kvp, device=dev)
    out = torch.empty(N, W, dtype=torch.float32, device=dev)
    K.decode_attn_masked(qd, W, 0, kvd, 2 * W, TK * 2 * W, 0, kvd, 2 * W, TK * 2 * W, W, out, W, 0,
                         K.DecodeIndex(np.arange(N), klen, dev), torch.tensor(wide, device=dev)[:, :klen], H, dk, N, TK)
    want = _reference(q, kv, wide[:, :klen], dk)
    # masked keys are finite here (only keys beyond klen are NaN): 1e-4, the standing fp32-vs-fp64 kernel gate
    assert float(np.abs(out.cpu().numpy() - want).max()) <= 1e-4
