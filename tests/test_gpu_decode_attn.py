"""esp_decode_attn (csrc/decode_attn.hip), the single-query attention of the cached decoder step, against an fp64
numpy restatement on unit-normal inputs.  Gate: atol 1e-4, the standing gate for fp32 kernels against fp64
(tests/test_gpu_inference.py).  Every source sequence has its own length (1, 2, one below / at / above the kernel's
64-key chunk, 374, and a short one), so a launch mixes lengths; rows pick sources with repeats and out of order;
K and V sit in one fused buffer behind column offsets; everything past a source's length is NaN, so a read of a
key at or beyond klen shows up as a non-finite output."""
import numpy as np
import pytest
import torch

from espnet_slurp_amd import _native
from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

H = 4
CH = K.DECODE_ATTN_CHUNK
SRC_LEN = np.array([1, 2, CH - 1, CH, CH + 1, 374, 17], dtype=np.int32)
TK = 376
ROWS = {1: None, 5: [5, 0, 5, 2, 3], 37: None}


def _case(dk, seed=0):
    """Fused K|V buffer (nsrc, TK, ld) with K at column 8 and V at 8 + H*dk + 4, NaN past each source's length."""
    rng = np.random.RandomState(seed)
    W = H * dk
    ld, koff, voff = 8 + W + 4 + W + 4, 8, 8 + W + 4
    kv = np.full((len(SRC_LEN), TK, ld), np.nan, dtype=np.float32)
    for s, n in enumerate(SRC_LEN):
        kv[s, :n, koff:koff + W] = rng.randn(n, W)
        kv[s, :n, voff:voff + W] = rng.randn(n, W)
    return kv, ld, koff, voff


def _reference(q, kv, koff, voff, src, dk):
    N, W = q.shape
    out = np.zeros((N, W), dtype=np.float64)
    for n in range(N):
        L = SRC_LEN[src[n]]
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            k = kv[src[n], :L, koff:koff + W][:, c].astype(np.float64)
            v = kv[src[n], :L, voff:voff + W][:, c].astype(np.float64)
            s = k @ q[n, c].astype(np.float64) / np.sqrt(dk)
            p = np.exp(s - s.max())
            out[n, c] = (p / p.sum()) @ v
    return out


def _run(dev, dk, src, kv_host, ld, koff, voff, seed):
    rng = np.random.RandomState(seed)
    N, W = len(src), H * dk
    ldq, qoff, ldo, ooff = W + 8, 4, W + 12, 8
    qbuf = rng.randn(N, ldq).astype(np.float32)
    q = torch.tensor(qbuf, device=dev)
    kv = torch.tensor(kv_host, device=dev)
    out = torch.full((N, ldo), 7.0, dtype=torch.float32, device=dev)
    idx = K.DecodeIndex(src, SRC_LEN[src], dev)
    K.decode_attn(q, ldq, qoff, kv, ld, TK * ld, koff, kv, ld, TK * ld, voff, out, ldo, ooff, idx, H, dk,
                  len(SRC_LEN), TK)
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), "a key at or beyond klen was read (NaN poison reached the output)"
    assert (got[:, :ooff] == 7.0).all() and (got[:, ooff + W:] == 7.0).all(), "wrote outside the out columns"
    want = _reference(qbuf[:, qoff:qoff + W], kv_host, koff, voff, src, dk)
    err = np.abs(got[:, ooff:ooff + W] - want).max()
    print(f"decode_attn dk={dk} N={N} max abs err {err:.3e}")
    assert err <= 1e-4, err


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("N", [1, 5, 37])
def test_decode_attn_matches_fp64(dev, dk, N):
    kv, ld, koff, voff = _case(dk)
    if N == 1:  # one row: every length in turn
        for s in range(len(SRC_LEN)):
            _run(dev, dk, np.array([s]), kv, ld, koff, voff, 10 + s)
        return
    src = np.array(ROWS[N]) if ROWS[N] is not None else np.random.RandomState(N).randint(0, len(SRC_LEN), N)
    assert len(set(src.tolist())) < N and (np.diff(src) < 0).any(), "src must repeat and be out of order"
    if N == 37:
        assert set(src.tolist()) == set(range(len(SRC_LEN))), "every length in one launch"
    _run(dev, dk, src, kv, ld, koff, voff, N)


def test_decode_attn_rejects_bad_arguments(dev):
    dk = 16
    W = H * dk
    q = torch.zeros(2, W, device=dev)
    kv = torch.zeros(1, 8, 2 * W, device=dev)
    out = torch.zeros(2, W, device=dev)
    with pytest.raises(_native.NativeError, match=r"\(-1\).*klen"):
        K.decode_attn(q, W, 0, kv, 2 * W, 8 * 2 * W, 0, kv, 2 * W, 8 * 2 * W, W, out, W, 0,
                      K.DecodeIndex([0, 0], [3, 0], dev), H, dk, 1, 8)
    q24 = torch.zeros(2, H * 24, device=dev)
    kv24 = torch.zeros(1, 8, 2 * H * 24, device=dev)
    with pytest.raises(_native.NativeError, match=r"\(-1\).*d_k 24"):
        K.decode_attn(q24, H * 24, 0, kv24, 2 * H * 24, 8 * 2 * H * 24, 0, kv24, 2 * H * 24, 8 * 2 * H * 24, H * 24,
                      torch.zeros(2, H * 24, device=dev), H * 24, 0, K.DecodeIndex([0, 0], [3, 3], dev), H, 24, 1, 8)
    assert float(out.abs().max()) == 0.0
