"""esp_maskctc_init_batch / esp_maskctc_fill_batch (csrc/maskctc.hip) against a NumPy restatement on the same fp32
inputs, and against the single-utterance entry points they share their device bodies with.

Both kernels only select (max, first argmax, rank), so ids, counts, the selected log-probabilities and the pass plan
must be equal exactly; no tolerance is involved.  The one arithmetic step, tok_prob = expf(tok_logp), is compared
bit for bit with esp_maskctc_init's on the same utterance (the same device code), and the mask decisions are checked
as (double)tok_prob < threshold on the kernel's own tok_prob."""
import numpy as np
import pytest
import torch

from espnet_slurp_amd import _native
from espnet_slurp_amd import kernels as K
from tests.test_gpu_maskctc_kernels import _collapse, _fill_np, _frames

pytestmark = pytest.mark.gpu

U, TMAX, V = 5, 37, 11
TLENS = (37, 1, 20, 36, 5)
MASK = V  # <mask> follows the CTC vocabulary


def _i32(a, dev):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)


def _plan(mask_num, n_it):
    """The reference's pass plan (maskctc_model.py:319-323)."""
    num_iter = n_it if mask_num >= n_it > 0 else mask_num
    return num_iter, (mask_num // num_iter if num_iter else 0)


def _init_inputs():
    rng = np.random.Generator(np.random.PCG64(77))
    kinds = ("mixed", "noblank", "blank", "mixed", "noblank")  # utterance 2 is all blank
    lp = np.full((U, TMAX, V), np.nan, dtype=np.float32)  # garbage in the frames beyond tlens
    for u, (T, kind) in enumerate(zip(TLENS, kinds)):
        lp[u, :T] = _frames(T, V, rng, kind)
    return lp


@pytest.mark.parametrize("n_it", [0, 1, 3])
@pytest.mark.parametrize("thr", [0.9, 1.5])  # 1.5: above every probability, every token is masked
def test_init_batch_matches_restatement_and_single(dev, n_it, thr):
    lp = _init_inputs()
    y, tl, tp, counts = K.maskctc_init_batch(torch.from_numpy(lp).to(dev), _i32(TLENS, dev), MASK, thr, n_it)
    assert y.shape == tl.shape == tp.shape == (U, TMAX) and counts.shape == (U, 4) and counts.dtype == torch.int32
    y, tl, tp, counts = y.cpu().numpy(), tl.cpu().numpy(), tp.cpu().numpy(), counts.cpu().numpy()
    seen = set()
    for u, T in enumerate(TLENS):
        toks, logp = _collapse(lp[u, :T])
        L = len(toks)
        y1, tl1, tp1, c1 = K.maskctc_init(torch.from_numpy(lp[u, :T].copy()).to(dev), MASK, thr)
        assert c1.cpu().tolist() == [int(counts[u, 0]), int(counts[u, 1])]
        assert counts[u, 0] == L
        assert tl[u, :L].tobytes() == logp.tobytes() == tl1[:L].cpu().numpy().tobytes()
        assert tp[u, :L].tobytes() == tp1[:L].cpu().numpy().tobytes()
        masked = tp[u, :L].astype(np.float64) < thr
        assert np.array_equal(masked, np.exp(logp).astype(np.float64) < thr)
        assert np.array_equal(y[u, :L], np.where(masked, MASK, toks)) and np.array_equal(y[u, :L], y1[:L].cpu().numpy())
        assert (y[u, L:] == 0).all()  # a fixed valid id beyond L
        mask_num = int(masked.sum())
        if thr > 1.0:
            assert mask_num == L
        assert counts[u].tolist() == [L, mask_num, *_plan(mask_num, n_it)], (u, counts[u], L, mask_num, n_it)
        seen.add((L == 0, mask_num == 0))
    assert (True, True) in seen and (False, False) in seen  # an all-blank utterance and a masked one are in


def test_init_batch_ignores_frames_beyond_tlens(dev):
    """The frames beyond tlens, whatever they hold, change nothing."""
    lp = _init_inputs()
    other = lp.copy()
    for u, T in enumerate(TLENS):
        other[u, T:] = _frames(TMAX, V, np.random.Generator(np.random.PCG64(u)), "noblank")[T:]
    a = K.maskctc_init_batch(torch.from_numpy(lp).to(dev), _i32(TLENS, dev), MASK, 0.9, 3)
    b = K.maskctc_init_batch(torch.from_numpy(other).to(dev), _i32(TLENS, dev), MASK, 0.9, 3)
    ca = a[3].cpu().numpy()
    assert np.array_equal(ca, b[3].cpu().numpy()) and np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())
    for u in range(U):
        L = int(ca[u, 0])
        for x, z in zip(a[1:3], b[1:3]):
            assert x[u, :L].cpu().numpy().tobytes() == z[u, :L].cpu().numpy().tobytes()


# ------------------------------------------------------------------ fill
LMAX, V1 = 70, 12
FMASK = V1 - 1
LS = (70, 1, 33, 64, 65)
NUM_ITER = (3, 1, 0, 2, 3)
ROWS = (4, 0, 3, 1)  # a permuted subset: utterance 2 (no pass) is not in the decoder's batch


def _fill_inputs():
    rng = np.random.Generator(np.random.PCG64(5))
    y0 = np.zeros((U, LMAX + 3), dtype=np.int64)  # a leading dimension above Lmax
    counts = np.zeros((U, 4), dtype=np.int32)
    for u, L in enumerate(LS):
        tok = rng.integers(1, FMASK, size=L)
        masked = rng.random(L) < 0.6
        masked[0] = True
        if L >= 64:
            masked[[3, 40, 63]] = True
        tok[masked] = FMASK
        y0[u, :L] = tok
        y0[u, L:] = FMASK  # beyond L: looks masked, must never be touched
        n = int(masked.sum())
        counts[u] = [L, n, NUM_ITER[u], n // NUM_ITER[u] if NUM_ITER[u] else 0]
        assert NUM_ITER[u] <= n
    logits = []
    for t in range(4):
        lg = rng.standard_normal((len(ROWS), LMAX, V1)).astype(np.float32)
        for a, u in enumerate(ROWS):
            if LS[u] >= 64:
                lg[a, 40, 2] = lg[a, 63, 4] = 40.0  # exact tie of two maxima: the lower index ranks first
                lg[a, 3, FMASK] = 50.0  # this position's argmax is <mask> in every pass: it stays <mask>
        logits.append(lg)
    return y0, counts, logits


def test_fill_batch_follows_each_utterances_plan(dev):
    y0, counts, logits = _fill_inputs()
    y = torch.from_numpy(y0.copy()).to(dev)
    cd, rows = torch.from_numpy(counts).to(dev), _i32(ROWS, dev)
    want = y0.copy()
    for t in range(4):
        K.maskctc_fill_batch(torch.from_numpy(logits[t]).to(dev), y, cd, rows, FMASK, t)
        for a, u in enumerate(ROWS):
            L, n, num_iter, k = (int(v) for v in counts[u])
            if t < num_iter:
                want[u, :L] = _fill_np(logits[t][a, :L], want[u, :L], FMASK, k if t < num_iter - 1 else 0)
        got = y.cpu().numpy()
        assert np.array_equal(got, want), (t, np.argwhere(got != want))
        for u in range(U):
            if LS[u] >= 64:
                assert got[u, 3] == FMASK  # also at t >= num_iter: a later pass does not refill it
    # utterance 3's last pass was t = 1; at t = 2, 3 its row (with the <mask> left at position 3) did not move
    assert want[3, 3] == FMASK and NUM_ITER[3] == 2
    assert np.array_equal(want[2], y0[2])  # never served
    assert np.array_equal(want[:, LMAX:], y0[:, LMAX:])
    for u in range(U):
        assert np.array_equal(want[u, LS[u]:], y0[u, LS[u]:])


def test_fill_batch_tie_takes_lower_index_under_topk(dev):
    """k = 2 with the maxima 50 (position 3, argmax <mask>), 40 (position 40) and 40 (position 63): 3 and 40 rank."""
    y0, counts, logits = _fill_inputs()
    counts = counts.copy()
    counts[:, 2], counts[:, 3] = 5, 2
    y = torch.from_numpy(y0.copy()).to(dev)
    K.maskctc_fill_batch(torch.from_numpy(logits[0]).to(dev), y, torch.from_numpy(counts).to(dev), _i32(ROWS, dev),
                         FMASK, 0)
    got = y.cpu().numpy()
    for a, u in enumerate(ROWS):
        L = LS[u]
        assert np.array_equal(got[u, :L], _fill_np(logits[0][a, :L], y0[u, :L], FMASK, min(2, L)))
        if L >= 64:
            assert got[u, 3] == FMASK and got[u, 40] == 2 and got[u, 63] == FMASK


@pytest.mark.parametrize("T", [1, 37, 300])
def test_single_utterance_batch_equals_old_entry_points(dev, T):
    rng = np.random.Generator(np.random.PCG64(T))
    lp = torch.from_numpy(_frames(T, 37, rng, "noblank" if T == 1 else "mixed")).to(dev)
    y1, tl1, tp1, c1 = K.maskctc_init(lp, 37, 0.9)
    yb, tlb, tpb, cb = K.maskctc_init_batch(lp.unsqueeze(0), _i32([T], dev), 37, 0.9, 3)
    L, n = c1.cpu().tolist()
    assert cb[0, :2].cpu().tolist() == [L, n] and L >= 1
    for a, b in ((y1, yb), (tl1, tlb), (tp1, tpb)):
        assert a[:L].cpu().numpy().tobytes() == b[0, :L].cpu().numpy().tobytes()
    num_iter, k = (int(v) for v in cb[0, 2:].cpu())
    assert (num_iter, k) == _plan(n, 3)
    logits = torch.from_numpy(rng.standard_normal((L, 38)).astype(np.float32)).to(dev)
    rows = _i32([0], dev)
    for t in range(num_iter):
        K.maskctc_fill(logits, y1, 37, k if t < num_iter - 1 else 0)
        K.maskctc_fill_batch(logits.unsqueeze(0), yb, cb, rows, 37, t)
        assert torch.equal(y1[:L], yb[0, :L]), t


def test_bad_sizes_are_refused(dev):
    lp = torch.zeros(2, 4, 5, device=dev)
    with pytest.raises(_native.NativeError, match="esp_maskctc_init_batch: bad sizes"):
        K.maskctc_init_batch(lp, _i32([4, 4], dev), 5, 0.9, 3, blank=5)
    with pytest.raises(_native.NativeError, match="esp_maskctc_init_batch: bad sizes"):
        K.maskctc_init_batch(lp, _i32([4, 4], dev), 5, 0.9, -1)
    counts = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    rows = _i32([0], dev)
    y = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    with pytest.raises(_native.NativeError, match="esp_maskctc_fill_batch: bad sizes"):  # y_in narrower than Lmax
        K.maskctc_fill_batch(torch.zeros(1, 9, 6, device=dev), y, counts, rows, 5, 0)
    with pytest.raises(_native.NativeError, match="esp_maskctc_fill_batch: bad sizes"):
        K.maskctc_fill_batch(torch.zeros(1, 8, 6, device=dev), y, counts, rows, 5, -1)
    wide = torch.zeros(2, K.MASKCTC_FILL_MAX_L + 1, dtype=torch.int64, device=dev)
    with pytest.raises(_native.NativeError, match="esp_maskctc_fill_batch: bad sizes"):  # above the LDS ranking
        K.maskctc_fill_batch(torch.zeros(1, K.MASKCTC_FILL_MAX_L + 1, 2, device=dev), wide, counts, rows, 1, 0)
