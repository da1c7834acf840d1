"""Host-side parts of the cached decoder on CPU: esp_decode_attn's argument checks (they run before any launch,
so the library answers without a GPU), the DecoderCache bookkeeping (doubling growth, reorder, select) on CPU
tensors, the pinned-rank rule on the committed BatchBeamSearch fixture, and tools/bench_decode.py's trace split."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from espnet_slurp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load()


def _decode_attn(lib, src, klen, dk, ldk=128, koff=0, nsrc=2, Tk=8):
    idx = np.array(list(src) + list(klen), dtype=np.int32)
    a = 1 << 12  # an aligned, never dereferenced address: every case below fails its check before the launch
    rc = lib.esp_decode_attn(a, 64, 0, a, ldk, Tk * ldk, koff, a, ldk, Tk * ldk, 64, a, 64, 0, idx.ctypes.data, a,
                             len(src), 64 // dk if 64 % dk == 0 else 2, dk, nsrc, Tk, None)
    return rc, lib.esp_last_error().decode()


def test_decode_attn_argument_checks():
    lib = _lib()
    for args, word in ((dict(src=[0, 1], klen=[3, 0], dk=16), "klen[1] = 0"),
                       (dict(src=[0, 1], klen=[3, 9], dk=16), "klen[1] = 9"),
                       (dict(src=[0, 2], klen=[3, 3], dk=16), "src[1] = 2"),
                       (dict(src=[0], klen=[3], dk=24), "d_k 24"),
                       (dict(src=[0], klen=[3], dk=16, koff=2), "16-byte"),
                       (dict(src=[0], klen=[3], dk=16, ldk=100), "leading dimension")):
        rc, msg = _decode_attn(lib, **args)
        assert rc == -1 and word in msg, (args, rc, msg)


def test_decoder_cache_grows_by_doubling_and_reorders():
    from espnet_slurp_amd.asr.decoder.transformer_decoder import DecoderCache
    c = DecoderCache(2, 4, "cpu", rows=3, capacity=8)
    assert c.buf.shape == (2, 3, 8, 8) and c.len == 0 and c.n == 3
    c.ensure(3, 5)
    c.buf[:, :3, :5] = torch.arange(2 * 3 * 5 * 8, dtype=torch.float32).view(2, 3, 5, 8)
    c.len = 5
    before = c.buf[:, :3, :5].clone()
    c.ensure(3, 9)
    assert c.capacity == 16 and torch.equal(c.buf[:, :3, :5], before)
    c.ensure(3, 33)
    assert c.capacity == 64
    sel = c.select([2, 0])
    assert sel.n == 2 and sel.len == 5 and torch.equal(sel.buf[:, :, :5], before[:, [2, 0]])
    c.reorder([2, 2, 0, 1, 1])  # longer than the row count: the rows double to 6
    assert c.n == 5 and c.row_capacity == 6 and torch.equal(c.buf[:, :5, :5], before[:, [2, 2, 0, 1, 1]])
    c.reorder(torch.tensor([4]))
    assert c.n == 1 and torch.equal(c.buf[:, :1, :5], before[:, [1]])


def test_batch_fixture_pins_the_ranks_where_batch_and_plain_differ():
    """The committed reference BatchBeamSearch results: twice the 1e-3 relative allowance separates ranks 1-6 of
    fixture a (ranks 4-6 are where the batch and the plain reference differ), rank 1 of b and none of c."""
    g = golden("inference")

    def pinned(s):
        return [i for i in range(len(s))
                if all(abs(s[i] - s[j]) > 2e-3 * abs(s[i]) for j in (i - 1, i + 1) if 0 <= j < len(s))]
    assert pinned(g["bs_a_batch_score"]) == [0, 1, 2, 3, 4, 5]
    assert pinned(g["bs_b_batch_score"]) == [0] and pinned(g["bs_c_batch_score"]) == []
    plain = [y[y >= 0].tolist() for y in g["bs_a_plain_yseq"]]
    batch = [y[y >= 0].tolist() for y in g["bs_a_batch_yseq"]]
    assert plain[:3] == batch[:3] and all(plain[i] != batch[i] for i in (3, 4, 5))


def test_bench_decode_splits_a_trace_into_self_and_source(tmp_path):
    rows = ["Kernel_Name,Start_Timestamp,End_Timestamp"]
    t = 1000
    for step in range(2):
        for layer in range(6):
            for dur in (2000, 5000):  # self, then source
                rows.append(f'"void (anonymous namespace)::decode_attn_kernel<64>(float const*)",{t},{t + dur}')
                t += 10000
            rows.append(f'"gemm_kernel",{t},{t + 1000}')
            t += 10000
    p = tmp_path / "x_kernel_trace.csv"
    p.write_text("\n".join(rows) + "\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_decode.py"), "--analyze-trace", str(p),
                          "--utts", "2"], capture_output=True, text=True, check=True).stdout
    r = json.loads(out)
    assert r["decode_attn_launches"] == 24 and r["self"]["launches"] == 12 and r["source"]["launches"] == 12
    assert r["self"]["mean_us"] == 2.0 and r["source"]["mean_us"] == 5.0
    # source, step 0 (2 rows) and step 1 (40 rows) over 374 keys of D = 256, K and V, plus q and out
    req = 6 * ((2 + 40) * 374 * 256 * 8 + 2 * (2 + 40) * 256 * 4)
    assert abs(r["source"]["requested_GBps"] - req / (12 * 5e-6) / 1e9) < 0.1
