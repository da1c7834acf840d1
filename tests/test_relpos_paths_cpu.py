"""kernels.relpos_attn_paths: the rel-pos attention path table, written out here independently of the function
(all 32 flag settings x latest / legacy / legacy length-bucketed x fp32 / bf16 compute x the shapes at which a
predicate flips).  No GPU: the native library loads lazily and nothing here calls into it."""
import itertools

import pytest

from espnet_slurp_amd import kernels as K

FLAGS = ("FLASH_ATTN", "ATTN_FWD32", "FUSED_ATTN_BWD", "ATTN_DSCORES", "RELPOS_BWD_DS")
# (T, d_k): fits the 32-row-block kernels (T <= 449), fits the dS-only backward (T <= 480), fits the
# probabilities / flash kernels (T <= 512) -- each only at d_k 64
SHAPES = {
    (374, 64): (True, True, True),     # the workload shape
    (449, 64): (True, True, True),     # the last T for which the fused forms fit
    (450, 64): (False, True, True),    # the first T for which they do not
    (480, 64): (False, True, True),    # the last T for the dS-only backward
    (481, 64): (False, False, True),   # just past it
    (512, 64): (False, False, True),   # the probabilities kernel's limit
    (513, 64): (False, False, False),  # just past that limit
    (100, 32): (False, False, False),  # d_k is not 64
}


def _expected(flags, fits, legacy, bucketed, fp32):
    flash, fwd32, fused_bwd, dscores, bwd_ds = flags
    fits32, fits_ds, fits512 = fits
    if flash and fits512 and not bucketed:
        return "flash", "flash", dscores
    if fits512 and not fwd32:
        fwd = "probs"
    elif not legacy and fits32:
        fwd = "block32"
    else:
        fwd = "gemm"
    if not legacy and bwd_ds and fits_ds and not fused_bwd and not dscores and fp32:
        bwd = "ds"
    elif not legacy and fits32 and fused_bwd:
        bwd = "fused"
    elif dscores and not bucketed:
        bwd = "dscores"
    else:
        bwd = "rowpass"
    return fwd, bwd, dscores or bwd == "ds"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_relpos_attn_paths_table(monkeypatch, mode):
    monkeypatch.setattr(K, "_COMPUTE", [K.GEMM_FP32 if mode == "fp32" else K.GEMM_BF16])
    n = 0
    for flags in itertools.product([False, True], repeat=5):
        for name, v in zip(FLAGS, flags):
            monkeypatch.setattr(K, name, v)
        for (T, dk), fits in SHAPES.items():
            for legacy, bucketed in ((False, False), (True, False), (True, True)):
                got = K.relpos_attn_paths(T, dk, legacy, bucketed)
                assert got == _expected(flags, fits, legacy, bucketed, mode == "fp32"), (flags, T, dk, legacy, bucketed)
                assert isinstance(got[2], bool)
                n += 1
    assert n == 32 * 8 * 3


def test_relpos_attn_paths_defaults():
    """The shipped flags: the workload shape takes the probabilities kernel and the dS-only backward with an fp32
    ctx (latest), the row-wise pass with ctx planes (legacy)."""
    assert [getattr(K, f) for f in FLAGS] == [False, False, False, False, True]
    assert K._COMPUTE[0] == K.GEMM_FP32
    assert K.relpos_attn_paths(374, 64, False, False) == ("probs", "ds", True)
    assert K.relpos_attn_paths(374, 64, True, False) == ("probs", "rowpass", False)
    assert K.relpos_attn_paths(374, 64, True, True) == ("probs", "rowpass", False)
    assert K.relpos_attn_paths(875, 64, False, False) == ("gemm", "rowpass", False)


def test_relpos_attn_paths_reads_replaced_predicates(monkeypatch):
    """Tests switch the fused kernels off by replacing the predicates on the module: the table must see that."""
    monkeypatch.setattr(K, "relpos_fused_ok", lambda T, dk: False)
    monkeypatch.setattr(K, "relpos_probs_ok", lambda T, dk: False)
    assert K.relpos_attn_paths(100, 64, False, False) == ("gemm", "ds", True)
    monkeypatch.setattr(K, "FUSED_ATTN_BWD", True)
    assert K.relpos_attn_paths(100, 64, False, False) == ("gemm", "rowpass", False)
