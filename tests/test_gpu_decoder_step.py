"""The cached one-step decoder (TransformerDecoder.prepare_memory / forward_one_step / score / batch_score) against
an fp64 run of oracle.espnet_cpu.decoder on the same parameters.

Two models: tests/helpers.small_cfg (D=64, H=4: d_k 16, 2 layers, V=32) and one with d_k 64 (D=128, H=2, 1 layer).
U=2 memories of lengths 59 and 41, N=5 decode rows over them, stepped L=1..66 from a cache of capacity 8 (it
doubles to 16, 32, 64, 128) with the rows reordered by the parent index [3, 3, 0, 1, 4] after two of the steps.

Gate at L in {1, 2, 16, 17, 63, 64, 65, 66}: the cached step's log-probabilities may be at most twice as far from
the fp64 run as the existing full-prefix TransformerDecoder.forward + log_softmax is (same arithmetic, another
summation order); both errors are taken as the maximum over the checked lengths and printed."""
import functools

import numpy as np
import pytest
import torch

from espnet_slurp_amd import kernels as K
from espnet_slurp_amd.asr.decoder.transformer_decoder import DecoderCache, RowState
from oracle import espnet_cpu as O
from tests.helpers import build_model, load_seeded, small_cfg

pytestmark = pytest.mark.gpu

CHECK = (1, 2, 16, 17, 63, 64, 65, 66)
PARENTS = [3, 3, 0, 1, 4]
REORDER_AFTER = (5, 40)
HLENS = [59, 41]
LMAX = 66


def _cfg(which):
    if which == "dk16":
        return small_cfg("latest", D=64, blocks=2, V=32)
    return O.ModelCfg(vocab_size=32, enc=O.EncCfg(output_size=128, attention_heads=2, linear_units=128, num_blocks=1),
                      dec=O.DecCfg(attention_heads=2, linear_units=128, num_blocks=1), ctc_weight=0.3, lsm_weight=0.1)


@functools.lru_cache(maxsize=None)
def _setup(which):
    """Model parameters, inputs, the row history under the reorders, and the fp64 log-probabilities at CHECK."""
    cfg = _cfg(which)
    D, V = cfg.enc.output_size, cfg.vocab_size
    g = torch.Generator().manual_seed(3)
    hs = torch.randn(2, max(HLENS), D, generator=g)
    toks = torch.randint(1, V - 1, (5, LMAX), generator=g)
    P64 = {k: v.double() for k, v in O.deterministic_params(cfg, 17).items()}
    ys, rows = toks.clone(), np.array([0, 0, 0, 1, 1])
    hist, want = {}, {}
    for L in range(1, LMAX + 1):
        ys[:, L - 1] = toks[:, L - 1]
        hist[L] = (ys[:, :L].clone(), rows.copy())
        if L in CHECK:
            logits = O.decoder(P64, hs[rows].double(), torch.tensor(HLENS)[rows], ys[:, :L],
                               torch.full((5,), L), cfg.dec, training=False)
            want[L] = torch.log_softmax(logits[:, -1], -1).numpy()
        if L in REORDER_AFTER:
            ys, rows = ys[PARENTS].clone(), rows[PARENTS]
    return cfg, hs, hist, want


def _decoder(which, dev):
    cfg = _setup(which)[0]
    model = build_model(cfg, dev, dropout=0.0)
    load_seeded(model, cfg, 17)
    model.eval()
    return model.decoder


@pytest.mark.parametrize("which", ["dk16", "dk64"])
def test_cached_step_matches_fp64(dev, which):
    cfg, hs, hist, want = _setup(which)
    dec = _decoder(which, dev)
    mem = dec.prepare_memory(hs.to(dev), HLENS)
    cache = dec.init_cache(5, capacity=8)
    grown = set()
    e_step, e_full = {}, {}
    for L in range(1, LMAX + 1):
        ys, rows = hist[L]
        logp, cache = dec.forward_one_step(ys, None, (mem, rows), cache=cache)
        grown.add(cache.capacity)
        assert logp.shape == (5, cfg.vocab_size) and cache.len == L
        if L in CHECK:
            e_step[L] = float(np.abs(logp.cpu().numpy() - want[L]).max())
            logits, _ = dec(hs[rows].to(dev), torch.tensor(HLENS)[rows], ys, torch.full((5,), L))
            last = logits[:, -1].contiguous()
            full = torch.empty_like(last)
            K.log_softmax(last, full, 5, last.shape[1])
            e_full[L] = float(np.abs(full.cpu().numpy() - want[L]).max())
        if L in REORDER_AFTER:
            cache.reorder(PARENTS)
    assert grown == {8, 16, 32, 64, 128}, grown
    msg = (f"{which}: cached step max err {max(e_step.values()):.3e} vs full-prefix forward {max(e_full.values()):.3e}; "
           f"per L step {e_step} full {e_full}")
    print(msg)
    assert max(e_step.values()) <= 2 * max(e_full.values()), msg


def test_batch_score_forms_agree(dev):
    """batch_score with the reference's list-of-states arguments, and with a plain (N, T, D) memory, against the
    batched call.  List form: the same kernels on the same rows, the cache only gathered another way; the gate
    is one fp32 rounding of a log-probability of magnitude < 8 (4.8e-7), in case a GEMM splits differently.
    Plain memory: the K/V projection runs over N*T instead of U*T rows, which may change its GEMM's tiling and
    so the order of D = 64 fp32 additions; through two layers that stays below 1e-5 on the log-probabilities."""
    cfg, hs, hist, _ = _setup("dk16")
    dec = _decoder("dk16", dev)
    full = [59, 59]  # a plain memory has no lengths: compare on memories used in full
    mem = dec.prepare_memory(hs.to(dev), full)
    cache, states, plain = None, [None] * 5, None
    for L in range(1, 9):
        ys, rows = hist[L]
        logp, cache = dec.batch_score(ys, cache, (mem, rows))
        assert isinstance(cache, DecoderCache)
        got, states = dec.batch_score(ys, states, (mem, rows))
        assert isinstance(states, list) and all(isinstance(s, RowState) for s in states)
        d = float((got - logp).abs().max())
        assert d <= 4.8e-7, (L, d)
        got, plain = dec.batch_score(ys, plain, hs[rows].to(dev))
        d = float((got - logp).abs().max())
        print(f"L={L} plain-memory diff {d:.3e}")
        assert d <= 1e-5, (L, d)
        if L in REORDER_AFTER:
            cache.reorder(PARENTS)
            states = [states[p] for p in PARENTS]
            plain.reorder(PARENTS)
    # score(): one hypothesis, the reference's argument order
    ys, rows = hist[3]
    st = None
    for L in range(1, 4):
        lp1, st = dec.score(ys[0, :L], st, hs[rows[0]].to(dev))
    lp, _ = dec.batch_score(ys, None, (mem, rows))
    assert float((lp1 - lp[0]).abs().max()) <= 1e-5


def test_step_is_eval_only(dev):
    cfg, hs, hist, _ = _setup("dk16")
    dec = _decoder("dk16", dev)
    mem = dec.prepare_memory(hs.to(dev), HLENS)
    dec.train()
    ys, rows = hist[1]
    with pytest.raises(RuntimeError):
        dec.forward_one_step(ys, None, (mem, rows))
    with pytest.raises(RuntimeError):
        dec.batch_score(ys, None, (mem, rows))
    with pytest.raises(RuntimeError):
        dec.prepare_memory(hs.to(dev), HLENS)
