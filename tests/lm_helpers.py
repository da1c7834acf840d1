"""Shared pieces of the LM tests: the small LMs of tests/golden/lm.npz (make_lm_golden.py) built from the fixture's
parameters, and the prefix history of the stepped batch_score check (the reorder pattern of test_gpu_decoder_step)."""
import functools
import json

import torch

from tests.helpers import golden

V = 32
LM_CFGS = dict(A=dict(pos_enc=None, embed_unit=16, att_unit=64, head=2, unit=96, layer=2, dropout_rate=0.0),
               B=dict(pos_enc="sinusoidal", embed_unit=16, att_unit=64, head=4, unit=96, layer=2, dropout_rate=0.0),
               C=dict(pos_enc=None, embed_unit=16, att_unit=128, head=2, unit=64, layer=1, dropout_rate=0.0))
TRANSFORMER2 = dict(pos_enc=None, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16, dropout_rate=0.1)
CHECK = (1, 2, 16, 17, 63, 64, 65, 66)
PARENTS = [3, 3, 0, 1, 4]
REORDER_AFTER = (5, 40)
LMAX = 66


@functools.lru_cache(maxsize=None)
def lm_golden():
    return golden("lm")


def golden_keys():
    return json.loads(str(lm_golden()["keys_json"]))


def golden_state(tag):
    g = lm_golden()
    pre = f"{tag}.p."
    return {k[len(pre):]: torch.tensor(g[k]) for k in g if k.startswith(pre)}


def build_lm(tag, device=None):
    """TransformerLM `tag` with the fixture's parameters, in eval mode (flattened on `device` when one is given)."""
    from espnet_slurp_amd.lm import TransformerLM
    lm = TransformerLM(V, **LM_CFGS[tag])
    lm.load_state_dict(golden_state(tag), strict=True)
    lm.eval()
    if device is not None:
        lm = lm.to(device)
        lm.flatten()
    return lm


def history():
    """{L: (5, L) prefixes} for L = 1..LMAX: column L-1 comes from bs_toks, rows are reordered by PARENTS after the
    lengths in REORDER_AFTER (as make_lm_golden.history)."""
    toks = torch.tensor(lm_golden()["bs_toks"])
    ys, hist = toks.clone(), {}
    for L in range(1, LMAX + 1):
        ys[:, L - 1] = toks[:, L - 1]
        hist[L] = ys[:, :L].clone()
        if L in REORDER_AFTER:
            ys = ys[PARENTS].clone()
    return hist
