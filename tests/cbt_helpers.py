"""Shared by tests/golden/make_cbt_golden.py (fixture generation, reference side) and the contextual block
Transformer tests (this package's side): the fixtures' configurations and inputs.  Imports nothing of the reference.
Parameters come from branchformer_helpers.seeded_params (regenerated from a seed, not stored)."""
import json
import os

import numpy as np
import torch

from tests import branchformer_helpers as BH

GOLDEN = BH.GOLDEN
LAYOUT_CASES = {"8/3/3": (8, 3, 3, [9, 11, 12, 13, 20, 29]), "40/16/16": (40, 16, 16, [41, 56, 57, 75, 374])}


def encoder_conf(D=32, heads=2, units=48, blocks=3, bs=8, hop=3, la=3, ctx_pos_enc=True, dropout=0.0):
    return dict(output_size=D, attention_heads=heads, linear_units=units, num_blocks=blocks, dropout_rate=dropout,
                positional_dropout_rate=dropout, attention_dropout_rate=dropout, input_layer="conv2d",
                normalize_before=True, block_size=bs, hop_size=hop, look_ahead=la, init_average=True,
                ctx_pos_enc=ctx_pos_enc)


INPUT_SIZE = 20  # feature bins of the encoder-only fixtures (conv2d: 4 bins after subsampling)


def _lens(T):
    return [T, T - 5, T - 11]


# encoder-only fixtures: name -> (encoder_conf, T', lengths, seed).  T = 4 T' + 3 feature frames, B = 3, unequal
# lengths.  T' 9: two blocks, the second partial; 11: the last block exactly full; 12 / 13: three blocks, one and two
# frames past a hop; 8: T' <= block_size, the plain stack with the pad mask
ENC_FIXTURES = {
    "cbt_enc_t9": (encoder_conf(), 9, _lens(39), 91),
    "cbt_enc_t11": (encoder_conf(), 11, _lens(47), 92),
    "cbt_enc_t12": (encoder_conf(), 12, _lens(51), 93),
    "cbt_enc_t13": (encoder_conf(), 13, _lens(55), 94),
    "cbt_enc_t13_noctxpe": (encoder_conf(ctx_pos_enc=False), 13, _lens(55), 95),
    "cbt_enc_t8_short": (encoder_conf(), 8, _lens(35), 96),
    # block_size 64: S = 66 slots, above the fused attention's 64 -- block mode on the generic attention kernels
    "cbt_enc_bs64": (encoder_conf(bs=64, hop=24, la=24), 70, _lens(283), 99),
}
# one case at S = 42, d_k = 64 (the recipe's block shape): gradient norms and a 16-element slice per tensor
S42 = dict(name="cbt_enc_s42", conf=encoder_conf(D=128, heads=2, units=256, blocks=2, bs=40, hop=16, la=16), T2=75,
           lens=[303, 280], seed=97)


def model_conf(dropout=0.0, V=32):
    """The small whole model: this encoder (3 layers, D = 32) + a 1-block decoder + CTC."""
    return dict(
        input_size=80, token_list_size=V, encoder="contextual_block_transformer", encoder_conf=encoder_conf(dropout=dropout),
        decoder="transformer",
        decoder_conf=dict(attention_heads=2, linear_units=48, num_blocks=1, dropout_rate=dropout,
                          positional_dropout_rate=dropout, self_attention_dropout_rate=dropout,
                          src_attention_dropout_rate=dropout),
        model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
        normalize="utterance_mvn", normalize_conf={}, ctc_conf={}, specaug=None, specaug_conf={})


# name -> (conf, B, T, lens, ulens, seed): T = 55 frames -> T' = 13, three blocks
MODEL_FIXTURE = ("cbt_model_small", model_conf(), 3, 55, [55, 50, 44], [4, 2, 3], 98)


def enc_inputs(T, lens, seed, input_size=INPUT_SIZE, D=32, T2=None):
    """Seeded features (zero past each utterance's length) and a fixed random cotangent for the encoder output."""
    rng = np.random.Generator(np.random.PCG64(seed))
    feats = rng.standard_normal((len(lens), T, input_size)).astype(np.float32)
    for i, l in enumerate(lens):
        feats[i, l:] = 0.0
    T2 = ((T - 3) // 2 + 1 - 3) // 2 + 1 if T2 is None else T2
    cot = rng.standard_normal((len(lens), T2, D)).astype(np.float32)
    return torch.from_numpy(feats), torch.tensor(lens, dtype=torch.long), torch.from_numpy(cot)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def load_json(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)
