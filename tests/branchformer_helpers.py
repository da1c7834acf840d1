"""Shared by tests/golden/make_branchformer_golden.py (fixture generation, reference side) and the Branchformer
tests (this package's side): the configurations of the fixtures, the seeded parameter fill, and the
argparse.Namespace that tasks.asr.build_model reads.  Imports nothing of the reference."""
import argparse
import contextlib
import copy
import json
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def token_list(V):
    return ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]


def small_conf(U=96, k=31, rel_pos_type="latest", use_attn=True, dropout=0.0, V=32):
    """The small Branchformer model of the fixtures: D=64, 4 heads, 2 blocks, decoder as helpers.small_cfg."""
    return dict(
        input_size=80, token_list_size=V, encoder="branchformer",
        encoder_conf=dict(output_size=64, use_attn=use_attn, attention_heads=4, attention_layer_type="rel_selfattn",
                          pos_enc_layer_type="rel_pos", rel_pos_type=rel_pos_type, use_cgmlp=True,
                          cgmlp_linear_units=U, cgmlp_conv_kernel=k, use_linear_after_conv=False,
                          gate_activation="identity", merge_method="concat", num_blocks=2, dropout_rate=dropout,
                          positional_dropout_rate=dropout, attention_dropout_rate=dropout, input_layer="conv2d",
                          stochastic_depth_rate=0.0),
        decoder="transformer",
        decoder_conf=dict(attention_heads=4, linear_units=128, num_blocks=2, dropout_rate=dropout,
                          positional_dropout_rate=dropout, self_attention_dropout_rate=dropout,
                          src_attention_dropout_rate=dropout),
        model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
        normalize="utterance_mvn", normalize_conf={}, ctc_conf={}, specaug=None, specaug_conf={})


# name -> (conf, B, T, lens, ulens, seed)
SMALL_FIXTURES = {
    "branchformer_small_k31": (small_conf(96, 31, "latest"), 3, 120, [120, 97, 64], [9, 5, 7], 78),
    "branchformer_small_k7_legacy": (small_conf(128, 7, "legacy"), 3, 300, [300, 211, 150], [9, 5, 7], 74),
    "branchformer_cgmlp_only": (small_conf(96, 31, "latest", use_attn=False), 3, 120, [120, 97, 64], [9, 5, 7], 76),
}
RECIPE_B2 = dict(name="branchformer_slurp_entity_b2", B=2, T=400, lens=[400, 333], ulens=[11, 7], seed=75,
                 num_blocks=2)


def load_fixture(name):
    """NAME.npz merged with its NAME.partK.npz files (the gradient tensors, split so that no file passes 1 MiB)."""
    out = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    k = 0
    while os.path.exists(os.path.join(GOLDEN, f"{name}.part{k}.npz")):
        out.update(np.load(os.path.join(GOLDEN, f"{name}.part{k}.npz"), allow_pickle=False))
        k += 1
    return out


@contextlib.contextmanager
def recorded_pos_table(g, conf, device):
    """Give the model under test the positional table of the fixture's reference run (g["pos_emb"]).

    The table is sin / cos of position * exp(-2i ln(1e4) / d), built on the host in fp32 exactly as the reference
    builds it (abs_encoder.pos_table).  torch's fp32 exp differs in the last bit between hosts for a few of the d / 2
    frequencies, and the position amplifies that bit: up to 5000 x in the legacy table, where one ulp moves two
    columns of the table by 1e-4 -- and with them linear_pos's weight gradient, above the tests' gate.  The table
    is a constant input of the model, like the batch, so the fixture records the one its run used and the test
    installs it in pos_table's cache for the duration of the block; it must agree with this host's own table to the
    size of that effect."""
    from espnet_slurp_amd.asr.encoder import abs_encoder as AE
    e = conf["encoder_conf"]
    kind = e.get("rel_pos_type", "latest")
    tab = torch.from_numpy(np.ascontiguousarray(g["pos_emb"]))
    D = e["output_size"]
    T = tab.shape[0] if kind == "legacy" else (tab.shape[0] + 1) // 2
    own = AE.pos_table(kind, T, D, "cpu")
    assert own.shape == tab.shape and float((own - tab).abs().max()) < 1e-3
    key = (kind, T, D, str(torch.device(device)), 5000)
    prev = AE._PE_CACHE.get(key)
    AE._PE_CACHE[key] = tab.to(device)
    try:
        yield
    finally:
        if prev is None:
            del AE._PE_CACHE[key]
        else:
            AE._PE_CACHE[key] = prev


def recipe_config():
    """egs2/slurp_entity/asr1's Branchformer training config as resolved values (settings only; written by
    tests/golden/make_branchformer_golden.py from the recipe YAML)."""
    with open(os.path.join(GOLDEN, "branchformer_slurp_entity.json")) as f:
        return json.load(f)


def recipe_b2_conf(conf):
    """The recipe's widths with num_blocks 2, every dropout 0 and SpecAug off (the b2 fixture's model)."""
    conf = copy.deepcopy(conf)
    for sec in ("encoder_conf", "decoder_conf"):
        for k in conf[sec]:
            if k.endswith("dropout_rate"):
                conf[sec][k] = 0.0
    conf["encoder_conf"]["num_blocks"] = RECIPE_B2["num_blocks"]
    conf["specaug"] = None
    return conf


def args_from_conf(conf, dropout=None):
    """argparse.Namespace with the fields ASRTask.build_model reads (asr.py:439-562)."""
    conf = copy.deepcopy(conf)
    if dropout is not None:
        for sec in ("encoder_conf", "decoder_conf"):
            for k in conf[sec]:
                if k.endswith("dropout_rate") and k != "stochastic_depth_rate":
                    conf[sec][k] = dropout
    return argparse.Namespace(
        token_list=token_list(conf["token_list_size"]), input_size=conf["input_size"], frontend=None, frontend_conf={},
        specaug=conf.get("specaug"), specaug_conf=conf.get("specaug_conf") or {}, normalize=conf["normalize"],
        normalize_conf=conf["normalize_conf"], preencoder=None, encoder=conf["encoder"],
        encoder_conf=conf["encoder_conf"], postencoder=None, decoder=conf["decoder"],
        decoder_conf=conf["decoder_conf"], ctc_conf=conf["ctc_conf"], model="espnet", model_conf=conf["model_conf"],
        init=None)


def seeded_params(shapes, seed, dtype=torch.float32):
    """A non-degenerate parameter fill from the (key, shape) list of a state_dict alone: each tensor drawn in
    fp64 from its own generator keyed by (seed, key), then cast.  Weights are N(0, 1) / sqrt(fan-in) (the
    depthwise convolution's fan-in is its k taps, so the gate varies along time and the convolution path
    shows -- the reference's own 1e-6 initialisation makes the gate a constant), LayerNorm weights
    1 + 0.1 N(0, 1), biases 0.1 N(0, 1), the gate convolution's bias 1 + 0.1 N(0, 1)."""
    out = {}
    for key, shape in shapes:
        shape = tuple(int(s) for s in shape)
        g = np.random.Generator(np.random.PCG64([seed, zlib.crc32(key.encode())]))
        x = g.standard_normal(shape)
        leaf = key.rsplit(".", 1)[-1]
        if "norm" in key and leaf == "weight":
            x = 1.0 + 0.1 * x
        elif key.endswith("csgu.conv.bias"):
            x = 1.0 + 0.1 * x
        elif len(shape) == 1:
            x = 0.1 * x
        else:  # (out, in, ...) weights, embeddings (V, D), pos_bias_u / v (h, d_k)
            x = x / np.sqrt(float(np.prod(shape[1:])))
        out[key] = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return out


def state_shapes(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def load_seeded(model, seed):
    """Fill `model` (this package's or the reference's: same keys and shapes) from seeded_params."""
    sd = model.state_dict()
    P = seeded_params([(k, tuple(v.shape)) for k, v in sd.items()], seed, next(model.parameters()).dtype)
    model.load_state_dict(P, strict=True)
    return P
