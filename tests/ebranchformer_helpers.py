"""Shared by tests/golden/make_ebranchformer_golden.py (fixture generation, reference side) and the E-Branchformer
tests (this package's side): the fixture table.  The seeded parameter fill, the argparse.Namespace for
tasks.asr.build_model and the fixture loader are tests/branchformer_helpers.py's.  Imports nothing of the reference."""
from tests.branchformer_helpers import (args_from_conf, load_fixture, load_seeded, recorded_pos_table,  # noqa: F401
                                        seeded_params, small_conf as _bf_conf, state_shapes, token_list)


def small_conf(use_ffn=True, macaron_ffn=True, merge_k=31, rel_pos_type="latest", act="swish", dropout=0.0, V=32):
    """The small E-Branchformer model of the fixtures: D=64, 4 heads, 2 blocks, cgMLP 96 units with k 31,
    feed-forward modules of 128 units; decoder, normalisation and loss weights as the Branchformer fixtures'."""
    conf = _bf_conf(U=96, k=31, rel_pos_type=rel_pos_type, dropout=dropout, V=V)
    conf["encoder"] = "e_branchformer"
    conf["encoder_conf"] = dict(
        output_size=64, attention_heads=4, attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos",
        rel_pos_type=rel_pos_type, cgmlp_linear_units=96, cgmlp_conv_kernel=31, use_linear_after_conv=False,
        gate_activation="identity", num_blocks=2, dropout_rate=dropout, positional_dropout_rate=dropout,
        attention_dropout_rate=dropout, input_layer="conv2d", layer_drop_rate=0.0, use_ffn=use_ffn,
        macaron_ffn=macaron_ffn, ffn_activation_type=act, linear_units=128, positionwise_layer_type="linear",
        merge_conv_kernel=merge_k)
    return conf


# name -> (conf, B, T, lens, ulens, seed)
FIXTURES = {
    # T' = 29: the 31-tap merge window is wider than half the utterance
    "ebf_small_mac_k31": (small_conf(True, True, 31, "latest"), 3, 120, [120, 97, 64], [9, 5, 7], 81),
    "ebf_small_ffn_k7_legacy": (small_conf(True, False, 7, "legacy"), 3, 300, [300, 211, 150], [9, 5, 7], 82),
    "ebf_small_noffn_k3": (small_conf(False, False, 3, "latest", act="relu"), 3, 120, [120, 97, 64], [9, 5, 7], 83),
}
