"""E-Branchformer encoder, the parts that need no GPU: registry, state_dict keys / shapes against the reference's
(recorded in the fixtures), the unsupported-option errors and the ABI's new entry points."""
import os
import re

import pytest
import torch

from tests import ebranchformer_helpers as EH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esp_ebf_merge_fwd", "esp_ebf_merge_bwd", "esp_ebf_merge_bwd_workspace_bytes")


def _encoder(**kw):
    from espnet_slurp_amd.asr.encoder.e_branchformer_encoder import EBranchformerEncoder
    conf = dict(EH.small_conf()["encoder_conf"])
    conf.update(kw)
    return EBranchformerEncoder(input_size=80, **conf)


def test_registry_resolves_e_branchformer():
    from espnet_slurp_amd.asr.encoder.e_branchformer_encoder import EBranchformerEncoder
    from espnet_slurp_amd.asr.encoder.branchformer_encoder import BranchformerEncoder
    from espnet_slurp_amd.tasks import asr
    # build_model resolves `encoder:` through encoder_class, which reads both encoder registries
    assert asr.encoder_class("e_branchformer") is EBranchformerEncoder
    assert asr.encoder_class("E_Branchformer") is EBranchformerEncoder
    assert asr.added_encoder_choices.get_class("e_branchformer") is EBranchformerEncoder
    assert asr.encoder_class("branchformer") is BranchformerEncoder
    with pytest.raises(ValueError, match="must be one of .*e_branchformer.*: --encoder vgg_rnn"):
        asr.encoder_class("vgg_rnn")


@pytest.mark.parametrize("name", list(EH.FIXTURES))
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    g = EH.load_fixture(name)
    conf = EH.FIXTURES[name][0]
    from espnet_slurp_amd.asr.encoder.e_branchformer_encoder import EBranchformerEncoder
    enc = EBranchformerEncoder(input_size=conf["input_size"], **conf["encoder_conf"])
    ref = {str(k): tuple(int(s) for s in shp if s) for k, shp in zip(g["enc_sd_keys"], g["enc_sd_shapes"])}
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == ref, (sorted(set(got) ^ set(ref)), [(k, got[k], ref[k]) for k in got if k in ref and got[k] != ref[k]])
    k = conf["encoder_conf"]["merge_conv_kernel"]
    assert got["encoders.0.depthwise_conv_fusion.weight"] == (128, 1, k)
    assert got["encoders.1.depthwise_conv_fusion.bias"] == (128,)
    assert got["encoders.0.merge_proj.weight"] == (64, 128)
    ffn, mac = conf["encoder_conf"]["use_ffn"], conf["encoder_conf"]["macaron_ffn"]
    assert ("encoders.0.feed_forward.w_1.weight" in got) == ffn and ("encoders.0.norm_ff.weight" in got) == ffn
    assert ("encoders.0.feed_forward_macaron.w_2.bias" in got) == mac
    assert ("encoders.0.norm_ff_macaron.bias" in got) == mac
    if ffn:
        assert got["encoders.0.feed_forward.w_1.weight"] == (128, 64)
    assert enc.encoders[0].ff_scale == (0.5 if mac else 1.0)


def test_fixtures_cannot_be_met_by_a_masked_merge():
    for name in EH.FIXTURES:
        g = EH.load_fixture(name)
        assert abs(float(g["loss_masked_merge_f64"]) - float(g["loss_f64"])) > 10 * 1e-4, name


@pytest.mark.parametrize("kw,word", [
    (dict(attention_layer_type="fast_selfattn", pos_enc_layer_type="abs_pos"), "abs_pos/fast_selfattn"),
    (dict(attention_layer_type="selfattn", pos_enc_layer_type="abs_pos"), "abs_pos/selfattn"),
    (dict(attention_layer_type="selfattn", pos_enc_layer_type="scaled_abs_pos"), "scaled_abs_pos/selfattn"),
    (dict(input_layer="linear"), "input_layer=linear"), (dict(input_layer="embed"), "input_layer=embed"),
    (dict(input_layer="conv2d8"), "input_layer=conv2d8"), (dict(input_layer=None), "input_layer=None"),
    (dict(layer_drop_rate=0.1), "layer_drop_rate=0.1"), (dict(zero_triu=True), "zero_triu"),
    (dict(use_linear_after_conv=True), "use_linear_after_conv=True"),
    (dict(gate_activation="swish"), "gate_activation=swish"),
    (dict(ffn_activation_type="gelu"), "ffn_activation_type=gelu"),
    (dict(positionwise_layer_type="conv1d"), "positionwise_layer_type=conv1d"),
])
def test_unsupported_options_raise_and_name_themselves(kw, word):
    with pytest.raises(NotImplementedError, match="EBranchformerEncoder: unsupported") as e:
        _encoder(**kw)
    assert word in str(e.value)


def test_unsupported_options_are_named_together():
    with pytest.raises(NotImplementedError) as e:
        _encoder(layer_drop_rate=0.2, input_layer="linear", zero_triu=True)
    for word in ("layer_drop_rate=0.2", "input_layer=linear", "zero_triu"):
        assert word in str(e.value)


@pytest.mark.parametrize("kw", [dict(merge_conv_kernel=30), dict(merge_conv_kernel=2), dict(merge_conv_kernel=0),
                                dict(merge_conv_kernel=33), dict(cgmlp_conv_kernel=8), dict(rel_pos_type="newest")])
def test_even_or_oversized_kernel_raises_value_error(kw):
    with pytest.raises(ValueError):
        _encoder(**kw)


def test_supported_variants_construct():
    assert _encoder(rel_pos_type="legacy").legacy
    assert _encoder(input_layer="conv2d6").embed.input_layer == "conv2d6"
    e = _encoder(use_ffn=False, macaron_ffn=True)  # the macaron module exists only with use_ffn
    assert e.encoders[0].feed_forward is None and e.encoders[0].feed_forward_macaron is None
    assert e.encoders[0].ff_scale == 1.0 and not any("feed_forward" in k or "norm_ff" in k for k in e.state_dict())
    e = _encoder(use_ffn=False, ffn_activation_type="gelu", positionwise_layer_type="conv1d")  # not used: not refused
    assert e.encoders[0].feed_forward is None
    from espnet_slurp_amd import kernels as K
    assert _encoder(ffn_activation_type="relu").encoders[0].feed_forward.act == K.ACT_RELU
    assert _encoder(merge_conv_kernel=1).encoders[1].depthwise_conv_fusion.weight.shape == (128, 1, 1)
    assert _encoder(max_pos_emb_len=777).max_pos_emb_len == 777
    assert K.EBF_MERGE_FUSED in (True, False) and K.EBF_MERGE_KMAX == 31


def test_reference_default_arguments():
    import inspect
    from espnet_slurp_amd.asr.encoder.e_branchformer_encoder import EBranchformerEncoder
    d = {k: p.default for k, p in inspect.signature(EBranchformerEncoder.__init__).parameters.items()}
    for k, v in dict(output_size=256, attention_heads=4, cgmlp_linear_units=2048, cgmlp_conv_kernel=31, num_blocks=12,
                     use_ffn=False, macaron_ffn=False, ffn_activation_type="swish", linear_units=2048,
                     merge_conv_kernel=3, rel_pos_type="latest", layer_drop_rate=0.0, max_pos_emb_len=5000).items():
        assert d[k] == v, k


def _args(proto):
    return [a for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",") if a.strip()]


def test_header_and_signature_table_have_the_entry_points():
    from espnet_slurp_amd import _native
    with open(os.path.join(ROOT, "include", "espnet_mi355.h"), encoding="utf-8") as f:
        h = f.read()
    for name in NEW:
        m = re.search(r"\b(?:int|long) " + name + r"\([^;]*\);", h)
        assert m, name
        assert name in _native.SIGNATURES, name
        assert len(_args(m.group(0))) == len(_native.SIGNATURES[name]), name
    with open(os.path.join(ROOT, "espnet_slurp_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        assert "ebf_merge.hip" in f.read()


def test_bench_tool_trace_analysis(tmp_path, capsys):
    """tools/bench_ebranchformer.py --analyze-trace: per-launch medians and the algorithmic bytes from the shapes."""
    import csv
    import json
    from tools import bench_ebranchformer as T
    fwd = "void (anonymous namespace)::ebf_merge_fwd_kernel<31>((anonymous namespace)::MergeArgs)"
    bwd = "void (anonymous namespace)::ebf_merge_bwd_kernel<31>((anonymous namespace)::MergeArgs)"
    with open(tmp_path / "t_kernel_trace.csv", "w", newline="") as f:
        w = csv.DictWriter(f, ["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writeheader()
        t = 0
        for name, dur in ((fwd, 40_000), (bwd, 90_000), ("ln_fwd_kernel<4>", 70_000), (fwd, 50_000), (fwd, 60_000)):
            w.writerow({"Kernel_Name": name, "Start_Timestamp": t, "End_Timestamp": t + dur})
            t += dur + 10
    T.analyze_trace(str(tmp_path / "t_kernel_trace.csv"), 64)
    out = json.loads(capsys.readouterr().out)
    M = 64 * 374
    assert out["rows_M"] == M and out["kernels"]["ebf_merge_fwd_kernel"]["launches"] == 3
    assert out["kernels"]["ebf_merge_fwd_kernel"]["median_us"] == 50.0
    assert out["kernels"]["ebf_merge_fwd_kernel"]["algorithmic_bytes"] == 2 * M * 1024 * 4 + 4 * 1024 * 32
    assert out["kernels"]["ebf_merge_bwd_kernel"]["algorithmic_bytes"] == 3 * M * 1024 * 4
    conf = T.bench_conf()
    assert conf["encoder"] == "e_branchformer" and conf["encoder_conf"]["num_blocks"] == 12
    assert conf["specaug"] == "specaug" and conf["decoder_conf"]["num_blocks"] == 6


def test_workspace_query_is_host_arithmetic():
    from espnet_slurp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    q = _native.workspace_bytes
    assert q("esp_ebf_merge_bwd", 0, 10, 128, 3) == 0
    one = q("esp_ebf_merge_bwd", 1, 1, 128, 3)
    assert one == 4 * 128 * 4  # one partial: C * (k + 1) floats
    assert q("esp_ebf_merge_bwd", 3, 256, 128, 3) == 3 * one  # a backward block walks four 64-frame tiles
    assert q("esp_ebf_merge_bwd", 3, 257, 128, 3) == 6 * one
    assert q("esp_ebf_merge_bwd", 2, 257, 80, 31) == 2 * 2 * 4 * 80 * 32
