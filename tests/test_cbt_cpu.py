"""Contextual block Transformer encoder, host side (no GPU): the registry, the state_dict against the reference's
recorded keys, the unsupported options, and the host block layout against the maps recorded from the reference's
forward_train (tests/golden/make_cbt_golden.py: one-hot coded frames through input_layer=None, the layer stack
replaced by a recording pass-through)."""
import pytest
import torch

from tests import cbt_helpers as CH


def _cls():
    from espnet_slurp_amd.tasks.asr import encoder_choices
    return encoder_choices.get_class("contextual_block_transformer")


def test_registry():
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder
    from espnet_slurp_amd.tasks.asr import encoder_choices
    assert _cls() is ContextualBlockTransformerEncoder
    assert set(encoder_choices.choices()) == {"conformer", "transformer", "branchformer",
                                              "contextual_block_transformer"}
    with pytest.raises(ValueError):
        encoder_choices.get_class("e_branchformer")


def test_state_dict_small():
    ref = CH.load_json("cbt_slurp_streaming")["small_encoder_state_dict"]
    enc = _cls()(CH.INPUT_SIZE, **CH.encoder_conf())
    got = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
    assert len(ref) == 56
    assert got == ref
    assert "embed.out.weight" in dict((k, s) for k, s in got)


def test_state_dict_streaming_recipe():
    conf = CH.load_json("cbt_slurp_streaming")
    e = conf["encoder_conf"]
    assert conf["encoder"] == "contextual_block_transformer"
    assert (e["output_size"], e["attention_heads"], e["num_blocks"]) == (512, 8, 12)
    assert (e["block_size"], e["hop_size"], e["look_ahead"]) == (40, 16, 16)
    with torch.device("meta"):
        enc = _cls()(conf["input_size"], **e)
    got = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
    assert got == conf["reference_encoder_state_dict"]


@pytest.mark.parametrize("kw,name", [
    (dict(input_layer="linear"), "input_layer"), (dict(input_layer="conv2d8"), "input_layer"),
    (dict(input_layer=None), "input_layer"), (dict(normalize_before=False), "normalize_before"),
    (dict(concat_after=True), "concat_after"), (dict(positionwise_layer_type="conv1d"), "positionwise_layer_type"),
    (dict(positionwise_layer_type="conv1d-linear"), "positionwise_layer_type"),
    (dict(pos_enc_class=torch.nn.Identity), "pos_enc_class"), (dict(init_average=False), "init_average"),
])
def test_unsupported_options_raise_and_are_named(kw, name):
    with pytest.raises(NotImplementedError) as ei:
        _cls()(CH.INPUT_SIZE, **{**CH.encoder_conf(), **kw})
    msg = str(ei.value)
    assert name in msg.split("; got ")[1]
    # one message that names every unsupported option
    for n in ("input_layer", "normalize_before", "concat_after", "positionwise_layer_type", "pos_enc_class",
              "init_average", "infer_mode", "forward_infer", "tvalid"):
        assert n in msg.split("; got ")[0], n


def test_unsupported_calls_raise():
    enc = _cls()(CH.INPUT_SIZE, **CH.encoder_conf())
    enc.eval()
    x, lens = torch.zeros(1, 39, CH.INPUT_SIZE), torch.tensor([39])
    with pytest.raises(NotImplementedError, match="infer_mode"):
        enc(x, lens, infer_mode=True)
    with pytest.raises(NotImplementedError, match="forward_infer"):
        enc.forward_infer(x, lens)
    with pytest.raises(NotImplementedError, match="tvalid"):
        enc.forward_prepared(x, lens, None, 0, tvalid=torch.tensor([9]))
    with pytest.raises(NotImplementedError, match="tvalid"):
        enc.run_forward(x, lens, None, False, tvalid=torch.tensor([9]))


@pytest.mark.parametrize("kw", [dict(hop_size=0), dict(hop_size=-1), dict(block_size=8, hop_size=6, look_ahead=3),
                                dict(block_size=4, hop_size=3, look_ahead=3)])
def test_bad_block_sizes_raise_value_error(kw):
    with pytest.raises(ValueError):
        _cls()(CH.INPUT_SIZE, **{**CH.encoder_conf(), **kw})
    # block_size 0 means no blocks at all: any hop is accepted
    _cls()(CH.INPUT_SIZE, **{**CH.encoder_conf(), "block_size": 0, "hop_size": 0})


@pytest.mark.parametrize("key", list(CH.LAYOUT_CASES))
def test_block_layout_equals_reference_maps(key):
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import BlockLayout
    bs, hop, la, Ts = CH.LAYOUT_CASES[key]
    maps = CH.load_json("cbt_layout")[key]
    assert sorted(int(t) for t in maps) == sorted(Ts)
    for T in Ts:
        ref = maps[str(T)]
        L = BlockLayout(T, bs, hop, la)
        assert L.nblk == ref["nblk"], T
        assert L.S == bs + 2
        assert L.chunk_source() == ref["chunk_source"], T
        assert [list(L.window(k)) for k in range(L.nblk)] == ref["ctx_window"], T
        assert [list(p) for p in L.output_source()] == ref["output_source"], T
    assert maps[str(Ts[-1])]["nblk"] == (8 if key == "8/3/3" else 22)


def test_short_input_has_no_layout():
    enc = _cls()(CH.INPUT_SIZE, **CH.encoder_conf())
    assert enc.layout(8) is None and enc.layout(3) is None
    assert enc.layout(9).nblk == 2
    enc0 = _cls()(CH.INPUT_SIZE, **{**CH.encoder_conf(), "block_size": 0})
    assert enc0.layout(500) is None


def test_output_lengths_come_from_the_pad_mask():
    enc = _cls()(CH.INPUT_SIZE, **CH.encoder_conf())
    for name, (conf, T2, lens, seed) in CH.ENC_FIXTURES.items():
        g = CH.load(name)
        assert enc.output_lengths(torch.tensor(lens), 4 * T2 + 3).tolist() == g["olens"].tolist()
