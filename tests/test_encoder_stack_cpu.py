"""The shared encoder plumbing (abs_encoder.StackedEncoder) and the one pre-LN Transformer layer, host side: no
native library is loaded.  The four encoder classes are built small on the CPU; a run stops at the first native
call (embed.fwd, patched to raise)."""
import pytest
import torch

from tests import cbt_helpers as CH
from tests import lm_helpers as LH

F = 20  # feature bins
LIMITS = {"conv2d": 7, "conv2d6": 11}  # check_short_utt (subsampling.py:31-39)


def _build(kind, input_layer="conv2d", **kw):
    from espnet_slurp_amd.asr.encoder.branchformer_encoder import BranchformerEncoder
    from espnet_slurp_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder
    from espnet_slurp_amd.asr.encoder.transformer_encoder import TransformerEncoder
    small = dict(output_size=32, attention_heads=2, num_blocks=2, input_layer=input_layer)
    if kind == "transformer":
        return TransformerEncoder(F, linear_units=48, **small)
    if kind == "conformer":
        return ConformerEncoder(F, linear_units=48, macaron_style=True, rel_pos_type="latest", cnn_module_kernel=7,
                                **small)
    if kind == "branchformer":
        return BranchformerEncoder(F, cgmlp_linear_units=48, cgmlp_conv_kernel=7, **{**small, **kw})
    assert kind == "contextual_block_transformer"
    return ContextualBlockTransformerEncoder(F, **{**CH.encoder_conf(), "input_layer": input_layer})


KINDS = ("transformer", "conformer", "branchformer", "contextual_block_transformer")


class _FirstNativeCall(Exception):
    pass


def _raise_first_native_call(*a, **k):
    raise _FirstNativeCall


@pytest.mark.parametrize("input_layer", list(LIMITS))
def test_frame_check_is_the_same_for_all_four(input_layer, monkeypatch):
    from espnet_slurp_amd.asr.encoder.abs_encoder import StackedEncoder, TooShortUttError
    from espnet_slurp_amd.blocks import Seeds
    lim = LIMITS[input_layer]
    T = lim - 1
    messages = set()
    for kind in KINDS:
        enc = _build(kind, input_layer).eval()
        assert isinstance(enc, StackedEncoder)
        assert enc.embed.min_frames == lim
        with pytest.raises(TooShortUttError) as ei:
            enc.run_forward(torch.zeros(2, T, F), torch.tensor([T, T - 1]), Seeds(0), False)
        assert ei.value.actual_size == T and ei.value.limit == lim
        messages.add(str(ei.value))
        # exactly lim frames pass the check: the run reaches the subsampling
        monkeypatch.setattr(enc.embed, "fwd", _raise_first_native_call)
        with pytest.raises(_FirstNativeCall):
            enc.run_forward(torch.zeros(2, lim, F), torch.tensor([lim, lim - 1]), Seeds(0), False)
    # the reference's text (conformer_encoder.py:321-328 and the same lines of the other three encoders)
    assert messages == {f"has {T} frames and is too short for subsampling (it needs more than {lim} frames), "
                        "return empty results"}


@pytest.mark.parametrize("input_layer", list(LIMITS))
def test_output_lengths_are_the_mask_lengths(input_layer):
    from espnet_slurp_amd.asr.encoder.abs_encoder import subsampled_lengths
    lens = torch.tensor([97, 64, 33, 12, 1])
    for kind in KINDS:
        enc = _build(kind, input_layer)
        for T in (97, 120):
            want = subsampled_lengths(lens, T, input_layer)
            assert enc.output_lengths(lens, T).tolist() == want.tolist()
    assert subsampled_lengths(lens, 97, "conv2d").tolist() != subsampled_lengths(lens, 97, "conv2d6").tolist()


def _attention_modules(enc):
    from espnet_slurp_amd.blocks import MultiHeadedAttention, RelPositionMultiHeadedAttention
    return [m for m in enc.modules() if isinstance(m, (MultiHeadedAttention, RelPositionMultiHeadedAttention))]


@pytest.mark.parametrize("kind,kw,per_layer", [
    ("transformer", {}, 1), ("conformer", {}, 1), ("branchformer", {}, 1), ("contextual_block_transformer", {}, 1),
    ("branchformer", dict(use_cgmlp=False), 1),  # attention-only layers
    ("branchformer", dict(use_attn=False), 0),  # cgMLP-only: nothing to reach, and no error
])
def test_attach_flat_reaches_every_attention_module(kind, kw, per_layer):
    enc = _build(kind, **kw)
    attn = _attention_modules(enc)
    assert len(enc.encoders) >= 2 and len(attn) == per_layer * len(enc.encoders)
    assert enc.flat is None
    flat = object()
    enc.attach_flat(flat)
    assert enc.flat is flat
    assert all(m.flat is flat for m in attn)


def test_the_shared_methods_are_defined_once():
    from espnet_slurp_amd.asr.encoder.abs_encoder import StackedEncoder
    for kind in KINDS:
        cls = type(_build(kind))
        for name in ("forward_prepared", "output_lengths", "output_size", "attach_flat", "_begin", "_klen", "_embed_rel",
                     "_embed_abs", "_embed_bwd", "_layers_fwd", "_layers_bwd"):
            assert getattr(cls, name) is getattr(StackedEncoder, name), (kind, name)


def test_the_contextual_block_layer_is_the_transformer_layer():
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockEncoderLayer
    from espnet_slurp_amd.asr.encoder.transformer_encoder import TransformerEncoderLayer
    assert issubclass(ContextualBlockEncoderLayer, TransformerEncoderLayer)
    assert ContextualBlockEncoderLayer.fwd is TransformerEncoderLayer.fwd
    assert ContextualBlockEncoderLayer.bwd is TransformerEncoderLayer.bwd
    assert not any(l.causal for l in _build("transformer").encoders)
    assert not any(l.causal for l in _build("contextual_block_transformer").encoders)


def test_lm_layers_are_causal_transformer_layers():
    from espnet_slurp_amd.asr.encoder.transformer_encoder import TransformerEncoderLayer
    from espnet_slurp_amd.lm import TransformerLM
    lm = TransformerLM(LH.V, **LH.LM_CFGS["A"])
    assert len(lm.encoder.encoders) == LH.LM_CFGS["A"]["layer"]
    for layer in lm.encoder.encoders:
        assert type(layer) is TransformerEncoderLayer
        assert layer.causal is True
    assert [[k, list(v.shape)] for k, v in lm.state_dict().items()] == LH.golden_keys()["A"]
