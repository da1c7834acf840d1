"""BranchformerEncoder — drop-in for espnet2/asr/encoder/branchformer_encoder.py:48-547.

Same constructor kwargs and state_dict keys; forward(xs_pad, ilens) -> (out, olens, None).
Computation: Conv2dSubsampling -> x*sqrt(D) + rel-pos table -> num_blocks Branchformer blocks -> after_norm.
A block runs two branches on the same input,
    x1 = drop(MHA_relpos(LN_mha(x)))   (no residual)        x2 = drop(cgMLP(LN_mlp(x)))
and merges them (merge_method concat): x = LN_final(x + drop(merge_proj([x1, x2]))).  The two branches write
the halves of one (M, 2D) buffer, so merge_proj is one GEMM with the dropout + residual epilogue and no
concatenation is made.  The cgMLP takes no mask (blocks.ConvolutionalSpatialGatingUnit).
Supported: input_layer conv2d / conv2d6, rel_selfattn + rel_pos (rel_pos_type latest and legacy), merge_method
concat, single-branch models (use_attn / use_cgmlp False: merge_proj is the identity); anything else raises
NotImplementedError.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch
from torch import nn

from ... import kernels as K
from ...blocks import (ConvolutionalGatingMLP, Ctx, Linear, make_subsampling, LayerNorm,
                       RelPositionMultiHeadedAttention, Seeds, empty, grad_buf)
from .abs_encoder import StackedEncoder


class BranchformerEncoderLayer(nn.Module):
    """branchformer_encoder.py:48-292, merge_method concat (or one branch and the identity merge)."""

    def __init__(self, size: int, attn: Optional[nn.Module], cgmlp: Optional[nn.Module], dropout_rate: float):
        super().__init__()
        assert attn is not None or cgmlp is not None, "At least one branch should be valid"
        self.size = size
        self.attn = attn
        self.cgmlp = cgmlp
        self.use_two_branches = attn is not None and cgmlp is not None
        if attn is not None:
            self.norm_mha = LayerNorm(size)
        if cgmlp is not None:
            self.norm_mlp = LayerNorm(size)
        self.norm_final = LayerNorm(size)
        self.merge_proj = Linear(size + size, size) if self.use_two_branches else nn.Identity()
        self.p = dropout_rate

    def fwd(self, x, pos, klen, B, T, seeds: Seeds, training: bool, tvalid=None):
        c = Ctx()
        p, D = self.p, self.size
        M = x.shape[0]
        two = self.use_two_branches
        # the branch outputs: the halves of the merge buffer, or the single branch's own (M, D)
        merge = empty(M, 2 * D if two else D, like=x)
        ld = 2 * D if two else None
        if self.attn is not None:
            h, c.ln_mha = self.norm_mha.fwd(x, gemm_only=True)
            _, c.mha = self.attn.fwd(h, None, pos, klen, B, T, p, seeds, training, tvalid=tvalid, out=merge, ldo=ld)
        if self.cgmlp is not None:
            h, c.ln_mlp = self.norm_mlp.fwd(x, gemm_only=True)
            _, c.mlp = self.cgmlp.fwd(h, B, T, p, seeds, training, tvalid=tvalid, out=merge, out_off=D if two else 0,
                                      ldo=ld)
        c.pm = p if training else 0.0
        c.sm = seeds.next()
        y = empty(M, D, like=x)
        if two:
            self.merge_proj.fwd(merge, y, drop_p=c.pm, seed=c.sm, R=x, beta=1.0)
            c.merge = merge
        else:  # x + drop(branch)
            K.scale_dropout(merge, y, drop_p=c.pm, seed=c.sm, r=x, beta=1.0)
        y, c.ln_final = self.norm_final.fwd(y)
        return y, c

    def bwd(self, c, d):
        D = self.size
        d = self.norm_final.bwd_new(c.ln_final, d)
        if self.use_two_branches:
            dz = grad_buf(d)
            K.scale_dropout(d, dz, drop_p=c.pm, seed=c.sm)
            w = self.merge_proj.weight
            K.linear_bwd_weight(dz, c.merge, w.grad, self.merge_proj.bias.grad)
            c.merge = None
            # the two halves of the merge buffer's gradient as two contiguous (M, D) tensors: each branch's
            # backward regenerates its own dropout mask over it
            d1 = empty(d.shape[0], D, like=d)
            K.linear_bwd_data(dz, w[:, :D], d1)
            d2 = empty(d.shape[0], D, like=d)
            K.linear_bwd_data(dz, w[:, D:], d2)
            del dz
        else:
            d1 = torch.empty_like(d)
            K.scale_dropout(d, d1, drop_p=c.pm, seed=c.sm)
            d2 = d1
        if self.cgmlp is not None:
            self.norm_mlp.bwd(c.ln_mlp, self.cgmlp.bwd(c.mlp, d2), d)
            c.mlp = None
        if self.attn is not None:
            self.norm_mha.bwd(c.ln_mha, self.attn.bwd(c.mha, d1), d)
        return d


class BranchformerEncoder(StackedEncoder):
    def __init__(
        self,
        input_size: int,
        output_size: int = 256,
        use_attn: bool = True,
        attention_heads: int = 4,
        attention_layer_type: str = "rel_selfattn",
        pos_enc_layer_type: str = "rel_pos",
        rel_pos_type: str = "latest",
        use_cgmlp: bool = True,
        cgmlp_linear_units: int = 2048,
        cgmlp_conv_kernel: int = 31,
        use_linear_after_conv: bool = False,
        gate_activation: str = "identity",
        merge_method: str = "concat",
        cgmlp_weight: Union[float, List[float]] = 0.5,
        attn_branch_drop_rate: Union[float, List[float]] = 0.0,
        num_blocks: int = 12,
        dropout_rate: float = 0.1,
        positional_dropout_rate: float = 0.1,
        attention_dropout_rate: float = 0.0,
        input_layer: Optional[str] = "conv2d",
        zero_triu: bool = False,
        padding_idx: int = -1,
        stochastic_depth_rate: Union[float, List[float]] = 0.0,
        max_pos_emb_len: int = 5000,
    ):
        super().__init__(output_size, positional_dropout_rate)
        # rel_pos_type remap, branchformer_encoder.py:328-337
        if rel_pos_type == "legacy":
            if pos_enc_layer_type == "rel_pos":
                pos_enc_layer_type = "legacy_rel_pos"
            if attention_layer_type == "rel_selfattn":
                attention_layer_type = "legacy_rel_selfattn"
        elif rel_pos_type == "latest":
            assert attention_layer_type != "legacy_rel_selfattn"
            assert pos_enc_layer_type != "legacy_rel_pos"
        else:
            raise ValueError("unknown rel_pos_type: " + rel_pos_type)
        unsupported = []
        if input_layer not in ("conv2d", "conv2d6"):
            unsupported.append(f"input_layer={input_layer}")
        if (pos_enc_layer_type, attention_layer_type) not in (("rel_pos", "rel_selfattn"),
                                                              ("legacy_rel_pos", "legacy_rel_selfattn")):
            unsupported.append(f"{pos_enc_layer_type}/{attention_layer_type}")
        if use_attn and use_cgmlp and merge_method != "concat":
            unsupported.append(f"merge_method={merge_method}")
        if use_cgmlp and use_linear_after_conv:
            unsupported.append("use_linear_after_conv=True")
        if use_cgmlp and gate_activation != "identity":
            unsupported.append(f"gate_activation={gate_activation}")
        if zero_triu:
            unsupported.append("zero_triu")
        sdr = stochastic_depth_rate if isinstance(stochastic_depth_rate, list) else [stochastic_depth_rate]
        if any(r != 0.0 for r in sdr):
            unsupported.append("stochastic_depth_rate")
        if unsupported:
            raise NotImplementedError("espnet_slurp_amd BranchformerEncoder: unsupported " + ", ".join(unsupported))
        if not (use_attn or use_cgmlp):
            raise ValueError("At least one branch should be valid")
        self.legacy = pos_enc_layer_type == "legacy_rel_pos"
        self.embed = make_subsampling(input_layer, input_size, output_size)
        self.encoders = nn.ModuleList([
            BranchformerEncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, self.legacy)
                if use_attn else None,
                ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate,
                                       use_linear_after_conv, gate_activation) if use_cgmlp else None,
                dropout_rate,
            ) for _ in range(num_blocks)
        ])
        self.after_norm = LayerNorm(output_size)
        self.dropout_rate = dropout_rate
        self.max_pos_emb_len = max_pos_emb_len

    # ---------------------------------------------------------------- explicit passes
    def run_forward(self, feats, ilens_cpu, seeds: Seeds, training: bool, klen=None, tvalid=None, inter=None):
        """tvalid: optional device int32 (1,) = the reference batch's T' when feats are padded to a length
        bucket: frames beyond it are outside the cgMLP's depthwise window (read as its zero padding, written
        as 0) and the legacy rel_shift is taken at T'; every other op is per frame or masked by klen."""
        assert inter is None
        B, olens = self._begin(feats, ilens_cpu)
        klen = self._klen(klen, olens, feats.device)
        x, pos, c_emb = self._embed_rel(feats, seeds, training)
        x, ctxs = self._layers_fwd(x, pos, klen, B, c_emb.T2, seeds, training, tvalid=tvalid)
        return self._finish(x, B, olens, emb=c_emb, layers=ctxs)
