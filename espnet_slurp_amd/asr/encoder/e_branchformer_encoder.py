"""EBranchformerEncoder — drop-in for espnet2/asr/encoder/e_branchformer_encoder.py:48-421.

Same constructor kwargs and state_dict keys; forward(xs_pad, ilens) -> (out, olens, None).
Computation: Conv2dSubsampling -> x*sqrt(D) + rel-pos table -> num_blocks E-Branchformer blocks -> after_norm.
A block is the Branchformer's two branches between optional (macaron) feed-forward modules, with the enhanced
merge:
    x  = x + ff_scale drop(FFN_mac(LN(x)))                                   (macaron_ffn)
    x1 = drop(MHA_relpos(LN_mha(x)))    x2 = drop(cgMLP(LN_mlp(x)))          (no residual)
    xc = [x1, x2];  u = xc + depthwise_conv_fusion(xc);  x = x + drop(merge_proj(u))
    x  = x + ff_scale drop(FFN(LN(x)))                                       (use_ffn)
    x  = LN_final(x)
ff_scale is 0.5 only with the macaron module.  The two branches write the halves of one (M, 2D) buffer, u comes
from one pass over it (kernels.ebf_merge_fwd, csrc/ebf_merge.hip) in merge_proj's operand format, and merge_proj
runs with the dropout + residual epilogue.  Like the cgMLP, the merge convolution takes no mask.
Supported: input_layer conv2d / conv2d6, rel_selfattn + rel_pos (rel_pos_type latest and legacy), use_ffn /
macaron_ffn, ffn_activation_type swish / relu, positionwise_layer_type linear, gate_activation identity,
use_linear_after_conv False, layer_drop_rate 0, zero_triu False; anything else raises NotImplementedError.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ... import kernels as K
from ...blocks import (ConvolutionalGatingMLP, Ctx, Linear, make_subsampling, LayerNorm, PositionwiseFeedForward,
                       RelPositionMultiHeadedAttention, Seeds, empty, grad_buf)
from .abs_encoder import StackedEncoder


class EBranchformerEncoderLayer(nn.Module):
    """e_branchformer_encoder.py:48-176."""

    def __init__(self, size: int, attn: nn.Module, cgmlp: nn.Module, feed_forward: Optional[nn.Module],
                 feed_forward_macaron: Optional[nn.Module], dropout_rate: float, merge_conv_kernel: int = 3):
        super().__init__()
        self.size = size
        self.attn = attn
        self.cgmlp = cgmlp
        self.feed_forward = feed_forward
        self.feed_forward_macaron = feed_forward_macaron
        self.ff_scale = 1.0
        if feed_forward is not None:
            self.norm_ff = LayerNorm(size)
        if feed_forward_macaron is not None:
            self.ff_scale = 0.5
            self.norm_ff_macaron = LayerNorm(size)
        self.norm_mha = LayerNorm(size)
        self.norm_mlp = LayerNorm(size)
        self.norm_final = LayerNorm(size)
        self.depthwise_conv_fusion = nn.Conv1d(size + size, size + size, merge_conv_kernel, 1,
                                               (merge_conv_kernel - 1) // 2, groups=size + size, bias=True)
        self.merge_proj = Linear(size + size, size)
        self.merge_conv_kernel = merge_conv_kernel
        self.p = dropout_rate

    def fwd(self, x, pos, klen, B, T, seeds: Seeds, training: bool, tvalid=None):
        c = Ctx()
        p, D = self.p, self.size
        M = x.shape[0]
        if self.feed_forward_macaron is not None:
            h, c.ln_mac = self.norm_ff_macaron.fwd(x, gemm_only=True)
            x, c.ffm = self.feed_forward_macaron.fwd(h, x, self.ff_scale, p, seeds, training)
        # the branch outputs: the halves of the merge buffer xc
        xc = empty(M, 2 * D, like=x)
        h, c.ln_mha = self.norm_mha.fwd(x, gemm_only=True)
        _, c.mha = self.attn.fwd(h, None, pos, klen, B, T, p, seeds, training, tvalid=tvalid, out=xc, ldo=2 * D)
        h, c.ln_mlp = self.norm_mlp.fwd(x, gemm_only=True)
        _, c.mlp = self.cgmlp.fwd(h, B, T, p, seeds, training, tvalid=tvalid, out=xc, out_off=D, ldo=2 * D)
        cv = self.depthwise_conv_fusion
        u = K.ebf_merge_fwd(xc, cv.weight, cv.bias, B, T, self.merge_conv_kernel, tvalid=tvalid)
        c.pm = p if training else 0.0
        c.sm = seeds.next()
        y = empty(M, D, like=x)
        self.merge_proj.fwd(u, y, drop_p=c.pm, seed=c.sm, R=x, beta=1.0)
        # kept for the backward: u (merge_proj's weight gradient) and xc (the fusion convolution's)
        c.u, c.xc, c.B, c.T, c.tvalid = u, xc, B, T, tvalid
        if self.feed_forward is not None:
            h, c.ln_ff = self.norm_ff.fwd(y, gemm_only=True)
            y, c.ff = self.feed_forward.fwd(h, y, self.ff_scale, p, seeds, training)
        y, c.ln_final = self.norm_final.fwd(y)
        return y, c

    def bwd(self, c, d):
        D = self.size
        d = self.norm_final.bwd_new(c.ln_final, d)
        if self.feed_forward is not None:
            self.norm_ff.bwd(c.ln_ff, self.feed_forward.bwd(c.ff, d), d)
            c.ff = None
        dz = grad_buf(d)
        K.scale_dropout(d, dz, drop_p=c.pm, seed=c.sm)
        w = self.merge_proj.weight
        K.linear_bwd_weight(dz, c.u, w.grad, self.merge_proj.bias.grad)
        c.u = None
        # merge_proj's input gradient in one (M, 2D) GEMM; the merge backward hands each branch its own
        # contiguous (M, D) half (each branch's backward regenerates its dropout mask over it)
        du = empty(d.shape[0], 2 * D, like=d)
        K.linear_bwd_data(dz, w, du)
        del dz
        cv = self.depthwise_conv_fusion
        d1, d2 = K.ebf_merge_bwd(du, c.xc, cv.weight, cv.weight.grad, cv.bias.grad, c.B, c.T, self.merge_conv_kernel,
                                 tvalid=c.tvalid)
        c.xc = None
        del du
        self.norm_mlp.bwd(c.ln_mlp, self.cgmlp.bwd(c.mlp, d2), d)
        c.mlp = None
        self.norm_mha.bwd(c.ln_mha, self.attn.bwd(c.mha, d1), d)
        c.mha = None
        if self.feed_forward_macaron is not None:
            self.norm_ff_macaron.bwd(c.ln_mac, self.feed_forward_macaron.bwd(c.ffm, d), d)
        return d


_FFN_ACT = {"swish": K.ACT_SWISH, "relu": K.ACT_RELU}


class EBranchformerEncoder(StackedEncoder):
    def __init__(
        self,
        input_size: int,
        output_size: int = 256,
        attention_heads: int = 4,
        attention_layer_type: str = "rel_selfattn",
        pos_enc_layer_type: str = "rel_pos",
        rel_pos_type: str = "latest",
        cgmlp_linear_units: int = 2048,
        cgmlp_conv_kernel: int = 31,
        use_linear_after_conv: bool = False,
        gate_activation: str = "identity",
        num_blocks: int = 12,
        dropout_rate: float = 0.1,
        positional_dropout_rate: float = 0.1,
        attention_dropout_rate: float = 0.0,
        input_layer: Optional[str] = "conv2d",
        zero_triu: bool = False,
        padding_idx: int = -1,
        layer_drop_rate: float = 0.0,
        max_pos_emb_len: int = 5000,
        use_ffn: bool = False,
        macaron_ffn: bool = False,
        ffn_activation_type: str = "swish",
        linear_units: int = 2048,
        positionwise_layer_type: str = "linear",
        merge_conv_kernel: int = 3,
    ):
        super().__init__(output_size, positional_dropout_rate)
        # rel_pos_type remap, e_branchformer_encoder.py:214-223
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
        if use_linear_after_conv:
            unsupported.append("use_linear_after_conv=True")
        if gate_activation != "identity":
            unsupported.append(f"gate_activation={gate_activation}")
        if zero_triu:
            unsupported.append("zero_triu")
        if layer_drop_rate:
            unsupported.append(f"layer_drop_rate={layer_drop_rate}")
        if use_ffn and positionwise_layer_type != "linear":
            unsupported.append(f"positionwise_layer_type={positionwise_layer_type}")
        if use_ffn and ffn_activation_type not in _FFN_ACT:
            unsupported.append(f"ffn_activation_type={ffn_activation_type}")
        if unsupported:
            raise NotImplementedError("espnet_slurp_amd EBranchformerEncoder: unsupported " + ", ".join(unsupported))
        # (an even kernel makes the reference fail at x_concat + x_tmp: the convolution returns T' - 1 frames)
        if merge_conv_kernel < 1 or merge_conv_kernel % 2 == 0 or merge_conv_kernel > K.EBF_MERGE_KMAX:
            raise ValueError(f"merge_conv_kernel={merge_conv_kernel} must be odd and at most {K.EBF_MERGE_KMAX}")
        if output_size % 4:
            raise ValueError(f"output_size={output_size} must be a multiple of 4")
        self.legacy = pos_enc_layer_type == "legacy_rel_pos"
        self.embed = make_subsampling(input_layer, input_size, output_size)

        def ffn():
            return PositionwiseFeedForward(output_size, linear_units, dropout_rate, _FFN_ACT[ffn_activation_type])

        self.encoders = nn.ModuleList([
            EBranchformerEncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, self.legacy),
                ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate,
                                       use_linear_after_conv, gate_activation),
                ffn() if use_ffn else None,
                ffn() if use_ffn and macaron_ffn else None,
                dropout_rate,
                merge_conv_kernel,
            ) for _ in range(num_blocks)
        ])
        self.after_norm = LayerNorm(output_size)
        self.dropout_rate = dropout_rate
        self.max_pos_emb_len = max_pos_emb_len

    # ---------------------------------------------------------------- explicit passes
    def run_forward(self, feats, ilens_cpu, seeds: Seeds, training: bool, klen=None, tvalid=None, inter=None):
        """tvalid: optional device int32 (1,) = the reference batch's T' when feats are padded to a length
        bucket: frames beyond it are outside the cgMLP's and the merge's depthwise windows (read as their zero
        padding, written as 0) and the legacy rel_shift is taken at T'; every other op is per frame or masked
        by klen."""
        assert inter is None
        B, olens = self._begin(feats, ilens_cpu)
        klen = self._klen(klen, olens, feats.device)
        x, pos, c_emb = self._embed_rel(feats, seeds, training)
        x, ctxs = self._layers_fwd(x, pos, klen, B, c_emb.T2, seeds, training, tvalid=tvalid)
        return self._finish(x, B, olens, emb=c_emb, layers=ctxs)
