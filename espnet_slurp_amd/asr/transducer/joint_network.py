"""JointNetwork — drop-in for espnet2/asr_transducer/joint_network.py:8-59.

lin_out(act(lin_enc(enc_out) + lin_dec(dec_out))) with the reference's state_dict keys (lin_enc.{weight,bias},
lin_dec.weight, lin_out.{weight,bias}).  The three Linears and their adjoints are the MFMA GEMM launchers; the
broadcast sum + activation and its two-way adjoint are esp_rnnt_joint_fwd / _bwd (csrc/rnnt.hip).  The logits
(B, T, U1, V) and the joint activations (B, T, U1, J) are materialised.
"""
from __future__ import annotations

import torch
from torch import nn

from ... import kernels as K
from ...blocks import Ctx, Linear, empty


class JointNetwork(nn.Module):
    def __init__(self, output_size: int, encoder_size: int, decoder_size: int, joint_space_size: int = 256,
                 joint_activation_type: str = "tanh", **activation_parameters):
        super().__init__()
        self.act = K.rnnt_act(joint_activation_type)
        if activation_parameters:
            raise NotImplementedError(f"joint activation parameters {sorted(activation_parameters)}: tanh / relu take none")
        self.lin_enc = Linear(encoder_size, joint_space_size)
        self.lin_dec = Linear(decoder_size, joint_space_size, bias=False)
        self.lin_out = Linear(joint_space_size, output_size)
        self.joint_space_size = joint_space_size
        self.output_size = output_size

    def run_forward(self, hs2d, dec2d, B: int, T: int, U1: int):
        """hs2d (B*T, D_enc), dec2d (B*U1, D_dec) -> logits (B*T*U1, V) and the saved context."""
        J = self.joint_space_size
        pe = self.lin_enc.fwd(hs2d)
        pd = self.lin_dec.fwd(dec2d)
        z = K.rnnt_joint_fwd(pe, pd, empty(B * T * U1, J, like=hs2d), B, T, U1, J, self.act)
        return self.lin_out.fwd(z), Ctx(hs2d=hs2d, dec2d=dec2d, z=z, B=B, T=T, U1=U1)

    def run_backward(self, c, dlogits, hlens_i32, tlens_i32, dhs):
        """dlogits (B*T*U1, V) (zero in padded cells); dhs (B*T, D_enc) accumulated (+=); returns d dec2d."""
        B, T, U1, J = c.B, c.T, c.U1, self.joint_space_size
        dz = self.lin_out.bwd(dlogits, c.z)
        dpe = empty(B * T, J, like=dz)
        dpd = empty(B * U1, J, like=dz)
        K.rnnt_joint_bwd(dz, c.z, hlens_i32, tlens_i32, dpe, dpd, B, T, U1, J, self.act)
        self.lin_enc.bwd(dpe, c.hs2d, dx=dhs, accumulate=True)
        return self.lin_dec.bwd(dpd, c.dec2d)

    # ------------------------------------------------------------------ inference
    def project_enc(self, enc_out: torch.Tensor) -> torch.Tensor:
        """lin_enc of every frame at once: (T, D_enc) -> (T, J)."""
        with torch.no_grad():
            return self.lin_enc.fwd(enc_out.contiguous())

    def step_logp(self, pe_t: torch.Tensor, dec_out: torch.Tensor) -> torch.Tensor:
        """log_softmax(lin_out(act(pe_t + lin_dec(dec_out)))) for one projected frame pe_t (1, J) and n decoder
        outputs (n, D_dec): (n, V) on the device."""
        n, J, V = dec_out.shape[0], self.joint_space_size, self.output_size
        with torch.no_grad():
            pd = self.lin_dec.fwd(dec_out.contiguous())
            z = K.rnnt_joint_fwd(pe_t, pd, empty(n, J, like=pd), 1, 1, n, J, self.act)
            logits = self.lin_out.fwd(z)
            lp = torch.empty_like(logits)
            K.log_softmax(logits, lp, n, V)
        return lp

    def forward(self, enc_out: torch.Tensor, dec_out: torch.Tensor) -> torch.Tensor:
        """Inference-style joint of one frame and one decoder output: (D_enc,), (D_dec,) -> (V,) logits."""
        with torch.no_grad():
            pe = self.lin_enc.fwd(enc_out.reshape(1, -1).contiguous())
            pd = self.lin_dec.fwd(dec_out.reshape(1, -1).contiguous())
            J = self.joint_space_size
            z = K.rnnt_joint_fwd(pe, pd, empty(1, J, like=pd), 1, 1, 1, J, self.act)
            return self.lin_out.fwd(z)[0]
