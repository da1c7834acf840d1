"""Per-kernel times of the rel-pos attention backward chains at the bench shape (B=384, T'=374, H=4, d_k=64)."""
import math, sys, os
sys.path.insert(0, os.getcwd())
import torch
from espnet_slurp_amd import kernels as K
from espnet_slurp_amd.blocks import RelPositionMultiHeadedAttention, Seeds
from espnet_slurp_amd.asr.encoder.abs_encoder import pos_table
from espnet_slurp_amd.flat import FlatParams

dev = torch.device("cuda:0")
H, D, DK = 4, 256, 64
B = int(sys.argv[1]) if len(sys.argv) > 1 else 384
T = 374
Z, M, P = H * B, B * T, 2 * T - 1
Tp, Pp = K.pitch(T), K.pitch(P)
torch.manual_seed(0)
mod = RelPositionMultiHeadedAttention(H, D, 0.1, False).to(dev)
mod.flat = FlatParams(mod, dev)
x = torch.randn(M, D, device=dev); res = torch.randn(M, D, device=dev)
pos = pos_table("latest", T, D, dev)
klen = torch.full((B,), T, dtype=torch.int32, device=dev)
_, c = mod.fwd(x, res, pos, klen, B, T, 0.0, Seeds(7), True)
dctx = torch.randn(M, D, device=dev)
dPb = torch.empty(Z * T * Tp, device=dev); dS = torch.empty(Z * T * Tp, device=dev); dS2 = torch.empty(Z * T * Tp, device=dev)
dbd = K.relpos_band_buffer(Z, T, Pp, dev)
dqkv = torch.zeros(M, 3 * D, device=dev); dqkv2 = torch.zeros(M, 3 * D, device=dev)
tmp = torch.empty(M, D, device=dev); dp = torch.empty(P, D, device=dev); dp2 = torch.empty(P, D, device=dev)
dot = torch.empty(Z * T, device=dev)
du = torch.zeros(D, device=dev); dv = torch.zeros(D, device=dev)
bias_part = torch.empty(Z * ((T + 31) // 32) * 2 * DK, device=dev)
sq = math.sqrt(DK)

steps = {
 "old dP gemm": lambda: K.gemm(T, T, DK, dctx, c.qkv, dPb, mode_a=K.KC, lda=D, mode_b=K.KC, ldb=3 * D, ldc=Tp, b_off=2 * D, batch=Z, nb2=B, sa=(DK, T * D), sb=(DK, T * 3 * D), sc=(B * T * Tp, T * Tp)),
 "old softmax_bwd band": lambda: K.attn_softmax_bwd_relpos_band(c.attn, dPb, dS, dbd, Pp, c.pa, c.sa, sq, Z * T, T, Tp),
 "old dq_u gemm": lambda: K.gemm(T, DK, T, dS, c.qkv, dqkv, mode_a=K.KC, lda=Tp, mode_b=K.RC, ldb=3 * D, ldc=3 * D, b_off=D, batch=Z, nb2=B, sa=(B * T * Tp, T * Tp), sb=(DK, T * 3 * D), sc=(DK, T * 3 * D)),
 "old colsum u": lambda: K.colsum(dqkv, du, accumulate=True, M=M, N=D, ld=3 * D),
 "old dqv band": lambda: K.relpos_dqv(dbd, Pp, c.p, D, tmp, D, B, H, T),
 "old colsum v": lambda: K.colsum(tmp, dv, accumulate=True),
 "old add2d": lambda: K.add2d(tmp, D, dqkv, 3 * D, M, D),
 "old dp gemm": lambda: K.gemm(P, DK, B * T, dbd, c.q_v, dp, mode_a=K.RC, lda=Pp, mode_b=K.RC, ldb=DK, ldc=D, batch=H, nb2=1, sa=(B * T * Pp, 0), sb=(B * T * DK, 0), sc=(DK, 0)),
 "new prep": lambda: K.attn_bwd_prep(dctx, D, c.ctx, D, B, H, DK, T, dot, None, 0, 1),
 "new dscores": lambda: K.attn_dscores(dctx, D, c.qkv, 3 * D, c.attn, dot, dS2, None, 0, 1, B, H, DK, sq, c.pa, c.sa, T, Tp, v_off=2 * D),
 "new relpos_dq": lambda: K.relpos_dq(dS2, Tp, c.qkv, 3 * D, c.p, D, dqkv2, 3 * D, bias_part, B, H, T, k_off=D),
 "new relpos_dp(+reduces)": lambda: K.relpos_dp(dS2, Tp, c.q_v, 1, B, H, T, dp2, D, bias_part, None, du, dv, dqkv2, 3 * D),
}
tot = {"old": 0.0, "new": 0.0}
for name, f in steps.items():
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    tot[name.split()[0]] += ts[2]
    print(f"{name:28s} median {ts[2]:8.1f} us  min {ts[0]:8.1f}  max {ts[-1]:8.1f}", flush=True)
print(f"old chain {tot['old']:.1f} us, new chain {tot['new']:.1f} us per layer (B={B})")
from tests.helpers import rel_err
print("dS new vs old", rel_err(dS2.view(-1, Tp)[:, :T].cpu(), dS.view(-1, Tp)[:, :T].cpu()))
print("dp new vs old", rel_err(dp2.cpu(), dp.cpu()))
