"""Shared by the Mask-CTC tests and their fixture generator (tests/golden/make_maskctc_golden.py): the small-model
cases, seeded parameters with the <mask> row, our model's construction, and an fp64 restatement of the Mask-CTC
training step on the oracle's pieces (oracle/espnet_cpu.py), which the generator asserts equal to the reference's
fp64 step before a fixture is written."""
import math

import numpy as np
import torch

from oracle import espnet_cpu as O
from tests.helpers import small_cfg, token_list

B, T, LENS, ULENS = 3, 120, [120, 97, 64], [9, 5, 7]

# name -> (parameter seed, overrides of small_cfg("latest"): D = 64, 2 + 2 blocks, V = 32, ctc_weight 0.3)
CASES = {
    "base": (31, dict(lsm_weight=0.0)),
    "lsm": (32, dict(lsm_weight=0.1)),
    "noctc": (33, dict(ctc_weight=0.0, lsm_weight=0.1)),
    "lnorm": (34, dict(lsm_weight=0.1, length_normalized_loss=True)),
    "interctc": (35, dict(lsm_weight=0.1, interctc=True)),
}


def case_cfg(name):
    seed, over = CASES[name]
    over = dict(over)
    inter = over.pop("interctc", False)
    cfg = small_cfg("latest", blocks=3 if inter else 2)
    for k, v in over.items():
        setattr(cfg, k, v)
    if inter:
        cfg.enc.interctc_layer_idx = (1, 2)
        cfg.interctc_weight = 0.3
    return seed, cfg


def maskctc_params(cfg, seed, dtype=torch.float32):
    """oracle.deterministic_params plus the <mask> row of the decoder's embedding and output layer (a second seeded
    stream, so the first V rows are the plain model's)."""
    P = O.deterministic_params(cfg, seed, dtype)
    rng = np.random.Generator(np.random.PCG64(seed + 7919))
    D = cfg.enc.output_size
    extra = {"decoder.embed.0.weight": rng.standard_normal((1, D)),
             "decoder.output_layer.weight": rng.standard_normal((1, D)) / math.sqrt(D),
             "decoder.output_layer.bias": 0.05 * rng.standard_normal((1,))}
    for k, a in extra.items():
        P[k] = torch.cat([P[k], torch.tensor(a, dtype=dtype)], 0)
    return P


def batch(cfg, seed):
    return O.synthetic_batch(B, T, cfg.enc.input_size, cfg.vocab_size, LENS, ULENS, seed + 1)


def draws_from_targets(ys_out, ignore_id=-1):
    """mask_uniform's draws recovered from ys_out: the positions that carry a target."""
    return [np.nonzero(row != ignore_id)[0] for row in np.asarray(ys_out)]


def load_params(model, P):
    model.load_state_dict({k: P[k] for k in model.state_dict()}, strict=True)


def build_maskctc(cfg, device, dropout=None, report=False):
    from espnet_slurp_amd.asr.ctc import CTC
    from espnet_slurp_amd.asr.decoder.mlm_decoder import MLMDecoder
    from espnet_slurp_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_slurp_amd.asr.maskctc_model import MaskCTCModel
    from espnet_slurp_amd.layers.utterance_mvn import UtteranceMVN
    e, d = cfg.enc, cfg.dec
    p = e.dropout_rate if dropout is None else dropout
    enc = ConformerEncoder(input_size=e.input_size, output_size=e.output_size, attention_heads=e.attention_heads,
                           linear_units=e.linear_units, num_blocks=e.num_blocks, dropout_rate=p,
                           positional_dropout_rate=p, attention_dropout_rate=p, macaron_style=e.macaron_style,
                           rel_pos_type=e.rel_pos_type, use_cnn_module=e.use_cnn_module,
                           cnn_module_kernel=e.cnn_module_kernel, input_layer=e.input_layer,
                           interctc_layer_idx=list(e.interctc_layer_idx),
                           interctc_use_conditioning=e.interctc_use_conditioning)
    dec = MLMDecoder(vocab_size=cfg.vocab_size, encoder_output_size=e.output_size, attention_heads=d.attention_heads,
                     linear_units=d.linear_units, num_blocks=d.num_blocks, dropout_rate=p, positional_dropout_rate=p,
                     self_attention_dropout_rate=p, src_attention_dropout_rate=p)
    ctc = CTC(odim=cfg.vocab_size, encoder_output_size=e.output_size)
    m = MaskCTCModel(vocab_size=cfg.vocab_size, token_list=token_list(cfg.vocab_size), frontend=None, specaug=None,
                     normalize=UtteranceMVN(), preencoder=None, encoder=enc, postencoder=None, decoder=dec, ctc=ctc,
                     joint_network=None, ctc_weight=cfg.ctc_weight, interctc_weight=cfg.interctc_weight,
                     lsm_weight=cfg.lsm_weight, length_normalized_loss=cfg.length_normalized_loss, report_cer=report,
                     report_wer=report)
    m = m.to(device)
    m.flatten()
    return m


# ------------------------------------------------------------------ fp64 restatement on the oracle's pieces
def mlm_decoder(P, hs, hlens, ys_in, ys_in_lens, dcfg):
    """MLMDecoder.forward (mlm_decoder.py:109-130), dropout 0: the decoder of oracle.decoder with the target mask
    valid(i) & valid(j) instead of the causal one."""
    L = ys_in.size(1)
    valid = ~O.make_pad_mask(ys_in_lens, L)
    tgt_mask = valid[:, None, :] & valid[:, :, None]
    mem_mask = (~O.make_pad_mask(hlens, hs.size(1)))[:, None, :]
    D = hs.size(-1)
    x = P["decoder.embed.0.weight"][ys_in] * math.sqrt(D) + O.abs_pos_table(L, D).to(hs.dtype)
    H = dcfg.attention_heads
    for j in range(dcfg.num_blocks):
        pre = f"decoder.decoders.{j}"
        h = O.layer_norm(P, pre + ".norm1", x)
        x = x + O.mha(P, pre + ".self_attn", h, h, h, tgt_mask, H, 0.0, False)
        h = O.layer_norm(P, pre + ".norm2", x)
        x = x + O.mha(P, pre + ".src_attn", h, hs, hs, mem_mask, H, 0.0, False)
        h = O.layer_norm(P, pre + ".norm3", x)
        x = x + O.ffn(P, pre + ".feed_forward", h, "relu", 0.0, False)
    return O.linear(P, "decoder.output_layer", O.layer_norm(P, "decoder.after_norm", x))


def maskctc_forward(P, speech, slen, text, tlen, ys_in, ys_out, cfg):
    """MaskCTCModel.forward (maskctc_model.py:115-213) in train mode with every dropout 0 and the masks given."""
    text = text[:, : int(tlen.max())]
    feats = O.utterance_mvn(speech[:, : int(slen.max())], slen)
    hs, hlens = O.encoder(P, feats, slen, cfg.enc, {}, True)
    inter = None
    if isinstance(hs, tuple):
        hs, inter = hs
    stats = {}
    loss_ctc = None
    if cfg.ctc_weight != 0.0:
        loss_ctc = O.ctc_loss(P, hs, hlens, text, tlen, cfg.blank_id)
        stats["loss_ctc"] = loss_ctc.detach()
        if cfg.interctc_weight != 0.0 and inter:
            lic = 0.0
            for idx, h in inter:
                li = O.ctc_loss(P, h, hlens, text, tlen, cfg.blank_id)
                stats[f"loss_interctc_layer{idx}"] = li.detach()
                lic = lic + li
            loss_ctc = (1 - cfg.interctc_weight) * loss_ctc + cfg.interctc_weight * lic / len(inter)
    V1 = cfg.vocab_size + 1
    logits = mlm_decoder(P, hs, hlens, ys_in, tlen, cfg.dec)
    loss_mlm = O.label_smoothing_loss(logits, ys_out, V1, cfg.ignore_id, cfg.lsm_weight, cfg.length_normalized_loss)
    stats["loss_mlm"] = loss_mlm.detach()
    stats["acc_mlm"] = O.th_accuracy(logits.view(-1, V1), ys_out, cfg.ignore_id)
    loss = loss_mlm if cfg.ctc_weight == 0.0 else cfg.ctc_weight * loss_ctc + (1 - cfg.ctc_weight) * loss_mlm
    stats["loss"] = loss.detach()
    return loss, stats


def restated_grads(cfg, seed, g):
    """fp64 loss, stats and parameter gradients of a model fixture `g` (its batch and masks), on the CPU."""
    P = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k)
         for k, v in maskctc_params(cfg, seed, torch.float64).items()}
    speech, slen, text, tlen = batch(cfg, seed)
    loss, stats = maskctc_forward(P, speech.double(), slen, text, tlen, torch.from_numpy(g["ys_in"]),
                                  torch.from_numpy(g["ys_out"]), cfg)
    loss.backward()
    return loss, stats, {k: v.grad for k, v in P.items() if v.requires_grad and v.grad is not None}


# ------------------------------------------------------------------ mask-predict decoding cases
# name -> n_iterations and the mask count the generator aims the threshold at ("blank": a blank bias on ctc_lo
# instead, so that no token is left); the generator searches the input seed that satisfies the margins
DECODE_CASES = {
    "many": dict(n_iterations=3, want="ge"),      # mask_num >= n_iterations
    "few": dict(n_iterations=10, want="lt"),      # 0 < mask_num < n_iterations
    "none": dict(n_iterations=10, want="zero"),   # mask_num == 0
    "blank": dict(n_iterations=10, want="blank"),  # every frame blank: L == 0
    "one": dict(n_iterations=1, want="ge"),       # n_iterations = 1: one pass fills everything
}
DECODE_SEED = 41      # parameters of the decoding model (small_cfg)
DECODE_T = 120        # input frames of the decoding utterance (29 encoder frames)
CTC_SCALE = 12.0      # ctc_lo weight and bias are scaled by this, so that the posteriors are peaky


def decode_params(cfg, dtype=torch.float32, blank=False):
    P = maskctc_params(cfg, DECODE_SEED, dtype)
    P["ctc.ctc_lo.weight"] = P["ctc.ctc_lo.weight"] * CTC_SCALE
    P["ctc.ctc_lo.bias"] = P["ctc.ctc_lo.bias"] * CTC_SCALE
    if blank:
        P["ctc.ctc_lo.bias"][0] += 1000.0
    return P


def decode_speech(cfg, seed):
    speech, _, _, _ = O.synthetic_batch(1, DECODE_T, cfg.enc.input_size, cfg.vocab_size, [DECODE_T], [3], seed)
    return speech[0]
