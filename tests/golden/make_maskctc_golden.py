"""Mask-CTC fixtures from the REFERENCE's own classes (this container only, CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_maskctc_golden.py [meta] [model] [decode]

maskctc_meta.npz     state_dict keys / shapes of the reference MaskCTCModel (small model), mask_uniform outputs
                     under fixed NumPy seeds (ragged targets, one of length 1)
maskctc_model_<case>.npz   one training step of tests/maskctc_helpers.CASES in fp32 and fp64: the masks, the losses,
                     acc_mlm, per parameter the fp32 run's own gradient error against fp64, and the MLM decoder's
                     logits on a recorded encoder output.  The fp64 restatement the GPU test differentiates
                     (maskctc_helpers.maskctc_forward) is asserted equal to the reference's fp64 step here.
maskctc_decode.npz   MaskCTCInference.forward on recorded encoder outputs: the token row after every pass, the final
                     yseq, and the margins that make exact equality fair (asserted >= 100 x the reference's own
                     fp32-vs-fp64 deviation of the same quantity).

The fixtures are data; nothing of the reference's code travels with them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import refshim  # noqa: E402

refshim.install()

from espnet2.asr.ctc import CTC  # noqa: E402
from espnet2.asr.decoder.mlm_decoder import MLMDecoder  # noqa: E402
from espnet2.asr.encoder.conformer_encoder import ConformerEncoder  # noqa: E402
from espnet2.asr.maskctc_model import MaskCTCInference, MaskCTCModel  # noqa: E402
from espnet2.layers.utterance_mvn import UtteranceMVN  # noqa: E402
from espnet.nets.pytorch_backend.maskctc.add_mask_token import mask_uniform  # noqa: E402

from tests import maskctc_helpers as MH  # noqa: E402
from tests.helpers import rel_err, small_cfg, token_list  # noqa: E402

torch.set_num_threads(8)
MARGIN = 100.0


def build_reference(cfg):
    e, d = cfg.enc, cfg.dec
    enc = ConformerEncoder(
        input_size=e.input_size, output_size=e.output_size, attention_heads=e.attention_heads,
        linear_units=e.linear_units, num_blocks=e.num_blocks, dropout_rate=0.0, positional_dropout_rate=0.0,
        attention_dropout_rate=0.0, input_layer=e.input_layer, normalize_before=True, macaron_style=e.macaron_style,
        rel_pos_type=e.rel_pos_type, pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn",
        activation_type="swish", use_cnn_module=e.use_cnn_module, cnn_module_kernel=e.cnn_module_kernel,
        interctc_layer_idx=list(e.interctc_layer_idx), interctc_use_conditioning=e.interctc_use_conditioning)
    dec = MLMDecoder(vocab_size=cfg.vocab_size, encoder_output_size=e.output_size, attention_heads=d.attention_heads,
                     linear_units=d.linear_units, num_blocks=d.num_blocks, dropout_rate=0.0,
                     positional_dropout_rate=0.0, self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0)
    ctc = CTC(odim=cfg.vocab_size, encoder_output_size=e.output_size)
    return MaskCTCModel(vocab_size=cfg.vocab_size, token_list=token_list(cfg.vocab_size), frontend=None, specaug=None,
                        normalize=UtteranceMVN(), preencoder=None, encoder=enc, postencoder=None, decoder=dec, ctc=ctc,
                        joint_network=None, ctc_weight=cfg.ctc_weight, interctc_weight=cfg.interctc_weight,
                        lsm_weight=cfg.lsm_weight, length_normalized_loss=cfg.length_normalized_loss,
                        report_cer=False, report_wer=False)


def load(model, P):
    sd = model.state_dict()
    assert set(sd) <= set(P), set(sd) - set(P)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(P[k].shape), (k, sd[k].shape, P[k].shape)
    model.load_state_dict({k: P[k] for k in sd})


def meta_fixture():
    cfg = small_cfg("latest")
    ref = build_reference(cfg)
    sd = ref.state_dict()
    keys = list(sd)
    shapes = np.full((len(keys), 4), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, : sd[k].dim()] = list(sd[k].shape)
    out = dict(model_keys=np.array(keys), model_shapes=shapes, vocab_size=np.int64(ref.vocab_size),
               mask_token=np.int64(ref.mask_token), eos=np.int64(ref.eos), token_last=np.array(ref.token_list[-1]))
    # mask_uniform under fixed NumPy seeds: ragged targets, one of a single token
    ys_pad = torch.full((4, 6), -1, dtype=torch.long)
    rng = np.random.Generator(np.random.PCG64(3))
    for i, n in enumerate([6, 1, 4, 2]):
        ys_pad[i, :n] = torch.from_numpy(rng.integers(2, 31, size=n))
    out["mu_ys_pad"] = ys_pad.numpy()
    for s in (0, 5, 11):
        np.random.seed(s)
        yi, yo = mask_uniform(ys_pad, 32, 31, -1)
        out[f"mu_in_{s}"], out[f"mu_out_{s}"] = yi.numpy(), yo.numpy()
    np.savez_compressed(os.path.join(HERE, "maskctc_meta.npz"), **out)
    print("meta:", len(keys), "keys; vocab", int(out["vocab_size"]), "mask", int(out["mask_token"]))


def model_fixture(name):
    seed, cfg = MH.case_cfg(name)
    out = {}
    runs = {}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        model = build_reference(cfg).to(dt)
        load(model, MH.maskctc_params(cfg, seed, dt))
        model.train()
        speech, slen, text, tlen = MH.batch(cfg, seed)
        orig = model.decoder.forward
        rec = {"decoder": orig}

        def spy(hs, hlens, ys_in, ys_lens, rec=rec, orig=orig):
            rec["hs"], rec["hlens"], rec["ys_in"] = hs.detach(), hlens, ys_in.clone()
            rec["logits"], ol = orig(hs, hlens, ys_in, ys_lens)
            return rec["logits"], ol

        model.decoder.forward = spy
        crit = model.criterion_mlm.forward

        def spy_crit(x, target, rec=rec, crit=crit):
            rec["ys_out"] = target.clone()
            return crit(x, target)

        model.criterion_mlm.forward = spy_crit
        np.random.seed(seed)
        loss, stats, weight = model(speech.to(dt), slen.clone(), text.clone(), tlen.clone())
        loss.backward()
        runs[tag] = (model, rec, loss, stats)
        out[f"loss_{tag}"] = np.float64(loss.item())
        for k in ("loss_ctc", "loss_mlm", "acc_mlm"):
            if stats.get(k) is not None:
                out[f"{k}_{tag}"] = np.float64(float(stats[k]))
        for k in stats:
            if k.startswith("loss_interctc_layer"):
                out[f"{k}_{tag}"] = np.float64(float(stats[k]))
    m32, r32, _, s32 = runs["f32"]
    m64, r64, l64, s64 = runs["f64"]
    assert torch.equal(r32["ys_in"], r64["ys_in"]) and torch.equal(r32["ys_out"], r64["ys_out"])
    out["stat_keys"] = np.array(sorted(s64))
    out["ys_in"], out["ys_out"] = r64["ys_in"].numpy(), r64["ys_out"].numpy()
    g64 = {n: p.grad for n, p in m64.named_parameters() if p.grad is not None}
    for n, p in m32.named_parameters():
        out["eref/" + n] = np.float64(rel_err(p.grad.numpy(), g64[n].numpy()))
    # the restatement the GPU test differentiates must be the reference's fp64 step
    loss, stats, G = MH.restated_grads(cfg, seed, out)
    scale = max(float(g.abs().max()) for g in g64.values())
    worst = max((float((G[n] - g).abs().max()) / scale, n) for n, g in g64.items())
    dl = abs(loss.item() - l64.item())
    print(f"{name}: loss f64 {l64.item():.9f} f32 {out['loss_f32']:.9f}; restatement |dloss| {dl:.2e} worst grad "
          f"{worst[0]:.2e} ({worst[1]})")
    assert dl < 1e-10 and worst[0] < 1e-9, (dl, worst)
    assert abs(stats["acc_mlm"] - float(s64["acc_mlm"])) < 1e-12
    # the decoder on its own: both precisions on the SAME recorded encoder output (the fp64 run's, rounded to fp32)
    hs = r64["hs"].float()
    lg = {}
    for tag, (m, r, _, _) in runs.items():
        dt = torch.float32 if tag == "f32" else torch.float64
        with torch.no_grad():
            lg[tag] = r["decoder"](hs.to(dt), r["hlens"], r["ys_in"], MH.batch(cfg, seed)[3])[0]
    valid = (~MH.O.make_pad_mask(MH.batch(cfg, seed)[3], lg["f64"].shape[1])).numpy()
    out["dec_hs"] = hs.numpy()
    out["dec_hlens"] = np.asarray(r64["hlens"], dtype=np.int64)
    out["dec_logits_f64"] = lg["f64"].numpy()
    out["dec_valid"] = valid
    out["dec_eref"] = np.float64(np.abs(lg["f32"].double().numpy() - lg["f64"].numpy())[valid].max())
    out["seed"] = np.int64(seed)
    np.savez_compressed(os.path.join(HERE, f"maskctc_model_{name}.npz"), **out)
    print(f"{name}: stats {sorted(s64)}; decoder logits e_ref {float(out['dec_eref']):.2e}; worst grad e_ref "
          f"{max(float(v) for k, v in out.items() if k.startswith('eref/')):.2e}")


class Recorder(torch.nn.Module):
    """Stands where MaskCTCInference.mlm is: keeps every pass's input row and output logits."""

    def __init__(self, mlm):
        super().__init__()
        self.mlm, self.rows, self.preds = mlm, [], []

    def forward(self, enc, elens, y_in, ylens):
        pred, ol = self.mlm(enc, elens, y_in, ylens)
        self.rows.append(y_in[0].clone())
        self.preds.append(pred[0].detach().clone())
        return pred, ol


def run_reference_decode(model, enc, n_iterations, thr):
    inf = MaskCTCInference(asr_model=model, n_iterations=n_iterations, threshold_probability=thr)
    inf.mlm = Recorder(model.decoder)
    with torch.no_grad():
        hyp = inf(enc)
        lp = model.ctc.log_softmax(enc.unsqueeze(0))[0]
    rec = inf.mlm
    rows = rec.rows + [hyp.yseq[1:-1].clone()]  # the row before pass 1, ..., after the last pass
    return hyp.yseq, rows, rec.preds, lp


def top2_gap(x):
    s = np.sort(x, axis=-1)
    return s[..., -1] - s[..., -2]


def token_probs(lp):
    """Greedy CTC tokens and their probabilities (maskctc_model.py:288-305 restated on a (T, V) log-softmax)."""
    ids = lp.argmax(-1)
    p = np.exp(lp.max(-1))
    toks, probs = [], []
    for t in range(len(ids)):
        if t > 0 and ids[t] == ids[t - 1]:
            probs[-1] = max(probs[-1], p[t])
        else:
            toks.append(int(ids[t]))
            probs.append(p[t])
    keep = [i for i, k in enumerate(toks) if k != 0]
    return np.array([toks[i] for i in keep], dtype=np.int64), np.array([probs[i] for i in keep])


def decode_case(name, spec, cfg, models):
    blank = spec["want"] == "blank"
    m32, m64 = models[blank]
    mask = m64.mask_token
    for seed in range(500, 560):
        speech = MH.decode_speech(cfg, seed)
        lengths = torch.tensor([speech.shape[0]])
        with torch.no_grad():
            enc64 = m64.encode(speech.double().unsqueeze(0), lengths)[0][0]
        enc = enc64.float()  # the recorded encoder output: both precisions decode this
        lp32 = m32.ctc.log_softmax(enc.unsqueeze(0))[0].detach().numpy()
        lp64 = m64.ctc.log_softmax(enc.double().unsqueeze(0))[0].detach().numpy()
        toks, p64 = token_probs(lp64)
        toks32, p32 = token_probs(lp32.astype(np.float64))
        L = len(toks)
        n_it = spec["n_iterations"]
        # the threshold sits in the widest gap of the sorted token probabilities that gives the wanted count
        if spec["want"] == "blank":
            if L != 0:
                continue
            thr = 0.99
        else:
            if L < 12 or not np.array_equal(toks, toks32):
                continue
            ps = np.sort(p64)
            if spec["want"] == "zero":
                thr = float(ps[0]) * 0.5
            else:
                cands = range(max(n_it, 4), L) if spec["want"] == "ge" else range(2, min(n_it, L))
                gaps = [(ps[c] - ps[c - 1], c) for c in cands]  # c tokens below the threshold
                if not gaps:
                    continue
                gap, c = max(gaps)
                thr = float(0.5 * (ps[c] + ps[c - 1]))
        y32, rows32, preds32, _ = run_reference_decode(m32, enc, n_it, thr)
        y64, rows64, preds64, _ = run_reference_decode(m64, enc.double(), n_it, thr)
        if not torch.equal(y32, y64) or len(rows32) != len(rows64) or any(
                not torch.equal(a, b) for a, b in zip(rows32, rows64)):
            continue
        dev = dict(argmax=float(np.abs(lp32 - lp64).max()), prob=0.0, logit=0.0)
        mar = dict(argmax=float(top2_gap(lp64).min()), prob=np.inf, top1=np.inf, topk=np.inf)
        if L:
            dev["prob"] = float(np.abs(p32 - p64).max())
            mar["prob"] = float(np.abs(p64 - thr).min())
        mask_num = int((rows64[0] == mask).sum()) if L and preds64 else 0
        if spec["want"] == "ge" and not mask_num >= n_it:
            continue
        if spec["want"] == "lt" and not 0 < mask_num < n_it:
            continue
        if spec["want"] == "zero" and (mask_num != 0 or preds64):
            continue
        num_iter = len(preds64)
        for t, (a, b) in enumerate(zip(preds32, preds64)):
            a, b = a.double().numpy(), b.numpy()
            midx = np.nonzero(rows64[t].numpy() == mask)[0]
            dev["logit"] = max(dev["logit"], float(np.abs(a - b)[midx].max()))
            sc = b[midx].max(-1)
            if t < num_iter - 1:  # a top-k pass: the chosen positions' top-1 gaps, and the k-th against the (k+1)-th
                k = mask_num // num_iter
                order = np.argsort(-sc)
                mar["top1"] = min(mar["top1"], float(top2_gap(b[midx[order[:k]]]).min()))
                if len(order) > k:
                    mar["topk"] = min(mar["topk"], float(sc[order[k - 1]] - sc[order[k]]))
            else:
                mar["top1"] = min(mar["top1"], float(top2_gap(b[midx]).min()))
        ok = (mar["argmax"] >= MARGIN * dev["argmax"] and mar["prob"] >= MARGIN * dev["prob"]
              and mar["top1"] >= MARGIN * dev["logit"] and mar["topk"] >= MARGIN * dev["logit"])
        print(f"decode {name}: seed {seed} L {L} mask_num {mask_num} passes {num_iter} thr {thr:.6f} dev {dev} "
              f"margins {mar} -> {'ok' if ok else 'retry'}", flush=True)
        if not ok:
            continue
        out = {f"{name}/enc": enc.numpy(), f"{name}/seed": np.int64(seed), f"{name}/thr": np.float64(thr),
               f"{name}/n_iterations": np.int64(n_it), f"{name}/yseq": y64.numpy(), f"{name}/L": np.int64(L),
               f"{name}/mask_num": np.int64(mask_num), f"{name}/passes": np.int64(num_iter),
               f"{name}/blank": np.int64(blank),
               f"{name}/rows": (np.stack([r.numpy() for r in rows64]) if L else np.zeros((1, 0), dtype=np.int64)),
               f"{name}/tok_prob": p32.astype(np.float32), f"{name}/lp": lp32, f"{name}/tokens": toks}
        for k, v in dev.items():
            out[f"{name}/dev_{k}"] = np.float64(v)
        for k, v in mar.items():
            out[f"{name}/margin_{k}"] = np.float64(v)
        if preds64:  # the first pass's logits: the prepared-memory pass against run_forward and fp64
            out[f"{name}/pred0_f64"] = preds64[0].numpy()
            out[f"{name}/pred0_eref"] = np.float64(np.abs(preds32[0].double().numpy() - preds64[0].numpy()).max())
        return out
    raise RuntimeError(f"decode {name}: no input satisfies the margins")


def decode_fixture():
    cfg = small_cfg("latest")
    models = {}
    for blank in (False, True):
        pair = []
        for dt in (torch.float32, torch.float64):
            m = build_reference(cfg).to(dt)
            load(m, MH.decode_params(cfg, dt, blank=blank))
            m.eval()
            pair.append(m)
        models[blank] = pair
    out = {}
    for name, spec in MH.DECODE_CASES.items():
        out.update(decode_case(name, spec, cfg, models))
    np.savez_compressed(os.path.join(HERE, "maskctc_decode.npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["meta", "model", "decode"]
    if "meta" in which:
        meta_fixture()
    if "model" in which:
        for name in MH.CASES:
            model_fixture(name)
    if "decode" in which:
        decode_fixture()
