"""Golden vectors for the Transformer LM and LM shallow fusion, generated in THIS container with the reference's own
TransformerLM / ESPnetLanguageModel / BeamSearch / BatchBeamSearch (imported through refshim), in fp32 and in fp64.
Writes tests/golden/lm.npz and tests/golden/lm_small.pt (data only).
Run:  python tests/golden/make_lm_golden.py

lm.npz:
  {A,B,C}.p.<name>        parameters of three small LMs (V = 32, embed_unit 16, dropout 0), the seeded fill below
                            A: pos_enc None, att_unit 64, head 2 (d_k 32), unit 96, layer 2          (seed 1)
                            B: "sinusoidal",  att_unit 64, head 4 (d_k 16), unit 96, layer 2          (seed 3)
                            C: pos_enc None, att_unit 128, head 2 (d_k 64), unit 64, layer 1         (seed 5)
  keys_json               {"A" | "B" | "C" | "transformer2": [[state_dict key, shape], ...]} (transformer2: the
                          LibriSpeech train_lm_transformer2 config over 5000 tokens, built on `meta`)
  fwd_text, fwd_lens      a ragged batch (lengths 7, 5, 2), text padded with 0
  {A,B,C}.fwd_logits{32,64}, .nll{32,64}   ESPnetLanguageModel.nll's input -> lm.forward logits, and nll
  bs_toks                 (5, 66) the rows' tokens (column 0 = <sos>; rows 1 and 3 carry token 0 inside, whole runs
                          included); prefixes follow tests/test_gpu_decoder_step.py: rows reordered by PARENTS after
                          L in REORDER_AFTER
  {A,B,C}.bs_logp{32,64}  (8, 5, V) batch_score log-probabilities at L in CHECK
  {A,B}.score{32,64}      score() on the prefix [31, 4, 0, 7, 0]
  fuse_{a_lm,b_lm}_{plain,batch}_{yseq,score}, fuse_*_cfg   n-best lists of the joint search with the LM on the model /
                          encoder output of inference.npz (cfg = ctc_weight, beam, penalty, lm_weight)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import refshim  # noqa: E402

refshim.install()
from tests.golden.make_golden import build_reference, load_params, small_cfg  # noqa: E402

V = 32
LM_CFGS = dict(A=dict(pos_enc=None, embed_unit=16, att_unit=64, head=2, unit=96, layer=2, dropout_rate=0.0),
               B=dict(pos_enc="sinusoidal", embed_unit=16, att_unit=64, head=4, unit=96, layer=2, dropout_rate=0.0),
               C=dict(pos_enc=None, embed_unit=16, att_unit=128, head=2, unit=64, layer=1, dropout_rate=0.0))
LM_SEEDS = dict(A=1, B=3, C=5)
TRANSFORMER2 = dict(pos_enc=None, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16, dropout_rate=0.1)
CHECK = (1, 2, 16, 17, 63, 64, 65, 66)
PARENTS = [3, 3, 0, 1, 4]
REORDER_AFTER = (5, 40)
LMAX = 66
REL = 1e-3


def seeded_fill(model, seed):
    """Draws in named_parameters() order: LayerNorm weights 1 + 0.1 randn, other vectors 0.1 randn, matrices
    randn * 1.5 / sqrt(fan_in)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if p.dim() == 1:
                is_ln_w = name.endswith(".weight") and ("norm" in name or ".embed.1." in name)
                p.copy_(1.0 + 0.1 * r if is_ln_w else 0.1 * r)
            else:
                p.copy_(r * 1.5 / p.shape[1] ** 0.5)


def pinned_ranks(want_s):
    out = []
    for i, s in enumerate(want_s):
        a = 2 * REL * abs(s)
        if all(abs(s - want_s[j]) > a for j in (i - 1, i + 1) if 0 <= j < len(want_s)):
            out.append(i)
    return out


def history(toks):
    ys, hist = toks.clone(), {}
    for L in range(1, LMAX + 1):
        ys[:, L - 1] = toks[:, L - 1]
        hist[L] = ys[:, :L].clone()
        if L in REORDER_AFTER:
            ys = ys[PARENTS].clone()
    return hist


def main():
    from espnet.nets.batch_beam_search import BatchBeamSearch
    from espnet.nets.beam_search import BeamSearch
    from espnet.nets.scorers.ctc import CTCPrefixScorer
    from espnet.nets.scorers.length_bonus import LengthBonus
    from espnet2.lm.espnet_model import ESPnetLanguageModel
    from espnet2.lm.transformer_lm import TransformerLM

    out, keys = {}, {}
    g = torch.Generator().manual_seed(9)
    text = torch.zeros(3, 7, dtype=torch.int64)
    lens = torch.tensor([7, 5, 2])
    for i, l in enumerate(lens):
        text[i, :l] = torch.randint(1, V - 1, (int(l),), generator=g)
    out["fwd_text"], out["fwd_lens"] = text.numpy(), lens.numpy()
    toks = torch.randint(1, V - 1, (5, LMAX), generator=g)
    toks[:, 0] = V - 1
    toks[1, [3, 9, 10, 11, 30, 62, 63]] = 0
    toks[3, 1] = 0
    toks[3, 20:40] = 0
    toks[3, 64] = 0
    out["bs_toks"] = toks.numpy()
    hist = history(toks)
    prefix = torch.tensor([31, 4, 0, 7, 0])

    lms = {}
    for tag, conf in LM_CFGS.items():
        lm = TransformerLM(V, **conf)
        seeded_fill(lm, LM_SEEDS[tag])
        lm.eval()
        lms[tag] = lm
        keys[tag] = [[k, list(v.shape)] for k, v in lm.state_dict().items()]
        for k, v in lm.state_dict().items():
            out[f"{tag}.p.{k}"] = v.numpy().copy()
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            m = ESPnetLanguageModel(TransformerLM(V, **conf), V)
            m.lm.load_state_dict(lm.state_dict())
            m = m.to(dt).eval()
            with torch.no_grad():
                x = torch.nn.functional.pad(text, [1, 0], "constant", m.eos)
                for i, l in enumerate(lens):
                    x[i, l + 1:] = 0
                logits, _ = m.lm(x, None)
                nll, xl = m.nll(text, lens)
                out[f"{tag}.fwd_logits{bits}"] = logits.numpy()
                out[f"{tag}.nll{bits}"] = nll.numpy()
                assert xl.tolist() == [8, 6, 3]
                lp = [m.lm.batch_score(hist[L], [None] * 5, None)[0].numpy() for L in CHECK]
                out[f"{tag}.bs_logp{bits}"] = np.stack(lp)
                if tag in ("A", "B"):
                    out[f"{tag}.score{bits}"] = m.lm.score(prefix, None, None)[0].numpy()
    with torch.device("meta"):
        t2 = TransformerLM(5000, **TRANSFORMER2)
    keys["transformer2"] = [[k, list(v.shape)] for k, v in t2.state_dict().items()]
    out["keys_json"] = np.array(json.dumps(keys))
    torch.save(ESPnetLanguageModel(lms["A"], V).state_dict(), os.path.join(HERE, "lm_small.pt"))

    # fused n-best lists on the model / encoder output of inference.npz
    inf = np.load(os.path.join(HERE, "inference.npz"))
    cfg = small_cfg("latest", D=64, blocks=2, V=V)
    model = build_reference(cfg)
    load_params(model, cfg, 21)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if "bn." + name in inf:
                buf.copy_(torch.tensor(inf["bn." + name]))
    model.eval()
    with torch.no_grad():
        enc, _ = model.encode(torch.tensor(inf["speech"]), torch.tensor([inf["speech"].shape[1]]))
    assert float((enc[0] - torch.tensor(inf["enc"])).abs().max()) <= 1e-5
    for tag, base, which, ctc_w, beam, penalty, lm_w in (("a_lm", "a", "A", 0.3, 4, 0.0, 0.6),
                                                         ("b_lm", "b", "B", 0.5, 6, 0.2, 0.3)):
        scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(ctc=model.ctc, eos=model.eos),
                       length_bonus=LengthBonus(V), lm=lms[which])
        weights = dict(decoder=1.0 - ctc_w, ctc=ctc_w, length_bonus=penalty, lm=lm_w)
        for kind, cls in (("plain", BeamSearch), ("batch", BatchBeamSearch)):
            bs = BeamSearch(scorers=scorers, weights=weights, beam_size=beam, vocab_size=V, sos=model.sos,
                            eos=model.eos, token_list=None, pre_beam_score_key="full")
            bs.__class__ = cls
            with torch.no_grad():
                hyps = bs(x=enc[0], maxlenratio=0.0, minlenratio=0.0)
            n, L = len(hyps), max(len(h.yseq) for h in hyps)
            ys = np.full((n, L), -1, dtype=np.int64)
            for i, h in enumerate(hyps):
                ys[i, : len(h.yseq)] = h.yseq.numpy()
            sc = np.array([float(h.score) for h in hyps])
            out[f"fuse_{tag}_{kind}_yseq"], out[f"fuse_{tag}_{kind}_score"] = ys, sc
            pins = pinned_ranks(sc)
            base_best = inf[f"bs_{base}_{kind}_yseq"][0]
            print(tag, kind, "pinned", pins, "best", hyps[0].yseq.tolist(), float(sc[0]), "lengths",
                  sorted({len(h.yseq) for h in hyps}))
            assert pins[:3] == [0, 1, 2], (tag, kind, pins)
            assert hyps[0].yseq.tolist() != base_best[base_best >= 0].tolist(), (tag, kind, "the LM changes nothing")
        out[f"fuse_{tag}_cfg"] = np.array([ctc_w, beam, penalty, lm_w])
    np.savez_compressed(os.path.join(HERE, "lm.npz"), **out)
    print("wrote lm.npz", os.path.getsize(os.path.join(HERE, "lm.npz")), "bytes; lm_small.pt",
          os.path.getsize(os.path.join(HERE, "lm_small.pt")), "bytes")


if __name__ == "__main__":
    main()
