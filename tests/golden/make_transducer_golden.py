"""Transducer fixtures from the REFERENCE's own classes (this container only, CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_transducer_golden.py [meta] [model | model=<case>] [search] [eval]

transducer_meta.npz          state_dict keys / shapes of the reference ESPnetASRModel with a joint network, the stats
                             keys per configuration (ctc_weight 0.0 / 0.3, train / eval), get_transducer_task_io on a
                             ragged batch
transducer_model_<case>.npz  one training step of tests/transducer_helpers.CASES in fp32 and fp64: the losses, per
                             parameter the fp64 gradient's norm / maximum and the fp32 run's own errors against fp64,
                             the eval-mode stats keys and loss, three torch.optim.Adam steps.  The torch
                             restatement the GPU test differentiates (transducer_helpers.transducer_forward) is
                             asserted equal to the reference's fp64 step here.
transducer_search.npz        BeamSearchTransducer (greedy; default at beams 2 and 5, nbest 3) on recorded encoder
                             outputs: the n-best token lists and scores, the per-call log-probability rows, the
                             smallest decision margin and the largest fp32-vs-fp64 score distance (a case is kept only
                             when the fp32 and fp64 n-best lists are identical, the margin is >= 100 x the distance
                             and the best hypothesis is non-empty).

transducer_eval.npz          eval-mode cer_transducer / wer_transducer of the decoding models on short batches, kept
                             under the same margin rule (after `search`: it reads the accepted models from there)

`warprnnt_pytorch` is not installed: tests/rnnt_helpers.RNNTLoss (a plain-torch lattice over log_softmax(acts), mean
reduction) is registered under that name before the reference is imported.  The fixtures are data; nothing of the
reference's code travels with them.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests import rnnt_helpers  # noqa: E402

_w = types.ModuleType("warprnnt_pytorch")
_w.RNNTLoss = rnnt_helpers.RNNTLoss
sys.modules["warprnnt_pytorch"] = _w

import refshim  # noqa: E402

refshim.install()

from espnet2.asr.ctc import CTC  # noqa: E402
from espnet2.asr.decoder.transducer_decoder import TransducerDecoder  # noqa: E402
from espnet2.asr.encoder.conformer_encoder import ConformerEncoder  # noqa: E402
from espnet2.asr.encoder.transformer_encoder import TransformerEncoder  # noqa: E402
from espnet2.asr.espnet_model import ESPnetASRModel  # noqa: E402
from espnet2.asr.transducer.beam_search_transducer import BeamSearchTransducer  # noqa: E402
from espnet2.asr_transducer.joint_network import JointNetwork  # noqa: E402
from espnet2.asr_transducer.utils import get_transducer_task_io  # noqa: E402
from espnet2.layers.utterance_mvn import UtteranceMVN  # noqa: E402

from espnet_slurp_amd.asr.transducer.beam_search_transducer import default_beam_search  # noqa: E402
from tests import transducer_helpers as TH  # noqa: E402
from tests.helpers import token_list  # noqa: E402

torch.set_num_threads(8)
MARGIN = 100.0


def build_reference(cfg, tc, report=True):
    e = cfg.enc
    if e.kind == "conformer":
        enc = ConformerEncoder(
            input_size=e.input_size, output_size=e.output_size, attention_heads=e.attention_heads,
            linear_units=e.linear_units, num_blocks=e.num_blocks, dropout_rate=0.0, positional_dropout_rate=0.0,
            attention_dropout_rate=0.0, input_layer=e.input_layer, normalize_before=True,
            macaron_style=e.macaron_style, rel_pos_type=e.rel_pos_type, pos_enc_layer_type="rel_pos",
            selfattention_layer_type="rel_selfattn", activation_type="swish", use_cnn_module=e.use_cnn_module,
            cnn_module_kernel=e.cnn_module_kernel)
    else:
        enc = TransformerEncoder(
            input_size=e.input_size, output_size=e.output_size, attention_heads=e.attention_heads,
            linear_units=e.linear_units, num_blocks=e.num_blocks, dropout_rate=0.0, positional_dropout_rate=0.0,
            attention_dropout_rate=0.0, input_layer="conv2d")
    dec = TransducerDecoder(cfg.vocab_size, rnn_type="lstm", num_layers=tc.num_layers, hidden_size=tc.hidden_size,
                            dropout=0.0, dropout_embed=0.0, embed_pad=0)
    joint = JointNetwork(cfg.vocab_size, e.output_size, tc.hidden_size, joint_space_size=tc.joint_space_size,
                         joint_activation_type=tc.joint_activation_type)
    ctc = CTC(odim=cfg.vocab_size, encoder_output_size=e.output_size)
    return ESPnetASRModel(vocab_size=cfg.vocab_size, token_list=token_list(cfg.vocab_size), frontend=None,
                          specaug=None, normalize=UtteranceMVN(), preencoder=None, encoder=enc, postencoder=None,
                          decoder=dec, ctc=ctc, joint_network=joint, ctc_weight=cfg.ctc_weight, report_cer=report,
                          report_wer=report)


class default_dtype:
    """The reference's TransducerDecoder.init_state makes its zero state in torch's default dtype: the fp64 runs set
    it to float64 around every call of the model."""

    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dt)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def load(model, P):
    sd = model.state_dict()
    assert set(sd) <= set(P), set(sd) - set(P)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(P[k].shape), (k, sd[k].shape, P[k].shape)
    model.load_state_dict({k: P[k] for k in sd})


def meta_fixture():
    out = {}
    for name in ("tf_l1", "tf_l2_ctc"):
        seed, cfg, tc = TH.case_cfg(name)
        tag = "ctc" if cfg.ctc_weight else "noctc"
        ref = build_reference(cfg, tc)
        load(ref, TH.transducer_params(cfg, tc, seed))
        sd = ref.state_dict()
        keys = list(sd)
        shapes = np.full((len(keys), 4), -1, dtype=np.int64)
        for i, k in enumerate(keys):
            shapes[i, : sd[k].dim()] = list(sd[k].shape)
        out[f"{tag}.keys"], out[f"{tag}.shapes"] = np.array(keys), shapes
        speech, slen, text, tlen = TH.batch(cfg, seed)
        for mode in ("train", "eval"):
            ref.train(mode == "train")
            with torch.no_grad():
                _, stats, _ = ref(speech, slen.clone(), text.clone(), tlen.clone())
            out[f"{tag}.{mode}.stat_keys"] = np.array(list(stats))
            out[f"{tag}.{mode}.stat_none"] = np.array([stats[k] is None for k in stats])
        ref2 = build_reference(cfg, tc, report=False)  # both report flags off: the CTC error calculator's quirk
        out[f"{tag}.noreport.has_error_calculator"] = np.bool_(ref2.error_calculator is not None)
        out[f"{tag}.noreport.has_error_calculator_trans"] = np.bool_(ref2.error_calculator_trans is not None)
    text = torch.tensor([[5, 9, 3, -1, -1], [7, -1, -1, -1, -1], [2, 2, 8, 4, 6]])
    dec_in, target, t_len, u_len = get_transducer_task_io(text, torch.tensor([11, 9, 4]), ignore_id=-1, blank_id=0)
    out.update(io_text=text.numpy(), io_decoder_in=dec_in.numpy(), io_target=target.numpy().astype(np.int64),
               io_t_len=t_len.numpy().astype(np.int64), io_u_len=u_len.numpy().astype(np.int64))
    np.savez_compressed(os.path.join(HERE, "transducer_meta.npz"), **out)
    print("meta:", {k: (v.tolist() if v.size < 12 else v.shape) for k, v in out.items() if "stat" in k or "has_" in k})


def model_fixture(name):
    seed, cfg, tc = TH.case_cfg(name)
    out = {"seed": np.int64(seed)}
    runs = {}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        model = build_reference(cfg, tc).to(dt)
        load(model, TH.transducer_params(cfg, tc, seed, dt))
        model.train()
        speech, slen, text, tlen = TH.batch(cfg, seed)
        with default_dtype(dt):
            loss, stats, _ = model(speech.to(dt), slen.clone(), text.clone(), tlen.clone())
        loss.backward()
        runs[tag] = (model, loss, stats)
        out[f"loss_{tag}"] = np.float64(loss.item())
        for k in ("loss_ctc", "loss_transducer"):
            if stats.get(k) is not None:
                out[f"{k}_{tag}"] = np.float64(float(stats[k]))
        model.eval()
        with torch.no_grad(), default_dtype(dt):
            _, es, _ = model(speech.to(dt), slen.clone(), text.clone(), tlen.clone())
        out[f"eval.loss_{tag}"] = np.float64(float(es["loss"]))
        if tag == "f64":
            out["eval.stat_keys"] = np.array(list(es))
            out["eval.stat_none"] = np.array([es[k] is None for k in es])
    m32, _, _ = runs["f32"]
    m64, l64, s64 = runs["f64"]
    out["stat_keys"] = np.array(list(s64))
    out["stat_none"] = np.array([s64[k] is None for k in s64])
    g64 = {n: p.grad for n, p in m64.named_parameters() if p.grad is not None}
    for n, p in m32.named_parameters():
        g, r = p.grad.double(), g64[n]
        gm = float(r.abs().max())
        out["gmax_f64/" + n] = np.float64(gm)
        out["gn_f64/" + n] = np.float64(float(r.norm()))
        out["gn_f32/" + n] = np.float64(float(g.norm()))
        out["emax_f32/" + n] = np.float64(float((g - r).abs().max()))
    # the restatement the GPU test differentiates must be the reference's fp64 step
    loss, stats, G = TH.restated_grads(name)
    scale = max(float(g.abs().max()) for g in g64.values())
    worst = max((float((G[n] - g).abs().max()) / scale, n) for n, g in g64.items())
    dl = abs(loss.item() - l64.item())
    print(f"{name}: loss f64 {l64.item():.9f} f32 {out['loss_f32']:.9f}; restatement |dloss| {dl:.2e} worst grad "
          f"{worst[0]:.2e} ({worst[1]}); stats {list(s64)}")
    assert dl < 1e-10 and worst[0] < 1e-9, (dl, worst)
    assert set(G) == set(g64), set(G) ^ set(g64)
    # three Adam steps (lr 1e-3, clip 5.0) on the same batch, as the eager Trainer runs them
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        model = build_reference(cfg, tc).to(dt)
        load(model, TH.transducer_params(cfg, tc, seed, dt))
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        speech, slen, text, tlen = TH.batch(cfg, seed)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            with default_dtype(dt):
                loss, _, _ = model(speech.to(dt), slen.clone(), text.clone(), tlen.clone())
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
            opt.step()
            losses.append(loss.item())
        out[f"steps.loss_{tag}"] = np.array(losses, dtype=np.float64)
    print(f"{name}: steps f64 {out['steps.loss_f64']} f32-f64 {out['steps.loss_f32'] - out['steps.loss_f64']}")
    np.savez_compressed(os.path.join(HERE, f"transducer_model_{name}.npz"), **out)


class TooManyCalls(RuntimeError):
    pass


class Rows:
    """Stands where the search's joint network is: keeps every call's log-probability row."""
    CAP = 4000  # a search that needs more joint calls than this is not a case

    def __init__(self, joint):
        self.joint, self.rows = joint, []

    def __call__(self, enc_out, dec_out):
        if len(self.rows) >= self.CAP:
            raise TooManyCalls()
        y = self.joint(enc_out, dec_out)
        self.rows.append(torch.log_softmax(y, dim=-1).detach().clone())
        return y


def run_reference_search(model, enc, beam, nbest):
    rec = Rows(model.joint_network)
    bs = BeamSearchTransducer(decoder=model.decoder, joint_network=rec, beam_size=beam, search_type="default",
                              score_norm=False, nbest=nbest)
    with torch.no_grad(), default_dtype(enc.dtype):
        hyps = bs(enc)
    return [(list(h.yseq), float(h.score)) for h in hyps], torch.stack(rec.rows)


def replay_margin(rows, beam, n_frames, vocab, nbest_want):
    """The smallest decision margin of a search, from its recorded rows (fp64), and a check that the host logic
    on those rows gives the recorded n-best."""
    margins = []
    if beam <= 1:
        for r in rows:
            s = r.sort(descending=True)[0]
            margins.append(float(s[0] - s[1]))
        return min(margins)
    it = iter(rows)
    kept = default_beam_search(lambda hyp, t, cache: (next(it), None), n_frames, None, beam, vocab, 0,
                               trace=lambda kind, m: margins.append(m))
    kept.sort(key=lambda x: x.score, reverse=True)
    got = [(list(h.yseq), float(h.score)) for h in kept[: len(nbest_want)]]
    assert [g[0] for g in got] == [w[0] for w in nbest_want], (got, nbest_want)
    # the final ranking is a decision too
    sc = sorted((float(h.score) for h in kept), reverse=True)
    margins += [a - b for a, b in zip(sc[: len(nbest_want)], sc[1: len(nbest_want) + 1])]
    return min(margins)


SEARCHES = (("greedy", 1, 1), ("beam2", 2, 3), ("beam5", 5, 3))


def search_fixture():
    out = {}
    cases = []
    models_done = 0
    for cname, seed in TH.SEARCH_MODELS:
        if models_done == 2:
            break
        mname = f"{cname}@{seed}"
        _, cfg, tc = TH.case_cfg(cname)
        pair = []
        for dt in (torch.float32, torch.float64):
            m = build_reference(cfg, tc).to(dt)
            load(m, TH.search_params(cfg, tc, seed, dt))
            m.eval()
            pair.append(m)
        m32, m64 = pair
        found = []
        for useed in range(700, 730):
            if len(found) == 2:
                break
            speech = TH.search_speech(cfg, useed)
            lengths = torch.tensor([speech.shape[0]])
            with torch.no_grad():
                enc = m64.encode(speech.double().unsqueeze(0), lengths)[0][0].float()  # the recorded encoder output
            rec, ok = {}, True
            for sname, beam, nbest in SEARCHES:
                try:
                    n32, r32 = run_reference_search(m32, enc, beam, nbest)
                    n64, r64 = run_reference_search(m64, enc.double(), beam, nbest)
                except TooManyCalls:
                    print(f"search {mname} utt {useed} {sname}: more than {Rows.CAP} joint calls -> retry", flush=True)
                    ok = False
                    break
                same = [a[0] for a in n32] == [b[0] for b in n64] and r32.shape == r64.shape
                if not same:
                    print(f"search {mname} utt {useed} {sname}: fp32 and fp64 n-best differ -> retry", flush=True)
                    ok = False
                    break
                dist = max(float((r32.double() - r64).abs().max()), max(abs(a[1] - b[1]) for a, b in zip(n32, n64)))
                margin = replay_margin(r64, beam, enc.shape[0], cfg.vocab_size, n64)
                nonempty = len(n64[0][0]) > 1
                good = margin >= MARGIN * dist and nonempty
                print(f"search {mname} utt {useed} {sname}: best {n64[0][0]} score {n64[0][1]:.4f} n-best {len(n64)} "
                      f"calls {len(r64)} margin {margin:.3e} dist {dist:.3e} -> {'ok' if good else 'retry'}", flush=True)
                if not good:
                    ok = False
                    break
                rec[sname] = (n32, n64, r32, r64, margin, dist)
            if ok:
                found.append((useed, enc, rec))
        if len(found) < 2:
            print(f"search {mname}: {len(found)} utterance(s) only, model dropped", flush=True)
            continue
        for i, (useed, enc, rec) in enumerate(found):
            case = f"{mname}.u{i}"
            cases.append(case)
            out[f"{case}/enc"] = enc.numpy()
            out[f"{case}/utt_seed"] = np.int64(useed)
            for sname, (n32, n64, r32, r64, margin, dist) in rec.items():
                pre = f"{case}/{sname}/"
                L = max(len(y) for y, _ in n64)
                ys = np.full((len(n64), L), -1, dtype=np.int64)
                for j, (y, _) in enumerate(n64):
                    ys[j, : len(y)] = y
                out[pre + "yseq"] = ys
                out[pre + "score_f64"] = np.array([sc for _, sc in n64])
                out[pre + "score_f32"] = np.array([sc for _, sc in n32])
                out[pre + "rows"] = r64.numpy().astype(np.float32)
                out[pre + "margin"], out[pre + "dist"] = np.float64(margin), np.float64(dist)
        models_done += 1
    assert models_done == 2, models_done
    out["cases"] = np.array(cases)
    out["searches"] = np.array([s[0] for s in SEARCHES])
    out["search_beam"] = np.array([s[1] for s in SEARCHES])
    out["search_nbest"] = np.array([s[2] for s in SEARCHES])
    np.savez_compressed(os.path.join(HERE, "transducer_search.npz"), **out)


def eval_fixture():
    """Eval-mode cer_transducer / wer_transducer (ErrorCalculatorTransducer: beam 2, `default`, every padded frame) of
    the decoding models on short batches.  A batch is kept only when the fp32 and fp64 runs make the same joint
    calls and report the same rates, and no decision of the fp64 searches is closer than 100 x the fp32 run's distance."""
    gs = dict(np.load(os.path.join(HERE, "transducer_search.npz"), allow_pickle=False))
    out, names = {}, sorted({c.split(".")[0] for c in gs["cases"].tolist()})
    # (equal lengths: the padded frames of a shorter utterance are identical rows, and the search on them is a run
    # of exact ties that rounding decides)
    lens, ulens = [TH.SEARCH_T] * 3, [3, 1, 2]
    for mname in names:
        cfg, tc, seed = TH.search_model_of(mname)
        runs = {}
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            m = build_reference(cfg, tc).to(dt)
            load(m, TH.search_params(cfg, tc, seed, dt))
            m.eval()
            runs[tag] = m
        for bseed in range(800, 860):
            speech, slen, text, tlen = TH.O.synthetic_batch(3, TH.SEARCH_T, cfg.enc.input_size, cfg.vocab_size, lens,
                                                            ulens, bseed)
            res = {}
            try:
                for tag, m in runs.items():
                    dt = torch.float32 if tag == "f32" else torch.float64
                    rows = Rows(m.joint_network)
                    m.error_calculator_trans.beam_search.joint_network = rows
                    with torch.no_grad(), default_dtype(dt):
                        _, es, _ = m(speech.to(dt), slen.clone(), text.clone(), tlen.clone())
                    res[tag] = (torch.stack(rows.rows), float(es["cer_transducer"]), float(es["wer_transducer"]),
                                float(es["loss"]))
            except TooManyCalls:
                continue
            (r32, c32, w32, l32), (r64, c64, w64, l64) = res["f32"], res["f64"]
            if r32.shape != r64.shape or (c32, w32) != (c64, w64):
                print(f"eval {mname} batch {bseed}: fp32 and fp64 searches differ -> retry", flush=True)
                continue
            margins, it = [], iter(r64)
            n_frames = int(TH.O.subsampled_lengths(torch.tensor(lens), TH.SEARCH_T).max())
            for _ in range(3):
                default_beam_search(lambda hyp, t, cache: (next(it), None), n_frames, None, 2, cfg.vocab_size, 0,
                                    trace=lambda kind, mg: margins.append(mg))
            assert next(it, None) is None
            margin, dist = min(margins), float((r32.double() - r64).abs().max())
            good = margin >= MARGIN * dist
            print(f"eval {mname} batch {bseed}: cer {c64:.4f} wer {w64:.4f} calls {len(r64)} margin {margin:.3e} dist "
                  f"{dist:.3e} -> {'ok' if good else 'retry'}", flush=True)
            if good:
                out.update({f"{mname}/batch_seed": np.int64(bseed), f"{mname}/cer_transducer": np.float64(c64),
                            f"{mname}/wer_transducer": np.float64(w64), f"{mname}/loss_f64": np.float64(l64),
                            f"{mname}/loss_f32": np.float64(l32), f"{mname}/margin": np.float64(margin),
                            f"{mname}/dist": np.float64(dist)})
                break
        else:
            raise RuntimeError(f"eval {mname}: no batch satisfies the margins")
    out["models"] = np.array(names)
    out["lens"], out["ulens"] = np.array(lens), np.array(ulens)
    np.savez_compressed(os.path.join(HERE, "transducer_eval.npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["meta", "model", "search", "eval"]
    if "meta" in which:
        meta_fixture()
    for name in TH.CASES:
        if "model" in which or f"model={name}" in which:
            model_fixture(name)
    if "search" in which:
        search_fixture()
    if "eval" in which:
        eval_fixture()
