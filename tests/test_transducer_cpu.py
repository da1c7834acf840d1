"""The RNN-Transducer without a GPU: the registry, the state_dict keys, what raises by name, the host side of prepare,
the lattice of tests/rnnt_helpers.py against a brute-force sum over alignments and against the losses recorded from the
reference, and the host logic of default_beam_search on recorded log-probability rows (tests/golden/transducer_*.npz,
written by make_transducer_golden.py)."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import transducer_helpers as TH
from tests.helpers import golden, token_list
from tests.rnnt_helpers import brute_force_nll, lattice, rnnt_nll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esp_rnnt_joint_fwd", "esp_rnnt_joint_bwd", "esp_rnnt_logprobs", "esp_rnnt_alpha_beta", "esp_rnnt_grad",
       "esp_lstm_cell_fwd", "esp_lstm_cell_bwd")


def test_registry_resolves_the_transducer_decoder():
    from espnet_slurp_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_slurp_amd.tasks import asr
    assert asr.decoder_choices.get_class("transducer") is TransducerDecoder
    assert "transducer" in asr.decoder_choices.choices()


def test_header_and_signature_table_have_the_entry_points():
    from espnet_slurp_amd import _native
    with open(os.path.join(ROOT, "include", "espnet_mi355.h"), encoding="utf-8") as f:
        h = f.read()
    for name in NEW + ("esp_rnnt_loss_workspace_bytes", "esp_rnnt_joint_bwd_workspace_bytes"):
        m = re.search(r"\b(int|long) " + name + r"\([^;]*\);", h)
        assert m, name
        proto = m.group(0)
        args = [a for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",") if a.strip()]
        assert name in _native.SIGNATURES and len(args) == len(_native.SIGNATURES[name]), name
    assert _native.workspace_bytes("esp_rnnt_loss", 2, 3, 4) == 5 * 8 * 2 * 3 * 4
    assert _native.workspace_bytes("esp_rnnt_joint_bwd", 2, 33, 4, 5) == 4 * 2 * 3 * 4 * 5  # 3 tiles of 16 frames


def _build(name, **kw):
    seed, cfg, tc = TH.case_cfg(name)
    model = TH.build_transducer(cfg, tc, "cpu", **kw)
    return seed, cfg, tc, model


def test_state_dict_keys_and_shapes_are_the_reference_s():
    g = golden("transducer_meta")
    for name, tag in (("tf_l1", "noctc"), ("tf_l2_ctc", "ctc")):
        seed, cfg, tc, model = _build(name)
        sd = model.state_dict()
        assert list(sd) == g[f"{tag}.keys"].tolist()
        for k, shp in zip(g[f"{tag}.keys"].tolist(), g[f"{tag}.shapes"]):
            assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v >= 0), k
        TH.load_params(model, TH.transducer_params(cfg, tc, seed))
        # the reference's quirk: the CTC error calculator exists only when both report flags are off
        assert model.error_calculator is None and model.error_calculator_trans is not None
        quiet = _build(name, report=False)[3]
        assert (quiet.error_calculator is not None) == bool(g[f"{tag}.noreport.has_error_calculator"])
        assert (quiet.error_calculator_trans is not None) == bool(g[f"{tag}.noreport.has_error_calculator_trans"])
        # flatten() attached the joint network's parameters too
        ids = {id(p) for _, p in model.flat.params}
        assert all(id(p) in ids for p in model.joint_network.parameters())
        assert all(id(p) in ids for p in model.decoder.parameters())


def test_what_is_not_served_raises_by_name():
    from espnet_slurp_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_slurp_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from espnet_slurp_amd.asr.transducer.joint_network import JointNetwork
    with pytest.raises(NotImplementedError, match="gru"):
        TransducerDecoder(TH.V, rnn_type="gru")
    with pytest.raises(NotImplementedError, match="swish"):
        JointNetwork(TH.V, TH.D, TH.H, joint_activation_type="swish")
    dec, joint = TransducerDecoder(TH.V, hidden_size=8), JointNetwork(TH.V, TH.D, 8, joint_space_size=8)
    for st in ("tsd", "alsd", "nsc", "maes"):
        with pytest.raises(NotImplementedError, match=st):
            BeamSearchTransducer(dec, joint, 2, search_type=st)
    with pytest.raises(NotImplementedError, match="lm"):
        BeamSearchTransducer(dec, joint, 2, lm=torch.nn.Linear(1, 1))
    assert BeamSearchTransducer(dec, joint, 1, search_type="maes").search_algorithm.__name__ == "greedy_search"
    # interctc / self-conditioning with a transducer
    seed, cfg, tc = TH.case_cfg("cf_l1_ctc")
    from espnet_slurp_amd.asr.ctc import CTC
    from espnet_slurp_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_slurp_amd.asr.espnet_model import ESPnetASRModel

    def model(interctc_weight, cond):
        enc = ConformerEncoder(input_size=80, output_size=TH.D, attention_heads=4, linear_units=128, num_blocks=2,
                               interctc_layer_idx=[1], interctc_use_conditioning=cond)
        return ESPnetASRModel(vocab_size=TH.V, token_list=token_list(TH.V), frontend=None, specaug=None, normalize=None,
                              preencoder=None, encoder=enc, postencoder=None, decoder=dec,
                              ctc=CTC(odim=TH.V, encoder_output_size=TH.D), joint_network=joint, ctc_weight=0.3,
                              interctc_weight=interctc_weight)
    with pytest.raises(NotImplementedError, match="interctc_weight"):
        model(0.3, False)
    with pytest.raises(NotImplementedError, match="interctc_use_conditioning"):
        model(0.0, True)


def test_speech2text_refuses_the_other_searches_with_a_transducer():
    from espnet_slurp_amd.bin.asr_inference import Speech2Text
    model = _build("tf_l1")[3]
    for kw, word in ((dict(batch_search=True), "batch_search"), (dict(streaming=True), "streaming"),
                     (dict(lm=torch.nn.Linear(1, 1)), "lm")):
        with pytest.raises(ValueError, match=word):
            Speech2Text(model, **kw)
    s2t = Speech2Text(model, beam_size=2, transducer_conf=dict(score_norm=False, nbest=3))
    assert s2t.beam_search_transducer.nbest == 3 and s2t.beam_search_transducer.score_norm is False
    with pytest.raises(ValueError, match="decode_batch"):
        s2t.decode_batch([torch.zeros(20, 80)])


def test_build_model_constructs_decoder_and_joint_network_as_the_reference():
    from espnet_slurp_amd.tasks.asr import build_model
    args = argparse.Namespace(
        token_list=token_list(TH.V), input_size=80, specaug=None, specaug_conf={}, normalize="utterance_mvn",
        normalize_conf={}, encoder="transformer",
        encoder_conf=dict(output_size=TH.D, attention_heads=4, linear_units=128, num_blocks=1, input_layer="conv2d"),
        decoder="transducer", decoder_conf=dict(rnn_type="lstm", num_layers=1, hidden_size=24, dropout=0.1,
                                                dropout_embed=0.2),
        joint_net_conf=dict(joint_space_size=20), ctc_conf={}, model="espnet", model_conf=dict(ctc_weight=0.3), init=None)
    m = build_model(args, device="cpu")
    assert m.use_transducer_decoder and m.decoder.dunits == 24 and m.decoder.blank_id == 0
    assert m.joint_network.lin_enc.weight.shape == (20, TH.D) and m.joint_network.lin_dec.weight.shape == (20, 24)
    assert m.joint_network.lin_out.weight.shape == (TH.V, 20) and m.joint_network.lin_dec.bias is None
    assert m.decoder.dropout == 0.1 and m.decoder.dropout_embed == 0.2 and m.ctc is not None


def test_prepare_reproduces_get_transducer_task_io():
    g = golden("transducer_meta")
    model = _build("tf_l2_ctc")[3]
    text = torch.from_numpy(g["io_text"])
    tl = (text != -1).sum(1)
    sl = torch.tensor([60, 47, 33])
    prep = model.prepare(sl, text, tl, 60, 80)
    h = prep.host
    assert h["dec_in"].tolist() == g["io_decoder_in"].tolist()
    assert h["rnnt_target"].tolist() == g["io_target"].tolist()
    assert h["rnnt_ulens"].tolist() == g["io_u_len"].tolist() and h["rnnt_ulens"].dtype == torch.int32
    t_len = TH.O.subsampled_lengths(sl, 60).tolist()  # t_len is the encoder's output lengths
    assert h["hlens"].tolist() == t_len == [14, 12, 9] and prep.U1 == 6 and prep.Umax == 5
    assert h["ys"].tolist() == g["io_text"].tolist()  # the CTC branch keeps the -1 padding
    assert (h["dec_in_grad"] == -1).tolist() == (h["dec_in"] == 0).tolist()
    # u_bucket pads every target-side tensor with blank / -1, the lengths stay
    b = model.prepare(sl, text, tl, 60, 80, t_bucket=64, u_bucket=8)
    assert b.U1 == 9 and b.host["dec_in"].shape == (3, 9) and b.host["rnnt_target"].shape == (3, 8)
    assert b.host["dec_in"][:, :6].tolist() == g["io_decoder_in"].tolist() and (b.host["dec_in"][:, 6:] == 0).all()
    assert (b.host["rnnt_target"][:, 5:] == 0).all() and (b.host["ys"][:, 5:] == -1).all()
    assert b.host["rnnt_ulens"].tolist() == g["io_u_len"].tolist() and b.host["hlens"].tolist() == t_len


@pytest.mark.parametrize("T,U", [(3, 2), (2, 3), (1, 0), (1, 2), (4, 0)])
def test_lattice_equals_the_sum_over_all_alignments(T, U):
    g = torch.Generator().manual_seed(10 * T + U)
    V = 5
    logits = torch.randn(1, T, U + 1, V, generator=g, dtype=torch.float64) * 3
    y = torch.randint(1, V, (1, max(U, 1)), generator=g)[:, :U]
    lp = torch.log_softmax(logits[0], -1)
    want = brute_force_nll(lp, y[0].tolist())
    got = rnnt_nll(logits, y, [T], [U])[0]
    al, be = lattice(lp, y[0].tolist())
    assert abs(float(got - want)) < 1e-12 and abs(float(be[0, 0] + want)) < 1e-12
    # alpha + beta is the same total on every anti-diagonal's cut: sum over the cells of a diagonal
    tot = torch.logsumexp(torch.stack([al[t, d - t] + be[t, d - t] for d in [min(1, T + U - 1)]
                                       for t in range(T) if 0 <= d - t <= U]), 0)
    assert abs(float(tot + want)) < 1e-12


def test_lattice_equals_the_reference_s_recorded_losses():
    for name in TH.CASES:
        g = golden(f"transducer_model_{name}")
        loss, stats, G = TH.restated_grads(name)
        assert abs(float(loss) - float(g["loss_f64"])) < 1e-10, name
        assert abs(float(stats["loss_transducer"]) - float(g["loss_transducer_f64"])) < 1e-10, name
        assert abs(float(g["loss_f32"]) - float(g["loss_f64"])) < 1e-4
        scale = max(float(g["gmax_f64/" + n]) for n in G)  # (a key bias has no gradient at all: fp64 noise there)
        for n, gr in G.items():
            assert abs(float(gr.abs().max()) - float(g["gmax_f64/" + n])) <= 1e-9 * scale, n
        if "loss_ctc_f64" in g:
            assert abs(float(stats["loss_ctc"]) - float(g["loss_ctc_f64"])) < 1e-10
            assert g["stat_keys"].tolist() == ["loss_ctc", "cer_ctc", "loss_transducer", "cer_transducer",
                                               "wer_transducer", "loss"]
        else:
            assert g["stat_keys"].tolist() == ["loss_transducer", "cer_transducer", "wer_transducer", "loss"]


def test_default_beam_search_host_logic_on_recorded_rows():
    from espnet_slurp_amd.asr.transducer.beam_search_transducer import default_beam_search
    g = golden("transducer_search")
    cases = g["cases"].tolist()
    assert len(cases) >= 4
    for case in cases:
        n_frames = g[f"{case}/enc"].shape[0]
        for sname, beam, nbest in zip(g["searches"].tolist(), g["search_beam"].tolist(), g["search_nbest"].tolist()):
            pre = f"{case}/{sname}/"
            assert float(g[pre + "margin"]) >= 100.0 * float(g[pre + "dist"]) and g[pre + "yseq"][0, 1] >= 0
            rows = torch.from_numpy(g[pre + "rows"])
            want = [[int(t) for t in r if t >= 0] for r in g[pre + "yseq"]]
            if beam <= 1:  # greedy on the rows: a label moves on to the next recorded row of the same frame count
                y, score = [0], 0.0
                assert rows.shape[0] == n_frames
                for r in rows:
                    lp, k = torch.max(r, -1)
                    if int(k) != 0:
                        y.append(int(k))
                        score += float(lp)
                assert [y] == want and abs(score - float(g[pre + "score_f64"][0])) < 1e-4
                continue
            it = iter(rows)
            kept = default_beam_search(lambda hyp, t, cache: (next(it), None), n_frames, None, beam, TH.V, 0)
            assert next(it, None) is None  # every recorded call was made, in order
            kept.sort(key=lambda x: x.score, reverse=True)
            assert [h.yseq for h in kept[:nbest]] == want, (case, sname)
            for h, s in zip(kept[:nbest], g[pre + "score_f64"]):
                assert abs(h.score - float(s)) < 1e-4
