"""Generate the Branchformer fixtures by running the REFERENCE implementation (the container that holds the
reference only; the fixtures are DATA and nothing of the reference travels with them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_branchformer_golden.py

The oracle restatement has no Branchformer, so the fp64 truth is the reference model itself run in .double(),
stored next to its fp32 run.  Parameters come from tests/branchformer_helpers.seeded_params (not from the
reference's initialisation, whose 1e-6 gate-convolution weights hide the convolution path), inputs from
oracle.espnet_cpu.synthetic_batch.  A fixture is written as NAME.npz plus NAME.partK.npz files, each below
1 MiB (branchformer_helpers.load_fixture merges them).
"""
import json
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
from espnet2.asr.decoder.transformer_decoder import TransformerDecoder  # noqa: E402
from espnet2.asr.encoder.branchformer_encoder import BranchformerEncoder  # noqa: E402
from espnet2.asr.espnet_model import ESPnetASRModel  # noqa: E402
from espnet2.asr.layers.cgmlp import ConvolutionalSpatialGatingUnit  # noqa: E402
from espnet2.layers.utterance_mvn import UtteranceMVN  # noqa: E402

from oracle import espnet_cpu as O  # noqa: E402
from tests import branchformer_helpers as BH  # noqa: E402

torch.set_num_threads(8)
RECIPE_YAML = "egs2/slurp_entity/asr1/conf/tuning/train_asr_branchformer_e18_d6_size512_lr1e-3_warmup35k.yaml"
LOSS_TOL = 1e-4  # the tests' loss tolerance
PART_BYTES = 900_000


def build_reference(conf):
    V = conf["token_list_size"]
    enc = BranchformerEncoder(input_size=conf["input_size"], **conf["encoder_conf"])
    dec = TransformerDecoder(vocab_size=V, encoder_output_size=enc.output_size(), **conf["decoder_conf"])
    ctc = CTC(odim=V, encoder_output_size=enc.output_size(), **conf["ctc_conf"])
    norm = UtteranceMVN(**conf["normalize_conf"]) if conf.get("normalize") == "utterance_mvn" else None
    return ESPnetASRModel(vocab_size=V, frontend=None, specaug=None, normalize=norm, preencoder=None, encoder=enc,
                          postencoder=None, decoder=dec, ctc=ctc, joint_network=None, token_list=BH.token_list(V),
                          **conf["model_conf"])


def run(conf, batch, seed, dtype):
    """One training-mode forward + backward of the reference in `dtype` -> (model, loss, stats)."""
    model = build_reference(conf).to(dtype)
    BH.load_seeded(model, seed)
    model.train()
    # the positional table the run feeds its blocks (the embed's positional-encoding module returns (x, pos_emb))
    model.encoder.embed.out[1].register_forward_hook(
        lambda m, i, o: setattr(model, "pos_emb_used", o[1][0].detach().float().numpy().copy()))
    speech, slen, text, tlen = batch
    loss, stats, _ = model(speech.to(dtype).clone(), slen.clone(), text.clone(), tlen.clone())
    loss.backward()
    return model, loss, stats


def masked_conv_loss(conf, batch, seed):
    """The fp64 loss of a variant that zeroes each utterance's padded frames before the gate's depthwise
    convolution (a masked / per-utterance zero-padded convolution).  The reference does not do this; a fixture
    whose loss this variant also matches could not tell the two apart."""
    model = build_reference(conf).double()
    BH.load_seeded(model, seed)
    model.train()
    speech, slen, text, tlen = batch
    olens = model.encoder(speech.double(), slen)[1]
    orig = ConvolutionalSpatialGatingUnit.forward

    def forward(self, x, gate_add=None):
        x_r, x_g = x.chunk(2, dim=-1)
        x_g = self.norm(x_g)
        keep = (torch.arange(x_g.shape[1])[None, :] < olens[:, None]).to(x_g.dtype)[:, :, None]
        x_g = self.conv((x_g * keep).transpose(1, 2)).transpose(1, 2)
        return self.dropout(x_r * self.act(x_g))

    ConvolutionalSpatialGatingUnit.forward = forward
    try:
        loss, _, _ = model(speech.double().clone(), slen.clone(), text.clone(), tlen.clone())
    finally:
        ConvolutionalSpatialGatingUnit.forward = orig
    return float(loss.item())


def save_parts(name, out):
    """NAME.npz holds the small entries; the gradient tensors are packed into NAME.partK.npz files of at
    most PART_BYTES raw bytes each (no committed file above 1 MiB)."""
    for f in os.listdir(HERE):
        if f.startswith(name + ".part") and f.endswith(".npz"):
            os.remove(os.path.join(HERE, f))
    head = {k: v for k, v in out.items() if not k.startswith(("grad/", "grad64/"))}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **head)
    part, size, idx = {}, 0, 0
    for k, v in out.items():
        if k in head:
            continue
        if part and size + v.nbytes > PART_BYTES:
            np.savez_compressed(os.path.join(HERE, f"{name}.part{idx}.npz"), **part)
            part, size, idx = {}, 0, idx + 1
        part[k] = v
        size += v.nbytes
    if part:
        np.savez_compressed(os.path.join(HERE, f"{name}.part{idx}.npz"), **part)
    for f in sorted(os.listdir(HERE)):
        if f.startswith(name + "."):
            n = os.path.getsize(os.path.join(HERE, f))
            assert n < (1 << 20), (f, n)
            print(f"  {f}: {n} bytes")


def scalars(out, loss, stats, tag):
    out["loss_" + tag] = np.float64(loss.item())
    out["loss_ctc_" + tag] = np.float64(stats["loss_ctc"].item())
    out["loss_att_" + tag] = np.float64(stats["loss_att"].item())
    out["acc_" + tag] = np.float64(float(stats["acc"]))


def fixture(name, conf, B, T, lens, ulens, seed, full):
    batch = O.synthetic_batch(B, T, conf["input_size"], conf["token_list_size"], lens, ulens, seed + 1)
    m32, l32, s32 = run(conf, batch, seed, torch.float32)
    m64, l64, s64 = run(conf, batch, seed, torch.float64)
    speech, slen, text, tlen = batch
    # (copies: numpy views of the batch would follow any later in-place change of it)
    out = dict(speech=speech.numpy().copy(), speech_lengths=slen.numpy().copy(), text=text.numpy().copy(),
               text_lengths=tlen.numpy().copy(), seed=np.int64(seed))
    scalars(out, l32, s32, "f32")
    scalars(out, l64, s64, "f64")
    lm = masked_conv_loss(conf, batch, seed)
    out["loss_masked_conv_f64"] = np.float64(lm)
    print(f"{name}: loss f32 {l32.item():.6f} f64 {l64.item():.6f} |d|={abs(l32.item() - l64.item()):.2e}; "
          f"masked-convolution variant {lm:.6f} (differs by {abs(lm - l64.item()):.3e})")
    # a masked convolution must not satisfy the fixture: pick other lengths if this fails
    assert abs(lm - l64.item()) > 10 * LOSS_TOL, (lm, l64.item())
    sd = m32.encoder.state_dict()
    out["enc_sd_keys"] = np.array(list(sd.keys()))
    shp = np.zeros((len(sd), 4), dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shp[i, :v.dim()] = list(v.shape)
    out["enc_sd_shapes"] = shp
    # The table is sin / cos of position * exp(-2i ln(1e4) / d) in fp32: the last bit of the host's fp32 exp is
    # amplified by the position (up to 5000 in the legacy table: 1 ulp moves an entry by 1e-4), and hosts differ in
    # it.  The table this run used is recorded so that a test can give the model under test the same constant.
    out["pos_emb"] = m32.pos_emb_used
    out["num_params"] = np.int64(sum(p.numel() for p in m32.parameters()))
    for (n, p32), (_, p64) in zip(m32.named_parameters(), m64.named_parameters()):
        if full:
            out["grad/" + n] = p32.grad.numpy()
            out["grad64/" + n] = p64.grad.numpy()
        out["gn_f32/" + n] = np.float64(p32.grad.double().norm().item())
        out["gn_f64/" + n] = np.float64(p64.grad.norm().item())
    if full:
        m32.eval()
        with torch.no_grad():
            eo, el = m32.encode(speech.clone(), slen.clone())  # (UtteranceMVN normalises in place)
        out["enc_out"] = eo.numpy()
        out["enc_olens"] = el.numpy().astype(np.int64)
    save_parts(name, out)


def recipe_config():
    """The recipe's training config as the reference resolves it: egs2/slurp_entity/asr1/run.sh trains with
    --feats_type raw (the default frontend's 80-dim log-mel fbank) and --feats_normalize utterance_mvn."""
    import yaml
    with open(os.path.join(refshim.REF, RECIPE_YAML)) as f:
        conf = yaml.safe_load(f)
    keys = ("encoder", "encoder_conf", "decoder", "decoder_conf", "model_conf", "specaug", "specaug_conf", "optim",
            "optim_conf", "scheduler", "scheduler_conf", "batch_type", "batch_size", "accum_grad", "max_epoch",
            "best_model_criterion", "keep_nbest_models")
    resolved = {k: conf[k] for k in keys if k in conf}
    resolved["model_conf"] = {k: v for k, v in resolved["model_conf"].items() if k != "extract_feats_in_collect_stats"}
    resolved.update(input_size=80, normalize="utterance_mvn", normalize_conf={}, ctc_conf={}, frontend=None,
                    token_list_size=600,
                    source=RECIPE_YAML + " + egs2/slurp_entity/asr1/run.sh (raw -> 80-dim fbank, utterance_mvn); "
                    "token_list_size is the fixtures' (the recipe's word vocabulary comes from its data)")
    return resolved


def recipe_fixture():
    conf = recipe_config()
    ref = build_reference(conf)
    conf["reference_state_dict"] = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    conf["reference_num_params"] = int(sum(p.numel() for p in ref.parameters()))
    del ref
    with open(os.path.join(HERE, "branchformer_slurp_entity.json"), "w") as f:
        json.dump(conf, f, indent=1)
    print("recipe config:", conf["reference_num_params"], "parameters at V =", conf["token_list_size"])
    r = BH.RECIPE_B2
    fixture(r["name"], BH.recipe_b2_conf(conf), r["B"], r["T"], r["lens"], r["ulens"], r["seed"], full=False)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "recipe"]
    if "small" in which:
        for name, (conf, B, T, lens, ulens, seed) in BH.SMALL_FIXTURES.items():
            fixture(name, conf, B, T, lens, ulens, seed, full=name != "branchformer_cgmlp_only")
    if "recipe" in which:
        recipe_fixture()
