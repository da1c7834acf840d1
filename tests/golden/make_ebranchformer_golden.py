"""Generate the E-Branchformer fixtures by running the REFERENCE implementation (the container that holds the
reference only; the fixtures are DATA and nothing of the reference travels with them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ebranchformer_golden.py

The fp64 truth is the reference model itself run in .double(), stored next to its fp32 run, as in
make_branchformer_golden.py (whose run / save_parts / scalars this follows).  Parameters come from
tests/branchformer_helpers.seeded_params, inputs from oracle.espnet_cpu.synthetic_batch.  A fixture is written as
NAME.npz plus NAME.partK.npz files, each below 1 MiB (branchformer_helpers.load_fixture merges them).
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

import espnet.nets.pytorch_backend.transformer.repeat as _rp  # noqa: E402
import espnet2.asr.encoder.e_branchformer_encoder as _ebf  # noqa: E402


def _repeat(N, fn, layer_drop_rate=0.0):
    """The fork's repeat has no layer_drop_rate argument (signature only; make_cbt_golden.py's adapter)."""
    assert layer_drop_rate == 0.0
    return _rp.repeat(N, fn)


_ebf.repeat = _repeat

from espnet2.asr.ctc import CTC  # noqa: E402
from espnet2.asr.decoder.transformer_decoder import TransformerDecoder  # noqa: E402
from espnet2.asr.espnet_model import ESPnetASRModel  # noqa: E402
from espnet2.layers.utterance_mvn import UtteranceMVN  # noqa: E402

from oracle import espnet_cpu as O  # noqa: E402
from tests import ebranchformer_helpers as EH  # noqa: E402

torch.set_num_threads(8)
LOSS_TOL = 1e-4  # the tests' loss tolerance
PART_BYTES = 900_000


def build_reference(conf):
    V = conf["token_list_size"]
    enc = _ebf.EBranchformerEncoder(input_size=conf["input_size"], **conf["encoder_conf"])
    dec = TransformerDecoder(vocab_size=V, encoder_output_size=enc.output_size(), **conf["decoder_conf"])
    ctc = CTC(odim=V, encoder_output_size=enc.output_size(), **conf["ctc_conf"])
    norm = UtteranceMVN(**conf["normalize_conf"]) if conf.get("normalize") == "utterance_mvn" else None
    return ESPnetASRModel(vocab_size=V, frontend=None, specaug=None, normalize=norm, preencoder=None, encoder=enc,
                          postencoder=None, decoder=dec, ctc=ctc, joint_network=None, token_list=EH.token_list(V),
                          **conf["model_conf"])


def run(conf, batch, seed, dtype):
    """One training-mode forward + backward of the reference in `dtype` -> (model, loss, stats)."""
    model = build_reference(conf).to(dtype)
    EH.load_seeded(model, seed)
    model.train()
    # the positional table the run feeds its blocks (the embed's positional-encoding module returns (x, pos_emb))
    model.encoder.embed.out[1].register_forward_hook(
        lambda m, i, o: setattr(model, "pos_emb_used", o[1][0].detach().float().numpy().copy()))
    speech, slen, text, tlen = batch
    loss, stats, _ = model(speech.to(dtype).clone(), slen.clone(), text.clone(), tlen.clone())
    loss.backward()
    return model, loss, stats


def masked_merge_loss(conf, batch, seed):
    """The fp64 loss of a variant that zeroes each utterance's padded frames before depthwise_conv_fusion (a masked
    / per-utterance zero-padded merge convolution).  The reference does not do this; a fixture whose loss this
    variant also matches could not tell the two apart."""
    model = build_reference(conf).double()
    EH.load_seeded(model, seed)
    model.train()
    speech, slen, text, tlen = batch
    olens = model.encoder(speech.double(), slen)[1]

    def mask_input(mod, args):  # (B, 2D, T')
        x = args[0]
        keep = (torch.arange(x.shape[2])[None, :] < olens[:, None]).to(x.dtype)[:, None, :]
        return (x * keep,)

    hooks = [layer.depthwise_conv_fusion.register_forward_pre_hook(mask_input) for layer in model.encoder.encoders]
    try:
        loss, _, _ = model(speech.double().clone(), slen.clone(), text.clone(), tlen.clone())
    finally:
        for h in hooks:
            h.remove()
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


def fixture(name, conf, B, T, lens, ulens, seed):
    batch = O.synthetic_batch(B, T, conf["input_size"], conf["token_list_size"], lens, ulens, seed + 1)
    m32, l32, s32 = run(conf, batch, seed, torch.float32)
    m64, l64, s64 = run(conf, batch, seed, torch.float64)
    speech, slen, text, tlen = batch
    out = dict(speech=speech.numpy().copy(), speech_lengths=slen.numpy().copy(), text=text.numpy().copy(),
               text_lengths=tlen.numpy().copy(), seed=np.int64(seed))
    scalars(out, l32, s32, "f32")
    scalars(out, l64, s64, "f64")
    lm = masked_merge_loss(conf, batch, seed)
    out["loss_masked_merge_f64"] = np.float64(lm)
    print(f"{name}: loss f32 {l32.item():.6f} f64 {l64.item():.6f} |d|={abs(l32.item() - l64.item()):.2e}; "
          f"masked-merge variant {lm:.6f} (differs by {abs(lm - l64.item()):.3e})")
    # a masked merge convolution must not satisfy the fixture: pick another seed or other lengths if this fails
    assert abs(lm - l64.item()) > 10 * LOSS_TOL, (lm, l64.item())
    sd = m32.encoder.state_dict()
    out["enc_sd_keys"] = np.array(sorted(sd.keys()))
    shp = np.zeros((len(sd), 4), dtype=np.int64)
    for i, k in enumerate(sorted(sd.keys())):
        shp[i, :sd[k].dim()] = list(sd[k].shape)
    out["enc_sd_shapes"] = shp
    out["pos_emb"] = m32.pos_emb_used  # (see make_branchformer_golden.py: hosts differ in the table's last bit)
    out["num_params"] = np.int64(sum(p.numel() for p in m32.parameters()))
    for (n, p32), (_, p64) in zip(m32.named_parameters(), m64.named_parameters()):
        out["grad/" + n] = p32.grad.numpy()
        out["grad64/" + n] = p64.grad.numpy()
        out["gn_f32/" + n] = np.float64(p32.grad.double().norm().item())
        out["gn_f64/" + n] = np.float64(p64.grad.norm().item())
    m32.eval()
    with torch.no_grad():
        eo, el = m32.encode(speech.clone(), slen.clone())  # (UtteranceMVN normalises in place)
    out["enc_out"] = eo.numpy()
    out["enc_olens"] = el.numpy().astype(np.int64)
    save_parts(name, out)


if __name__ == "__main__":
    for name in sys.argv[1:] or EH.FIXTURES:
        fixture(name, *EH.FIXTURES[name])
