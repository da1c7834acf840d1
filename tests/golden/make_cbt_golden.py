"""Generate the contextual block Transformer fixtures by running the REFERENCE implementation (the container that
holds the reference only; the fixtures are DATA and nothing of the reference travels with them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cbt_golden.py [layout] [keys] [enc | cbt_enc_NAME] [s42] [model]

The reference's encoder does not import as shipped; beside refshim.install() it needs three signature-only
adapters, all here:
  * StreamPositionalEncoding is absent from the fork's embedding.py: a subclass of its PositionalEncoding whose
    forward(x, start_idx=0) asserts start_idx == 0 (forward_train never passes one);
  * the encoder calls its layers with the newer argument order (x, mask, infer_mode, past_ctx, next_ctx,
    is_short_segment, layer_idx, cache) and expects 7 values back, the fork's layer takes (x, mask, past_ctx,
    next_ctx, layer_idx, cache) and returns 5: a subclass that reorders and repacks, bound in the ENCODER module's
    namespace only (rebinding the name in the layer's own module would make its super() call recurse);
  * repeat without layer_drop_rate (refshim's S3).
The fp64 truth is the reference itself run in .double(), stored beside its fp32 run (as float32: the rounding, 6e-8
relative, is three orders below the tests' gates).  Parameters come from branchformer_helpers.seeded_params, all
dropouts are 0.
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

import espnet.nets.pytorch_backend.transformer.embedding as _emb  # noqa: E402
import espnet.nets.pytorch_backend.transformer.repeat as _rp  # noqa: E402


class StreamPositionalEncoding(_emb.PositionalEncoding):
    def forward(self, x, start_idx=0):
        assert start_idx == 0
        return super().forward(x)


_emb.StreamPositionalEncoding = StreamPositionalEncoding

import espnet2.asr.encoder.contextual_block_transformer_encoder as _cbe  # noqa: E402
from espnet.nets.pytorch_backend.transformer.contextual_block_encoder_layer import (  # noqa: E402
    ContextualBlockEncoderLayer as _Layer)


class LayerAdapter(_Layer):
    def forward(self, x, mask, infer_mode=False, past_ctx=None, next_ctx=None, is_short_segment=False, layer_idx=0,
                cache=None):
        assert not infer_mode and cache is None
        x, mask, next_ctx, next_ctx2, layer_idx = super().forward(x, mask, past_ctx, next_ctx, layer_idx, cache)
        return x, mask, infer_mode, next_ctx, next_ctx2, is_short_segment, layer_idx


def _repeat(N, fn, layer_drop_rate=0.0):
    assert layer_drop_rate == 0.0
    return _rp.repeat(N, fn)


_cbe.ContextualBlockEncoderLayer = LayerAdapter
_cbe.repeat = _repeat
RefEncoder = _cbe.ContextualBlockTransformerEncoder

from espnet2.asr.ctc import CTC  # noqa: E402
from espnet2.asr.decoder.transformer_decoder import TransformerDecoder  # noqa: E402
from espnet2.asr.espnet_model import ESPnetASRModel  # noqa: E402
from espnet2.layers.utterance_mvn import UtteranceMVN  # noqa: E402

from oracle import espnet_cpu as O  # noqa: E402
from tests import branchformer_helpers as BH  # noqa: E402
from tests import cbt_helpers as CH  # noqa: E402

torch.set_num_threads(8)
RECIPE_YAML = "egs2/slurp/asr1/conf/train_asr_streaming_transformer.yaml"


# ------------------------------------------------------------------------------------------------ layout maps
class _Recorder(torch.nn.Module):
    """Stands in for the layer stack: keeps the chunked input and the mask, returns a tensor coded by (block, slot)."""

    def forward(self, xs_chunk, mask, infer_mode, past_ctx, *rest):
        self.chunk, self.mask = xs_chunk.detach().clone(), mask.detach().clone()
        assert past_ctx is xs_chunk and not infer_mode
        out = torch.zeros_like(xs_chunk)
        out[..., 0] = torch.arange(xs_chunk.shape[1], dtype=out.dtype)[None, :, None]
        out[..., 1] = torch.arange(xs_chunk.shape[2], dtype=out.dtype)[None, None, :]
        return out, mask, None, None, None, None, None


class _Identity(torch.nn.Module):
    def forward(self, x, *a):
        return x


def record_layout(T, bs, hop, la):
    """The reference's forward_train with input_layer=None on one-hot coded frames (x[0, t] = e_t, in fp64), the
    positional step and after_norm replaced by the identity and the layer stack by the recorder."""
    D = T + T % 2  # (the positional table needs an even width)
    enc = RefEncoder(input_size=D, output_size=D, attention_heads=1, linear_units=4, num_blocks=1, dropout_rate=0.0,
                     positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer=None, block_size=bs,
                     hop_size=hop, look_ahead=la).double()
    enc.pos_enc, enc.after_norm, enc.encoders = _Identity(), _Identity(), _Recorder()
    enc.eval()
    with torch.no_grad():
        ys, olens, _ = enc.forward_train(torch.eye(T, D, dtype=torch.float64)[None], torch.tensor([T]))
    chunk, mask = enc.encoders.chunk[0], enc.encoders.mask[0]
    nblk, S, _ = chunk.shape
    assert S == bs + 2 and int(olens[0]) == T
    # fact 1: one mask for every block, queries 1..bs+1 see keys 0..bs
    want = torch.zeros(S, S, dtype=mask.dtype)
    want[1:, :bs + 1] = 1
    assert all(torch.equal(mask[k], want) for k in range(nblk))
    windows = []
    for k in range(nblk):  # the context slot is the window's indicator over its length
        v = chunk[k, S - 1]
        idx = torch.nonzero(v).flatten()
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        assert len(idx) == hi - lo and torch.allclose(v[lo:hi], torch.full((hi - lo,), 1.0 / (hi - lo), dtype=v.dtype))
        windows.append([lo, hi])
    src = []
    for k in range(nblk):
        row = []
        for s in range(S):
            v = chunk[k, s]
            if not bool(v.any()):
                row.append(-1)
            elif s in (0, S - 1):
                m = [j for j in range(nblk) if torch.equal(v, chunk[j, S - 1])]
                assert len(m) == 1
                row.append(-2 - m[0])
            else:
                idx = torch.nonzero(v).flatten()
                assert len(idx) == 1 and float(v[idx[0]]) == 1.0
                row.append(int(idx[0]))
        src.append(row)
    out = [[int(ys[0, t, 0]), int(ys[0, t, 1])] for t in range(T)]
    return dict(nblk=nblk, chunk_source=src, ctx_window=windows, output_source=out)


def layout_fixture():
    maps = {}
    for key, (bs, hop, la, Ts) in CH.LAYOUT_CASES.items():
        maps[key] = {str(T): record_layout(T, bs, hop, la) for T in Ts}
        print("layout", key, {T: m["nblk"] for T, m in maps[key].items()})
    with open(os.path.join(HERE, "cbt_layout.json"), "w") as f:
        json.dump(maps, f, separators=(",", ":"))


# ------------------------------------------------------------------------------------------------ state_dict keys
def recipe_config():
    import yaml
    with open(os.path.join(refshim.REF, RECIPE_YAML)) as f:
        conf = yaml.safe_load(f)
    keys = ("encoder", "encoder_conf", "decoder", "decoder_conf", "model_conf", "specaug", "specaug_conf", "optim",
            "optim_conf", "scheduler", "scheduler_conf", "batch_type", "batch_size", "max_epoch")
    resolved = {k: conf[k] for k in keys if k in conf}
    resolved["model_conf"] = {k: v for k, v in resolved["model_conf"].items() if k != "extract_feats_in_collect_stats"}
    resolved.update(input_size=80, normalize="utterance_mvn", normalize_conf={}, ctc_conf={}, frontend=None,
                    token_list_size=600,
                    source=RECIPE_YAML + " + egs2/slurp/asr1/run.sh (raw -> 80-dim fbank, utterance_mvn); "
                    "token_list_size is the fixtures' (the recipe's vocabulary comes from its data)")
    return resolved


def keys_fixture():
    conf = recipe_config()
    with torch.device("meta"):
        big = RefEncoder(input_size=80, **conf["encoder_conf"])
    small = RefEncoder(input_size=CH.INPUT_SIZE, **CH.encoder_conf())
    conf["reference_encoder_state_dict"] = [[k, list(v.shape)] for k, v in big.state_dict().items()]
    conf["small_encoder_state_dict"] = [[k, list(v.shape)] for k, v in small.state_dict().items()]
    print("keys:", len(conf["small_encoder_state_dict"]), "small,", len(conf["reference_encoder_state_dict"]), "recipe")
    with open(os.path.join(HERE, "cbt_slurp_streaming.json"), "w") as f:
        json.dump(conf, f, indent=1)


# ------------------------------------------------------------------------------------------------ encoder runs
def run_encoder(conf, feats, lens, cot, seed, dtype, input_size=CH.INPUT_SIZE):
    enc = RefEncoder(input_size=input_size, **conf).to(dtype)
    BH.load_seeded(enc, seed)
    enc.train()
    keep = {}

    def hook(mod, inp, outp):  # the gradient that reaches the embed output (B, T', D)
        outp[0].retain_grad()
        keep["embed"] = outp[0]

    enc.embed.register_forward_hook(hook)
    x = feats.to(dtype).clone().requires_grad_(True)
    out, olens, _ = enc(x, lens.clone())
    (out * cot.to(dtype)).sum().backward()
    return enc, out.detach(), olens, x.grad, keep["embed"].grad


def _f32(t):
    return t.detach().to(torch.float32).numpy().copy()


def enc_fixture(name, conf, T2, lens, seed):
    T = 4 * T2 + 3
    feats, lens_t, cot = CH.enc_inputs(T, lens, seed + 1, D=conf["output_size"])
    e32, o32, olens, dx32, de32 = run_encoder(conf, feats, lens_t, cot, seed, torch.float32)
    e64, o64, _, dx64, de64 = run_encoder(conf, feats, lens_t, cot, seed, torch.float64)
    assert o32.shape[1] == T2
    out = dict(out_f32=_f32(o32), out_f64=_f32(o64), olens=olens.numpy().astype(np.int64), dfeats_f32=_f32(dx32),
               dfeats_f64=_f32(dx64), dembed_f32=_f32(de32), dembed_f64=_f32(de64), seed=np.int64(seed))
    for (n, p32), (_, p64) in zip(e32.named_parameters(), e64.named_parameters()):
        r64 = p64.grad.numpy()
        out["grad64/" + n] = r64.astype(np.float32)
        out["eref/" + n] = np.float64(np.abs(p32.grad.double().numpy() - r64).max() / (np.abs(r64).max() + 1e-12))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: T'={T2} olens={olens.tolist()} |out32-out64|={float((o32.double() - o64).abs().max()):.2e} "
          f"{os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


def s42_fixture():
    c = CH.S42
    conf, T2, lens, seed = c["conf"], c["T2"], c["lens"], c["seed"]
    feats, lens_t, cot = CH.enc_inputs(4 * T2 + 3, lens, seed + 1, D=conf["output_size"])
    e32, o32, olens, _, de32 = run_encoder(conf, feats, lens_t, cot, seed, torch.float32)
    e64, o64, _, _, de64 = run_encoder(conf, feats, lens_t, cot, seed, torch.float64)
    out = dict(out_f32=_f32(o32), out_f64=_f32(o64), olens=olens.numpy().astype(np.int64), seed=np.int64(seed),
               dembed_f32=_f32(de32), dembed_f64=_f32(de64))
    for (n, p32), (_, p64) in zip(e32.named_parameters(), e64.named_parameters()):
        out["gn_f32/" + n] = np.float64(p32.grad.double().norm().item())
        out["gn_f64/" + n] = np.float64(p64.grad.norm().item())
        out["gmax_f64/" + n] = np.float64(p64.grad.abs().max().item())
        out["slice_f32/" + n] = p32.grad.flatten()[:16].double().numpy().copy()
        out["slice_f64/" + n] = p64.grad.flatten()[:16].numpy().copy()
    path = os.path.join(HERE, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    print(f"{c['name']}: olens={olens.tolist()} |out32-out64|={float((o32.double() - o64).abs().max()):.2e} "
          f"{os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


# ------------------------------------------------------------------------------------------------ whole model
def build_reference(conf):
    V = conf["token_list_size"]
    enc = RefEncoder(input_size=conf["input_size"], **conf["encoder_conf"])
    dec = TransformerDecoder(vocab_size=V, encoder_output_size=enc.output_size(), **conf["decoder_conf"])
    ctc = CTC(odim=V, encoder_output_size=enc.output_size(), **conf["ctc_conf"])
    return ESPnetASRModel(vocab_size=V, frontend=None, specaug=None, normalize=UtteranceMVN(), preencoder=None,
                          encoder=enc, postencoder=None, decoder=dec, ctc=ctc, joint_network=None,
                          token_list=BH.token_list(V), **conf["model_conf"])


def run_model(conf, batch, seed, dtype):
    model = build_reference(conf).to(dtype)
    BH.load_seeded(model, seed)
    model.train()
    speech, slen, text, tlen = batch
    loss, stats, _ = model(speech.to(dtype).clone(), slen.clone(), text.clone(), tlen.clone())
    loss.backward()
    return model, loss, stats


def model_fixture():
    name, conf, B, T, lens, ulens, seed = CH.MODEL_FIXTURE
    batch = O.synthetic_batch(B, T, conf["input_size"], conf["token_list_size"], lens, ulens, seed + 1)
    m32, l32, s32 = run_model(conf, batch, seed, torch.float32)
    m64, l64, s64 = run_model(conf, batch, seed, torch.float64)
    speech, slen, text, tlen = batch
    out = dict(speech=speech.numpy().copy(), speech_lengths=slen.numpy().copy(), text=text.numpy().copy(),
               text_lengths=tlen.numpy().copy(), seed=np.int64(seed),
               num_params=np.int64(sum(p.numel() for p in m32.parameters())))
    for tag, l, s in (("f32", l32, s32), ("f64", l64, s64)):
        out["loss_" + tag] = np.float64(l.item())
        out["loss_ctc_" + tag] = np.float64(s["loss_ctc"].item())
        out["loss_att_" + tag] = np.float64(s["loss_att"].item())
        out["acc_" + tag] = np.float64(float(s["acc"]))
    for (n, p32), (_, p64) in zip(m32.named_parameters(), m64.named_parameters()):
        r64 = p64.grad.numpy()
        out["grad64/" + n] = r64.astype(np.float32)
        out["eref/" + n] = np.float64(np.abs(p32.grad.double().numpy() - r64).max() / (np.abs(r64).max() + 1e-12))
    m32.eval()
    m64.eval()
    with torch.no_grad():
        eo, el = m32.encode(speech.clone(), slen.clone())  # (UtteranceMVN normalises in place)
        eo64, _ = m64.encode(speech.double().clone(), slen.clone())
    out["enc_out"] = eo.numpy()
    out["enc_out_f64"] = eo64.float().numpy()
    out["enc_olens"] = el.numpy().astype(np.int64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: loss f32 {l32.item():.6f} f64 {l64.item():.6f} acc {float(s64['acc']):.4f} "
          f"{os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    which = sys.argv[1:] or ["layout", "keys", "enc", "s42", "model"]
    if "layout" in which:
        layout_fixture()
    if "keys" in which:
        keys_fixture()
    for name, (conf, T2, lens, seed) in CH.ENC_FIXTURES.items():
        if "enc" in which or name in which:  # (a fixture's own name: that one alone)
            enc_fixture(name, conf, T2, lens, seed)
    if "s42" in which:
        s42_fixture()
    if "model" in which:
        model_fixture()
