"""Golden vectors for Transformer LM training, generated with the reference's own TransformerLM / ESPnetLanguageModel
(imported through refshim) in .train() mode, in fp32 and in fp64.  Data only.
Run:  python tests/golden/make_lm_train_golden.py

The LMs are A, B and C of lm.npz (make_lm_golden.py; dropout_rate 0).  B's PositionalEncoding keeps a dropout of its
own at the espnet1 Encoder's default positional_dropout_rate 0.1, which TransformerLM does not pass on; it is set to
0 here (and in the tests through TransformerLM.positional_dropout_rate), so every run is deterministic.
Two batches: "b1" = lm.npz's fwd_text (lengths 7, 5, 2) and "b2", drawn here, lengths (12, 1, 9, 12).

lm_train.npz:
  b2_text, b2_lens, b2_seed     the second batch and the seed it was drawn with
  {A,B,C}.{b1,b2}.loss_f32/_f64, .ntokens
  {A,B,C}.{b1,b2}.margin        the smallest |ReLU pre-activation| (fp64) over the valid positions of the input
                                layer's LayerNorm output and of every FFN's w_1 output; the generator asserts that
                                it is >= MARGIN and that the fp32 and fp64 signs agree everywhere, and draws b2 with
                                another seed until they do, so the reference alone stays clear of a ReLU flip
  {A,B,C}.{b1,b2}.gmax_f64/<p>  max |grad| (fp64) of parameter <p>
  {A,B,C}.{b1,b2}.gn_f64/<p>, gn_f32/<p>    the gradient's L2 norm in both precisions
  {A,B,C}.{b1,b2}.emax_f32/<p>  max |grad_f32 - grad_f64|: the reference fp32 run's own whole-tensor error
  A.steps.loss_f32/_f64         (3,) the losses of three optimizer steps (torch.optim.Adam lr 1e-3,
                                clip_grad_norm_ 5.0, batches b1, b2, b1) from the fixture parameters
lm_train.{A,B,C}.npz (one file per LM keeps every file below the repository's 1 MiB limit):
  {b1,b2}.g/<p>                 the whole fp64 gradient of parameter <p>, stored rounded to fp32 (6e-8 relative: three
                                orders below the gate's 1e-4 floor).  The fp32 run's gradients enter the gate only
                                through their error figures above, so they are not stored element by element.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import refshim  # noqa: E402

refshim.install()
from tests.golden.make_lm_golden import LM_CFGS, V  # noqa: E402

MARGIN = 1e-5
B2_LENS = (12, 1, 9, 12)
STEP_BATCHES = ("b1", "b2", "b1")


def build(tag, state, dtype):
    from espnet2.lm.espnet_model import ESPnetLanguageModel
    from espnet2.lm.transformer_lm import TransformerLM
    m = ESPnetLanguageModel(TransformerLM(V, **LM_CFGS[tag]), V)
    m.lm.load_state_dict(state)
    for mod in m.modules():  # B: PositionalEncoding's own dropout stays at the espnet1 Encoder's default 0.1
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(dtype).train()


def run(model, text, lens):
    """One training forward + backward; returns (loss, ntokens, {name: grad}, {site: pre-activation at valid rows})."""
    pre = {}
    hooks = []
    valid = (torch.arange(int(lens.max()) + 1)[None, :] < (lens + 1)[:, None])

    def keep(name):
        def hook(_m, _i, out):
            pre[name] = out.detach()[valid].double().clone()
        return hook

    enc = model.lm.encoder
    hooks.append(enc.embed[1].register_forward_hook(keep("front")))
    for i, layer in enumerate(enc.encoders):
        hooks.append(layer.feed_forward.w_1.register_forward_hook(keep(f"ffn{i}")))
    model.zero_grad(set_to_none=True)
    loss, _stats, weight = model(text, lens)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {n: p.grad.detach().clone() for n, p in model.lm.named_parameters()}
    return float(loss), int(weight), grads, pre


def margin(pre32, pre64):
    """(smallest |pre-activation| in fp64, whether every fp32 sign agrees with the fp64 one)."""
    m, agree = float("inf"), True
    for k, v64 in pre64.items():
        m = min(m, float(v64.abs().min()))
        agree = agree and bool(((pre32[k] > 0) == (v64 > 0)).all())
    return m, agree


def draw_b2(seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(B2_LENS)
    text = torch.zeros(len(B2_LENS), max(B2_LENS), dtype=torch.int64)
    for i, l in enumerate(lens):
        text[i, :l] = torch.randint(1, V - 1, (int(l),), generator=g)
    return text, lens


def main():
    lm = dict(np.load(os.path.join(HERE, "lm.npz"), allow_pickle=False))
    states = {t: {k[len(t) + 3:]: torch.tensor(v) for k, v in lm.items() if k.startswith(t + ".p.")} for t in LM_CFGS}
    b1 = (torch.tensor(lm["fwd_text"]), torch.tensor(lm["fwd_lens"]))

    def all_runs(batch):
        res = {}
        for tag in LM_CFGS:
            r32 = run(build(tag, states[tag], torch.float32), *batch)
            r64 = run(build(tag, states[tag], torch.float64), *batch)
            res[tag] = (r32, r64) + margin(r32[3], r64[3])
        return res

    runs = {"b1": all_runs(b1)}
    for tag, (_, _, m, agree) in runs["b1"].items():
        assert agree and m >= MARGIN, ("b1", tag, m, agree)
    seed = 100
    while True:
        b2 = draw_b2(seed)
        runs["b2"] = all_runs(b2)
        if all(agree and m >= MARGIN for (_, _, m, agree) in runs["b2"].values()):
            break
        print("b2 seed", seed, "inside the ReLU margin:", {t: r[2:] for t, r in runs["b2"].items()})
        seed += 1
    out = {"b2_text": b2[0].numpy(), "b2_lens": b2[1].numpy(), "b2_seed": np.array(seed)}
    parts = {t: {} for t in LM_CFGS}
    for bname, res in runs.items():
        for tag, (r32, r64, m, _agree) in res.items():
            key = f"{tag}.{bname}."
            assert r32[1] == r64[1]
            out[key + "loss_f32"], out[key + "loss_f64"] = np.array(r32[0]), np.array(r64[0])
            out[key + "ntokens"], out[key + "margin"] = np.array(r64[1]), np.array(m)
            for n, g64 in r64[2].items():
                g32 = r32[2][n].double()
                out[key + "gmax_f64/" + n] = np.array(float(g64.abs().max()))
                out[key + "gn_f64/" + n] = np.array(float(g64.norm()))
                out[key + "gn_f32/" + n] = np.array(float(g32.norm()))
                out[key + "emax_f32/" + n] = np.array(float((g32 - g64).abs().max()))
                parts[tag][f"{bname}.g/{n}"] = g64.numpy().astype(np.float32)
            print(tag, bname, "loss", r64[0], "fp32 off by", abs(r32[0] - r64[0]), "ntokens", r64[1], "margin", m)
    # three optimizer steps on A
    batches = {"b1": b1, "b2": b2}
    for bits, dt in ((32, torch.float32), (64, torch.float64)):
        model = build("A", states["A"], dt)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = []
        for bname in STEP_BATCHES:
            opt.zero_grad()
            loss, _, _ = model(*batches[bname])
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
            opt.step()
            losses.append(float(loss))
        out[f"A.steps.loss_f{bits}"] = np.array(losses)
        print("A steps", bits, losses)
    np.savez_compressed(os.path.join(HERE, "lm_train.npz"), **out)
    for tag, d in parts.items():
        np.savez_compressed(os.path.join(HERE, f"lm_train.{tag}.npz"), **d)
    for f in ["lm_train.npz"] + [f"lm_train.{t}.npz" for t in LM_CFGS]:
        size = os.path.getsize(os.path.join(HERE, f))
        print("wrote", f, size, "bytes")
        assert size < (1 << 20), f


if __name__ == "__main__":
    main()
