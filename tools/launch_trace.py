"""The native launch sequence of the small test models, one text file per case: the proof that a change of the
Python side alone moved neither behaviour nor speed.  Two commits whose traces are byte-identical launch the same
entry points in the same order with the same sizes, strides, rates and dropout seeds.

    python -m tools.launch_trace --out DIR [--case NAME ...] [--package-root PATH]
    python -m tools.launch_trace --out DIR --pack FILE | --unpack FILE      (no run: the kept form of the traces)

--package-root: import espnet_slurp_amd from PATH (a copy of another commit's package next to the same native
library) instead of from this tree; the cases, the inputs and the test helpers stay this tree's.

A line is `<entry point> <arg> ...` in the order of _native.SIGNATURES: integers and floats as they are passed, 64-bit
seeds in full, pointers as `p` (non-null) or `0` (null).  `# hook <module>` marks a module-done hook of the backward
(the data-parallel bucket launches hang on them), `# <phase>` the start of a phase.  Each case runs one training step
(forward + backward, every dropout 0.1, torch.manual_seed before it so that draw_seed is fixed) and one eval
forward, B = 2 with unequal lengths."""
import argparse
import copy
import ctypes
import hashlib
import os
import sys

import torch

SEED = 20240611
DROPOUT = 0.1


class Trace:
    def __init__(self, native):
        self.native, self.lines, self.names = native, [], {}

    def call(self, name, *args):
        out = [name]
        for t, a in zip(self.native.SIGNATURES[name], args):
            if t is self.native.P:
                null = a is None or a == 0 or (isinstance(a, ctypes.c_void_p) and not a.value)
                out.append("0" if null else "p")
            elif t is self.native.F:
                out.append(repr(float(a)))
            else:
                out.append(str(int(a)))
        assert len(args) == len(self.native.SIGNATURES[name]), name
        self.lines.append(" ".join(out))
        return self._call(name, *args)

    def hook(self, module):
        self.lines.append("# hook " + self.names.get(id(module), type(module).__name__))

    def mark(self, what):
        self.lines.append("# " + what)

    def watch(self, model):
        """Name the model's modules for the hook lines and hang the module-done hook where the autograd path
        looks for it."""
        self.names = {id(m): n or "model" for n, m in model.named_modules()}
        for m in (model, getattr(model, "encoder", None), getattr(model, "decoder", None)):
            if m is not None:
                m._grad_hook = self.hook

    def __enter__(self):
        self._call, self.native.call = self.native.call, self.call
        return self

    def __exit__(self, *exc):
        self.native.call = self._call


def _batch(dev, T, lens, ulens, V, F=80):
    g = torch.Generator().manual_seed(SEED)
    speech = torch.randn(len(lens), T, F, generator=g)
    for i, l in enumerate(lens):
        speech[i, l:] = 0.0
    text = torch.full((len(lens), max(ulens)), -1, dtype=torch.long)
    for i, u in enumerate(ulens):
        text[i, :u] = torch.randint(1, V - 1, (u,), generator=g)
    return speech.to(dev), torch.tensor(lens), text, torch.tensor(ulens)


def _model_step(tr, model, dev, T, lens, ulens, V, bucket=None, explicit=False):
    """One training step and one eval forward of a whole model.  bucket (frames, tokens): the step on the batch
    padded to its length bucket (tvalid).  explicit: forward_explicit / backward_explicit, the data-parallel path."""
    speech, sl, text, tl = _batch(dev, T, lens, ulens, V)
    tr.watch(model)
    model.train()
    model.flat.ensure_grads()
    torch.manual_seed(SEED)
    tr.mark("train")
    if bucket is None and not explicit:
        loss, _, _ = model(speech, sl, text, tl)
        loss.backward()
    else:
        tb = ub = None
        if bucket is not None:
            tb, ub = -(-T // bucket[0]) * bucket[0], -(-max(ulens) // bucket[1]) * bucket[1]
            speech = torch.nn.functional.pad(speech, (0, 0, 0, tb - T))
        prep = model.prepare(sl, text, tl, speech.shape[1], speech.shape[2], t_bucket=tb, u_bucket=ub)
        prep.to_device(dev)
        if explicit:
            loss, _, _, ctx = model.forward_explicit(speech, prep)
            tr.mark("backward")
            model.backward_explicit(ctx, torch.ones(1, device=dev), tr.hook)
        else:
            loss, _, _ = model.forward_prepared(speech, prep)
            loss.backward()
    model.eval()
    torch.manual_seed(SEED)
    tr.mark("eval")
    with torch.no_grad():
        model(speech[:, :T], sl, text, tl)
    torch.cuda.synchronize()


def _conformer(rel="latest", interctc=False):
    from tests import helpers as H
    cfg = H.small_cfg(rel)
    if interctc:
        cfg.enc.interctc_layer_idx = (1,)
        cfg.enc.interctc_use_conditioning = True
        cfg.interctc_weight = 0.3
    return cfg


def _oracle_model(tr, dev, cfg, **kw):
    from tests import helpers as H
    torch.manual_seed(SEED)
    model = H.build_model(cfg, dev, dropout=DROPOUT)  # (torch's own initialisation: the values launch nothing)
    _model_step(tr, model, dev, 97, [97, 70], [6, 4], cfg.vocab_size, **kw)


def _transformer(tr, dev):
    from tests import helpers as H
    cfg = H.c1_cfg()
    cfg.enc.num_blocks = 2
    _oracle_model(tr, dev, cfg)


def _conf_model(tr, dev, conf, T, lens, ulens):
    from espnet_slurp_amd.tasks.asr import build_model
    from tests import branchformer_helpers as BH
    model = build_model(BH.args_from_conf(conf, dropout=DROPOUT), device=dev)
    BH.load_seeded(model, 7)
    _model_step(tr, model, dev, T, lens, ulens, conf["token_list_size"])


def _branchformer(tr, dev, use_attn=True, use_cgmlp=True):
    from tests import branchformer_helpers as BH
    conf = copy.deepcopy(BH.small_conf(use_attn=use_attn))
    conf["encoder_conf"]["use_cgmlp"] = use_cgmlp
    _conf_model(tr, dev, conf, 97, [97, 70], [6, 4])


def _cbt_model(tr, dev, fused):
    from espnet_slurp_amd import kernels as K
    from tests import cbt_helpers as CH
    prev, K.CBT_ATTN_FUSED = K.CBT_ATTN_FUSED, fused
    try:
        _conf_model(tr, dev, CH.model_conf(), 55, [55, 44], [4, 3])  # T' = 13: three blocks
    finally:
        K.CBT_ATTN_FUSED = prev


def _cbt_encoder(tr, dev, T2):
    """The encoder alone through its own forward (EncoderFn): T' = 13 block mode, T' = 8 the short path."""
    from espnet_slurp_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder
    from espnet_slurp_amd.flat import FlatParams
    from tests import branchformer_helpers as BH
    from tests import cbt_helpers as CH
    enc = ContextualBlockTransformerEncoder(CH.INPUT_SIZE, **CH.encoder_conf(dropout=DROPOUT)).to(dev)
    enc.attach_flat(FlatParams(enc, dev))
    BH.load_seeded(enc, 7)
    T = 4 * T2 + 3
    feats, lens, cot = CH.enc_inputs(T, [T, T - 9], SEED)
    tr.names = {id(m): n or "encoder" for n, m in enc.named_modules()}
    enc._grad_hook = tr.hook
    assert (enc.layout(T2) is None) == (T2 <= 8)
    enc.train()
    torch.manual_seed(SEED)
    tr.mark("train")
    hs, _, _ = enc(feats.to(dev), lens)
    hs.backward(cot.to(dev))
    enc.eval()
    torch.manual_seed(SEED)
    tr.mark("eval")
    with torch.no_grad():
        enc(feats.to(dev), lens)
    torch.cuda.synchronize()


def _lm(tr, dev):
    from tests import lm_helpers as LH
    lm = LH.build_lm("B", dev)
    g = torch.Generator().manual_seed(SEED)
    ids = torch.randint(1, LH.V, (2, 9), generator=g)
    ids[1, 6:] = 0
    tr.mark("forward")
    lm(ids)
    tr.mark("forward_one_step")
    ys = ids[:, :4].clone()
    _, cache = lm.forward_one_step(ys[:, :3])
    lm.forward_one_step(ys, cache)
    torch.cuda.synchronize()


CASES = {
    "conformer_latest": lambda tr, dev: _oracle_model(tr, dev, _conformer()),
    "conformer_interctc_cond": lambda tr, dev: _oracle_model(tr, dev, _conformer(interctc=True)),
    "conformer_interctc_cond_explicit": lambda tr, dev: _oracle_model(tr, dev, _conformer(interctc=True),
                                                                      explicit=True),
    "conformer_legacy_tvalid": lambda tr, dev: _oracle_model(tr, dev, _conformer("legacy"), bucket=(64, 8)),
    "transformer": _transformer,
    "branchformer": _branchformer,
    "branchformer_attn_only": lambda tr, dev: _branchformer(tr, dev, use_cgmlp=False),
    "branchformer_cgmlp_only": lambda tr, dev: _branchformer(tr, dev, use_attn=False),
    "cbt_block_fused": lambda tr, dev: _cbt_model(tr, dev, True),
    "cbt_block_generic": lambda tr, dev: _cbt_model(tr, dev, False),
    "cbt_encoder_t13": lambda tr, dev: _cbt_encoder(tr, dev, 13),
    "cbt_encoder_t8_short": lambda tr, dev: _cbt_encoder(tr, dev, 8),
    "transformer_lm": _lm,
}


PACK_HEAD = ("# launch traces, packed: `## <case>` opens a case; `@N+K` stands for the K lines that begin at line N of "
             "the unpacked stream (every case's lines one after the other, its `## <case>` line first). "
             "python -m tools.launch_trace --unpack THIS --out DIR writes the cases back as DIR/<case>.trace")


def pack(traces):
    """{case: trace text} -> one text in which a run of two or more lines that stood earlier in the stream is
    written as a reference to it: the models share most launches, so 13 cases pack to a fifth of their lines."""
    stream, out, seen = [], [PACK_HEAD], {}
    for name, text in traces.items():
        lines = ["## " + name] + text.splitlines()
        i = 0
        while i < len(lines):
            k, n = 0, 0
            for m in seen.get(lines[i], ()):
                j = 0
                while i + j < len(lines) and m + j < len(stream) and stream[m + j] == lines[i + j]:
                    j += 1
                if j > k:
                    k, n = j, m
            k = k if k >= 2 else 1
            out.append(f"@{n + 1}+{k}" if k >= 2 else lines[i])
            for line in lines[i:i + k]:
                seen.setdefault(line, []).append(len(stream))
                stream.append(line)
            i += k
    return "\n".join(out) + "\n"


def unpack(text):
    """pack's inverse -> {case: trace text}."""
    stream = []
    for line in text.splitlines()[1:]:
        if line.startswith("@"):
            n, k = (int(v) for v in line[1:].split("+"))
            stream.extend(stream[n - 1:n - 1 + k])
        else:
            stream.append(line)
    traces, name = {}, None
    for line in stream:
        if line.startswith("## "):
            name = line[3:]
            traces[name] = ""
        else:
            traces[name] += line + "\n"
    return traces


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--package-root")
    ap.add_argument("--pack", metavar="FILE", help="no run: pack OUT/<case>.trace of every case into FILE")
    ap.add_argument("--unpack", metavar="FILE", help="no run: write FILE's cases to OUT/<case>.trace")
    args = ap.parse_args()
    if args.pack:
        with open(args.pack, "w") as f:
            f.write(pack({n: open(os.path.join(args.out, n + ".trace")).read() for n in CASES}))
        return
    if args.unpack:
        os.makedirs(args.out, exist_ok=True)
        for name, text in unpack(open(args.unpack).read()).items():
            with open(os.path.join(args.out, name + ".trace"), "w") as f:
                f.write(text)
            print(f"{name}: sha256 {hashlib.sha256(text.encode()).hexdigest()}")
        return
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    from espnet_slurp_amd import _native
    print("espnet_slurp_amd from", os.path.dirname(_native.__file__))
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda")
    for name in args.case or list(CASES):
        with Trace(_native) as tr:
            CASES[name](tr, dev)
        text = "\n".join(tr.lines) + "\n"
        with open(os.path.join(args.out, name + ".trace"), "w") as f:
            f.write(text)
        print(f"{name}: {sum(not l.startswith('#') for l in tr.lines)} launches, "
              f"{sum(l.startswith('# hook') for l in tr.lines)} hooks, sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
