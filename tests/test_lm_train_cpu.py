"""LM training without a GPU: the ABI's new entry points, the served-shape predicate of the fused causal attention,
and the self-consistency of the training fixture (tests/golden/lm_train*.npz, make_lm_train_golden.py)."""
import os
import re

import numpy as np

from tests.helpers import golden
from tests.lm_helpers import LM_CFGS, V, golden_state, lm_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esp_causal_attn_fwd", "esp_causal_attn_bwd", "esp_lm_front_fwd", "esp_lm_front_bwd")


def _header():
    with open(os.path.join(ROOT, "include", "espnet_mi355.h"), encoding="utf-8") as f:
        return f.read()


def _args(proto):
    return [a for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",") if a.strip()]


def test_header_and_signature_table_have_the_entry_points():
    from espnet_slurp_amd import _native
    h = _header()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\([^;]*\);", h)
        assert m, name
        assert name in _native.SIGNATURES, name
        assert len(_args(m.group(0))) == len(_native.SIGNATURES[name]), name


def test_abi_version_is_42_and_documented():
    from espnet_slurp_amd import _native
    assert _native.ABI_VERSION == 42
    documented = [int(n) for n in re.findall(r"ABI (\d+)", _header())]
    assert max(documented) == 42
    with open(os.path.join(ROOT, "espnet_slurp_amd", "csrc", "elementwise.hip"), encoding="utf-8") as f:
        assert re.search(r"esp_abi_version\(void\) \{ return 42; \}", f.read())


def test_causal_attn_ok_follows_the_table():
    from espnet_slurp_amd import kernels as K
    for L, dk in ((64, 64), (1, 16), (32, 128)):
        assert K.causal_attn_ok(L, dk), (L, dk)
    for L, dk in ((65, 64), (10, 48), (0, 16)):
        assert not K.causal_attn_ok(L, dk), (L, dk)
    assert K.causal_attn_ok(64, 128) and not K.causal_attn_ok(65, 128)  # Lmax(128) = 64, as the header states
    assert K.LM_ATTN_FUSED is True


def test_fixture_is_self_consistent():
    g = golden("lm_train")
    b1 = (lm_golden()["fwd_text"], lm_golden()["fwd_lens"])
    assert g["b2_lens"].tolist() == [12, 1, 9, 12] and g["b2_text"].shape == (4, 12)
    for row, n in zip(g["b2_text"], g["b2_lens"]):
        assert (row[:n] > 0).all() and (row[:n] < V - 1).all() and (row[n:] == 0).all()
    ntok = {"b1": int(b1[1].sum()) + len(b1[1]), "b2": int(g["b2_lens"].sum()) + 4}
    assert ntok == {"b1": 17, "b2": 38}
    for tag in LM_CFGS:
        part = golden(f"lm_train.{tag}")
        shapes = {k: tuple(v.shape) for k, v in golden_state(tag).items()}
        for b in ("b1", "b2"):
            key = f"{tag}.{b}."
            assert int(g[key + "ntokens"]) == ntok[b]
            assert float(g[key + "margin"]) >= 1e-5  # no ReLU decision of the reference within 1e-5 of zero
            l64, l32 = float(g[key + "loss_f64"]), float(g[key + "loss_f32"])
            assert 0.0 < l64 < 2 * np.log(V) and abs(l32 - l64) < 1e-5
            scale = max(float(g[key + "gmax_f64/" + n]) for n in shapes)
            for n, shp in shapes.items():
                gr = part[f"{b}.g/{n}"]
                assert gr.shape == shp and gr.dtype == np.float32 and np.isfinite(gr).all(), n
                gmax, gn = float(g[key + "gmax_f64/" + n]), float(g[key + "gn_f64/" + n])
                assert abs(float(np.abs(gr).max()) - gmax) <= 1e-6 * gmax + 1e-30, n
                assert abs(float(np.linalg.norm(gr.astype(np.float64))) - gn) <= 1e-6 * gn + 1e-30, n
                # (a key bias has no gradient at all: softmax is invariant to it; fp32 leaves noise there)
                assert float(g[key + "emax_f32/" + n]) <= 1e-3 * gmax + 1e-6 * scale, n
            assert set(k for k in part if k.startswith(b + ".g/")) == {f"{b}.g/{n}" for n in shapes}
    assert g["A.steps.loss_f64"].shape == (3,) and g["A.steps.loss_f32"].shape == (3,)
    assert abs(float(g["A.steps.loss_f64"][0]) - float(g["A.b1.loss_f64"])) <= 1e-12
