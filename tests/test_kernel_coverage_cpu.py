"""Every exported entry point of the native library is called by a GPU test directly.

espnet_slurp_amd/kernels.py is parsed (ast) into wrapper -> the "esp_*" names it passes to _native.call, names built
from a literal prefix included (every signature that starts with the prefix) and the private helpers a wrapper
calls followed through.  A key of _native.SIGNATURES counts as tested when some tests/test_gpu_*.py or
tests/*helpers.py calls one of its wrappers through the kernels module (`K.wrapper(`, whatever the module is
called there, or a name imported from it), or holds the entry point's name as a string literal of its own (a direct
_native.call).  Names in docstrings and comments do not count.  The entries that compute nothing are listed in
NOT_COMPUTE, each with its reason; the ones whose kernel-level test goes through the single class that owns the
launch (the LSTM layer, the frontend, the rel-pos attention module) in THROUGH_OWNER, each line checked
against the sources it names.
"""
import ast
import glob
import os
import re

from espnet_slurp_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "espnet_slurp_amd", "kernels.py")

# entry points that launch no computation: (pattern, reason)
NOT_COMPUTE = [
    (r"esp_last_error", "the message of the last failed call: read by _native.call on every error a test provokes"),
    (r"esp_abi_version", "checked by _native.load before any call"),
    (r"esp_set_\w+", "a process-wide switch: tested through the kernels it selects"),
    (r"esp_get_\w+", "reads a process-wide switch back"),
    (r"\w+_workspace_bytes", "host arithmetic: the launcher it belongs to checks the size it is handed"),
    (r"esp_attn_slot_check_errors", "the counter of a debugging build: -1 in every other build"),
    (r"esp_f32_gemm_products", "a constant of the build (6 or 1 products per fp32 GEMM term), read once by kernels.py"),
]

# Compute entry points whose kernel-level GPU test drives them through the one class that owns the launch, not
# through kernels.py: entry -> (test file, owner's source file, owner class the test file imports, what is compared).
# The check below holds each line to its word: the owner's source calls the entry's wrapper, the test file imports
# the owner.  A new entry point belongs in a direct test, not here.
THROUGH_OWNER = {
    "esp_fbank_fwd": ("tests/test_gpu_frontend.py", "espnet_slurp_amd/asr/frontend/default.py", "DefaultFrontend",
                      "log-mel features against the reference's golden output and the oracle, ragged lengths"),
    "esp_lstm_cell_fwd": ("tests/test_gpu_lstm.py", "espnet_slurp_amd/asr/decoder/transducer_decoder.py", "LSTMLayer",
                          "against torch.nn.LSTM, forward"),
    "esp_lstm_cell_bwd": ("tests/test_gpu_lstm.py", "espnet_slurp_amd/asr/decoder/transducer_decoder.py", "LSTMLayer",
                          "against torch.nn.LSTM's autograd"),
    "esp_relpos_attn_fwd": ("tests/test_gpu_blocks.py", "espnet_slurp_amd/blocks.py", "RelPositionMultiHeadedAttention",
                            "the 32-row-block score kernel against the fp64 oracle (test_relpos_mha_fused_dk64)"),
    "esp_relpos_attn_bwd": ("tests/test_gpu_blocks.py", "espnet_slurp_amd/blocks.py", "RelPositionMultiHeadedAttention",
                            "the fused score gradient against the fp64 oracle (test_relpos_mha_fused_dk64)"),
    "esp_relpos_flash_fwd": ("tests/test_gpu_flash.py", "espnet_slurp_amd/blocks.py", "RelPositionMultiHeadedAttention",
                             "against the fp64 oracle and the materialised path"),
    "esp_relpos_flash_bwd": ("tests/test_gpu_flash.py", "espnet_slurp_amd/blocks.py", "RelPositionMultiHeadedAttention",
                             "against the fp64 oracle and the materialised path"),
}


def _is_native_call(node):
    f = node.func
    return (isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name)
            and f.value.id == "_native")


def _entry_names(arg):
    """The SIGNATURES keys the first argument of a _native.call can name."""
    if isinstance(arg, ast.Constant) and isinstance(arg.value, str):
        return {arg.value}
    if isinstance(arg, ast.IfExp):
        return _entry_names(arg.body) | _entry_names(arg.orelse)
    out = set()  # a built name ("esp_x" + suffix, an f-string): every signature with one of its literal prefixes
    for n in ast.walk(arg):
        if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value.startswith("esp_"):
            out |= {k for k in _native.SIGNATURES if k.startswith(n.value)}
    return out


def wrapper_map():
    """Top-level function or class of kernels.py -> the entry points it reaches (through private helpers too)."""
    with open(KERNELS) as f:
        tree = ast.parse(f.read())
    tops = {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    direct, helpers = {}, {}
    for name, node in tops.items():
        direct[name], helpers[name] = set(), set()
        for c in ast.walk(node):
            if not isinstance(c, ast.Call):
                continue
            if _is_native_call(c) and c.args:
                direct[name] |= _entry_names(c.args[0])
            elif isinstance(c.func, ast.Name) and c.func.id in tops and c.func.id.startswith("_"):
                helpers[name].add(c.func.id)

    def reach(name, seen):
        out = set(direct[name])
        for h in helpers[name] - seen:
            out |= reach(h, seen | {name})
        return out
    return {name: reach(name, set()) for name in tops if not name.startswith("_")}


def _base(func):
    """(alias, attribute) of the innermost `alias.attribute` of a call's function expression, or None."""
    while isinstance(func, ast.Attribute):
        if isinstance(func.value, ast.Name):
            return func.value.id, func.attr
        func = func.value
    return None


def _tested_in(path, wrappers):
    """(wrappers of kernels.py the file calls, string literals of the file that are entry-point names)."""
    with open(path) as f:
        tree = ast.parse(f.read())
    aliases, imported = set(), {}
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and (n.module == "espnet_slurp_amd" or (n.level and not n.module)):
            aliases |= {a.asname or a.name for a in n.names if a.name == "kernels"}
        elif isinstance(n, ast.ImportFrom) and n.module == "espnet_slurp_amd.kernels":
            imported.update({a.asname or a.name: a.name for a in n.names})
        elif isinstance(n, ast.Import):
            aliases |= {a.asname for a in n.names if a.name == "espnet_slurp_amd.kernels" and a.asname}
    called, literal = set(), set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Call):
            b = _base(n.func)
            if b and b[0] in aliases and b[1] in wrappers:
                called.add(b[1])
            elif b and b[0] in imported and imported[b[0]] in wrappers:  # Planes.of(...)
                called.add(imported[b[0]])
            elif isinstance(n.func, ast.Name) and imported.get(n.func.id) in wrappers:
                called.add(imported[n.func.id])
        elif isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value in _native.SIGNATURES:
            literal.add(n.value)
    return called, literal


def untested_entry_points():
    wrappers = wrapper_map()
    files = sorted(set(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))
                       + glob.glob(os.path.join(ROOT, "tests", "*helpers.py"))))
    assert files
    covered = set()
    for path in files:
        called, literal = _tested_in(path, wrappers)
        covered |= literal
        for w in called:
            covered |= wrappers[w]
    return sorted(k for k in _native.SIGNATURES
                  if k not in covered and not any(re.fullmatch(p, k) for p, _ in NOT_COMPUTE))


def test_through_owner_lines_hold():
    wrappers = wrapper_map()
    direct_missing = set(untested_entry_points())
    for entry, (test_file, owner_file, owner, what) in THROUGH_OWNER.items():
        assert entry in _native.SIGNATURES and what, entry
        assert entry in direct_missing, f"{entry} has a direct test now: drop its THROUGH_OWNER line"
        called, _ = _tested_in(os.path.join(ROOT, owner_file), wrappers)
        assert any(entry in wrappers[w] for w in called), f"{owner_file} does not launch {entry}"
        with open(os.path.join(ROOT, owner_file)) as f:
            assert any(isinstance(n, ast.ClassDef) and n.name == owner for n in ast.walk(ast.parse(f.read()))), owner
        with open(os.path.join(ROOT, test_file)) as f:
            tree = ast.parse(f.read())
        assert any(isinstance(n, ast.ImportFrom) and any(a.name == owner for a in n.names) for n in ast.walk(tree)), \
            f"{test_file} does not import {owner}"


def test_wrapper_map_reads_kernels_py():
    """The parse finds what it is meant to find: plain wrappers, a class, names chosen by a branch, a private helper."""
    w = wrapper_map()
    assert w["layernorm_bwd"] == {"esp_layernorm_bwd"}
    assert w["scale_dropout"] == {"esp_scale_dropout", "esp_scale_dropout_planes"}
    assert w["conv1_fwd"] == {"esp_conv1_fwd", "esp_conv1_fwd_bf16", "esp_conv1_fwd_bits"}
    assert "esp_f32_to_planes" in w["Planes"]
    assert {"esp_gemm_f32", "esp_gemm_f32_pl"} <= w["gemm"]
    reached = set().union(*w.values())
    missing = [k for k in _native.SIGNATURES
               if k not in reached and not any(re.fullmatch(p, k) for p, _ in NOT_COMPUTE)]
    assert not missing, f"entry points no wrapper of kernels.py passes to _native.call: {missing}"


def test_not_compute_list_is_exact():
    for pat, reason in NOT_COMPUTE:
        assert reason and any(re.fullmatch(pat, k) for k in _native.SIGNATURES), pat


def test_every_compute_entry_point_has_a_direct_gpu_test():
    missing = [k for k in untested_entry_points() if k not in THROUGH_OWNER]
    assert not missing, f"entry points no GPU test calls directly: {missing}"
