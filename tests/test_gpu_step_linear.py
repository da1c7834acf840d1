"""esp_step_linear (csrc/lm_step.hip), the weight-streaming skinny linear of the LM step,
out[n, :] = act(LN?(x[n, :]) . W^T + b) (+ R[n, :]), against an fp64 restatement.

Shapes: N in {1, 5, 33, the row cap, the row cap + 1 (kernels.lm_step_linear then takes the generic kernels)}, K_in in
{16, 64, 100, 2048}, M in {48, 192, 33}: more than one row tile (8 rows) and column block (16 columns), sizes that
are no multiple of either, a K below one 256-float sweep and one of eight sweeps.  Every option on its own and all
together.  Split store: into a cache with more rows and positions than used, at pos 0 and 17; everything outside
[:N, pos] must stay as it was and the dense part must equal the unsplit launch's columns bit for bit.

Gate: the error relative to fp64 (max |got - want| / max |want|) may be at most twice that of the existing
LayerNorm + linear_fwd path on the same inputs (kernels.lm_step_linear with LM_STEP_FUSED off); both are printed."""
import pytest
import torch

from espnet_slurp_amd import _native
from espnet_slurp_amd import kernels as K

pytestmark = pytest.mark.gpu

CAP = K.LM_STEP_MAX_ROWS
OPTIONS = {"plain": (), "ln": ("ln",), "bias": ("bias",), "relu": ("relu",), "residual": ("res",),
           "all": ("ln", "bias", "relu", "res")}
SHAPES = sorted({(5, k, m) for k in (16, 64, 100, 2048) for m in (48, 192, 33)}
                | {(n, k, m) for n in (1, 5, 33, CAP, CAP + 1) for k, m in ((64, 48), (2048, 33), (100, 192))})


def _inputs(N, Kin, M, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(N, Kin), W=r(M, Kin) / Kin ** 0.5, b=0.5 * r(M), gamma=1 + 0.1 * r(Kin), beta=0.1 * r(Kin), R=r(N, M))


def _want(t, opts, eps):
    x = t["x"].double()
    if "ln" in opts:
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + eps) * t["gamma"].double() + t["beta"].double()
    y = x @ t["W"].double().T
    if "bias" in opts:
        y = y + t["b"].double()
    if "relu" in opts:
        y = torch.relu(y)
    if "res" in opts:
        y = y + t["R"].double()
    return y


def _kw(d, opts, eps):
    return dict(ln=(d["gamma"], d["beta"], eps) if "ln" in opts else None, relu="relu" in opts,
                R=d["R"] if "res" in opts else None)


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.fixture
def count_calls(monkeypatch):
    calls = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


@pytest.mark.parametrize("N,Kin,M", SHAPES)
def test_step_linear_matches_fp64(dev, monkeypatch, count_calls, N, Kin, M):
    t = _inputs(N, Kin, M, 1000 * N + Kin + M)
    d = {k: v.to(dev) for k, v in t.items()}
    for name, opts in OPTIONS.items():
        eps = 1e-5 if name == "ln" else 1e-12
        want = _want(t, opts, eps)
        b = d["b"] if "bias" in opts else None
        del count_calls[:]
        monkeypatch.setattr(K, "LM_STEP_FUSED", True)
        got = K.lm_step_linear(d["x"], d["W"], b, **_kw(d, opts, eps))
        used = list(count_calls)
        assert (used == ["esp_step_linear"]) == (N <= CAP), (N, used)
        monkeypatch.setattr(K, "LM_STEP_FUSED", False)
        ref = K.lm_step_linear(d["x"], d["W"], b, **_kw(d, opts, eps))
        assert "esp_step_linear" not in count_calls[len(used):]
        e_got, e_ref = _rel(got, want), _rel(ref, want)
        print(f"N={N} K={Kin} M={M} {name}: step_linear {e_got:.3e}, LayerNorm + linear_fwd {e_ref:.3e}")
        assert got.shape == (N, M) and torch.isfinite(got).all()
        assert e_got <= 2 * e_ref, (name, e_got, e_ref)


def test_step_linear_beyond_the_cap_on_the_kernel_itself(dev):
    """The cap is a dispatch choice, not a limit of the kernel: one row more than the cap, in a last, partial tile."""
    N, Kin, M = CAP + 1, 64, 48
    t = _inputs(N, Kin, M, 3)
    d = {k: v.to(dev) for k, v in t.items()}
    out = torch.empty(N, M, device=dev)
    K.step_linear(d["x"], d["W"], d["b"], out, ln=(d["gamma"], d["beta"], 1e-12), relu=True, R=d["R"])
    assert _rel(out, _want(t, OPTIONS["all"], 1e-12)) <= 1e-5  # fp32 over K = 64 products: ~1e-7; a wrong row is O(1)


@pytest.mark.parametrize("pos", [0, 17])
@pytest.mark.parametrize("fused", [True, False])
def test_split_store_writes_only_its_slot(dev, monkeypatch, pos, fused):
    N, Kin, D = 5, 64, 64
    M, c0 = 3 * D, D
    t = _inputs(N, Kin, M, 7)
    d = {k: v.to(dev) for k, v in t.items()}
    monkeypatch.setattr(K, "LM_STEP_FUSED", fused)
    kw = dict(ln=(d["gamma"], d["beta"], 1e-12))
    whole = K.lm_step_linear(d["x"], d["W"], d["b"], **kw)
    cache = torch.full((N + 3, 32, M - c0), -77.0, device=dev)
    q = K.lm_step_linear(d["x"], d["W"], d["b"], c0=c0, cache=cache, pos=pos, **kw)
    assert torch.equal(q[:, :c0], whole[:, :c0]), "the dense part must equal the unsplit launch"
    assert torch.equal(cache[:N, pos], whole[:, c0:])
    keep = torch.ones(N + 3, 32, dtype=torch.bool, device=dev)
    keep[:N, pos] = False
    assert bool((cache[keep] == -77.0).all()), "a cache element outside [:N, pos] changed"
    want = _want(t, ("ln", "bias"), 1e-12)
    assert _rel(torch.cat([q[:, :c0], cache[:N, pos]], 1), want) <= 1e-5


def test_step_linear_rejects_a_store_outside_the_cache(dev):
    x, W = torch.zeros(5, 64, device=dev), torch.zeros(192, 64, device=dev)
    q = torch.zeros(5, 64, device=dev)
    cache = torch.zeros(4, 8, 128, device=dev)
    with pytest.raises(_native.NativeError, match=r"\(-1\).*split store"):
        K.step_linear(x, W, None, q, c0=64, cache=cache, pos=0)  # 5 rows into a cache of 4
    cache = torch.zeros(8, 8, 128, device=dev)
    with pytest.raises(_native.NativeError, match=r"\(-1\).*split store"):
        K.step_linear(x, W, None, q, c0=64, cache=cache, pos=8)  # position 8 of 8
    with pytest.raises(_native.NativeError, match=r"\(-1\).*multiple of 4"):
        K.step_linear(torch.zeros(5, 66, device=dev)[:, :62], torch.zeros(8, 62, device=dev), None,
                      torch.zeros(5, 8, device=dev))
    assert float(cache.abs().max()) == 0.0
