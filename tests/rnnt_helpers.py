"""The RNN-Transducer lattice in plain torch: autograd-differentiable, any dtype (the tests use fp64 as the truth and
fp32 as the yardstick), no project imports.  Shared by the GPU tests, the CPU tests and the fixture generator
(tests/golden/make_transducer_golden.py registers RNNTLoss below as the `warprnnt_pytorch` the reference imports).

    alpha[0,0] = 0;  alpha[t,u] = lse(alpha[t-1,u] + lp_blank[t-1,u], alpha[t,u-1] + lp_y[t,u-1])
    beta[T-1,U] = lp_blank[T-1,U];  beta[t,u] = lse(beta[t+1,u] + lp_blank[t,u], beta[t,u+1] + lp_y[t,u])
    nll = -(alpha[T-1,U] + lp_blank[T-1,U]) = -beta[0,0]
"""
import itertools

import torch


def _lse(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return torch.logaddexp(a, b)


def lattice(lp, y, blank=0):
    """lp (T, U+1, V) log-probabilities of one utterance, y its U labels: (alpha, beta) as (T, U+1) tensors."""
    T, U1, _ = lp.shape
    U = U1 - 1
    assert len(y) == U, (len(y), U)
    lpb = lp[:, :, blank]
    lpy = [[lp[t, u, int(y[u])] for u in range(U)] for t in range(T)]
    al = [[None] * U1 for _ in range(T)]
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                al[t][u] = lp.new_zeros(())
                continue
            a = al[t - 1][u] + lpb[t - 1, u] if t > 0 else None
            b = al[t][u - 1] + lpy[t][u - 1] if u > 0 else None
            al[t][u] = _lse(a, b)
    be = [[None] * U1 for _ in range(T)]
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            if t == T - 1 and u == U:
                be[t][u] = lpb[t, u]
                continue
            a = be[t + 1][u] + lpb[t, u] if t + 1 < T else None
            b = be[t][u + 1] + lpy[t][u] if u < U else None
            be[t][u] = _lse(a, b)
    return torch.stack([torch.stack(r) for r in al]), torch.stack([torch.stack(r) for r in be])


def rnnt_nll(logits, targets, t_lens, u_lens, blank=0):
    """logits (B, T, U1, V) raw joint outputs, targets (B, >= max U) label ids, t_lens / u_lens (B,): nll (B,) from
    the forward variables, each utterance on its own valid sub-lattice."""
    out = []
    for b in range(logits.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        lp = torch.log_softmax(logits[b, :T, :U + 1], dim=-1)
        al, _ = lattice(lp, [int(v) for v in targets[b][:U]], blank)
        out.append(-(al[T - 1, U] + lp[T - 1, U, blank]))
    return torch.stack(out)


def brute_force_nll(lp, y, blank=0):
    """-log of the sum over every alignment (T blanks interleaved with the U labels in order, ending with a blank
    from (T-1, U)) of one utterance's lp (T, U+1, V): the definition the recursions must equal."""
    T, U1, _ = lp.shape
    U = U1 - 1
    terms = []
    for pos in itertools.combinations(range(T + U - 1), U):  # the final move is the blank out of (T-1, U)
        t = u = 0
        s = lp.new_zeros(())
        for k in range(T + U - 1):
            if k in pos:
                s = s + lp[t, u, int(y[u])]
                u += 1
            else:
                s = s + lp[t, u, blank]
                t += 1
        assert t == T - 1 and u == U
        terms.append(s + lp[t, u, blank])
    return -torch.logsumexp(torch.stack(terms), 0)


class RNNTLoss(torch.nn.Module):
    """warprnnt_pytorch.RNNTLoss's call form: acts (B, T, U1, V) raw joint outputs (log_softmax is applied here),
    labels (B, U) int, act_lens / label_lens (B,); mean reduction by default, fastemit_lambda 0 only."""

    def __init__(self, blank=0, reduction="mean", fastemit_lambda=0.0):
        super().__init__()
        assert fastemit_lambda == 0.0, fastemit_lambda
        self.blank, self.reduction = blank, reduction

    def forward(self, acts, labels, act_lens, label_lens):
        nll = rnnt_nll(acts, labels, act_lens, label_lens, self.blank)
        if self.reduction == "mean":
            return nll.mean()
        if self.reduction == "sum":
            return nll.sum()
        return nll
