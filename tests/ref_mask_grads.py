"""The mask explainers' gradient restated in torch on the CPU — a test helper.

d loss / d mask_logit of one triple, at any mask, by autograd of oracle.ref_explain._layer's op order over the triple's
computation graph (ref_explain.computation_graph + get_adj_coo, the masked values as leaves through _spmm), in float64
or float32.  Nothing here knows the HIP kernel's hand-derived backward.  The gradients are listed over the real
(non-placeholder) entries of the computation graph, relation by relation in get_adj_coo's order: that is
explain.mask_candidates' order (tests/test_mask_batched_host.py holds the two together).

tests/test_mask_grads_host.py ties `trajectory` to oracle.ref_explain.mask_explainer at 1e-12 and uses the mutation
switches (`cut_alpha`, `drop_ae_layer`, `struct_scale`, `grad_scale`: a backward that is wrong on purpose) to show
what a bar can and cannot see.  No GPU test passes a switch."""
import numpy as np
import torch

from oracle import ref_explain
from oracle.ref_utils import get_adj_coo


def _layer(xh, xt, aeh, aet, K, S, Wa, ba, cut_alpha):
    """ref_explain._layer on the two rows (aeh[i], aet[i]: AE_i[h], AE_i[t] as (1, D)); `cut_alpha` detaches the
    softmax, so nothing flows back through the dynamic weights."""
    ho, to = xh @ S, xt @ S
    alpha = torch.softmax(xh @ Wa + ba, dim=-1)
    if cut_alpha:
        alpha = alpha.detach()
    for i in range(K.shape[0]):
        w = torch.sigmoid(alpha[:, i])[:, None]
        ho = ho + w * (aeh[i] @ K[i])
        to = to + w * (aet[i] @ K[i])
    return torch.sigmoid(ho), torch.sigmoid(to)


def _forward(P, tr, coo, vals, cut_alpha=False, drop_ae_layer=None):
    """ref_explain.forward_with_values for one triple; `drop_ae_layer` (1, 2, 3) feeds that layer detached aggregates:
    its AE gradient is missing."""
    E = P["E"]
    h, r, t = (int(x) for x in tr)
    ae = [ref_explain._spmm(torch.as_tensor(idx[:, 0]), torch.as_tensor(idx[:, 1]), v, E)
          for (idx, _), v in zip(coo, vals)]
    aeh, aet = [a[h][None] for a in ae], [a[t][None] for a in ae]
    xh, xt = E[h][None], E[t][None]
    for l in (1, 2, 3):
        ah, at = (aeh, aet) if l != drop_ae_layer else ([a.detach() for a in aeh], [a.detach() for a in aet])
        xh, xt = _layer(xh, xt, ah, at, P[f"K{l}"], P[f"S{l}"], P[f"Wa{l}"], P[f"ba{l}"], cut_alpha)
    return torch.sigmoid(torch.sum(xh * P["rel"][r] * xt, dim=-1))[0]


def _params(params, dtype):
    return {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}


def _mask_of(mask, r):
    mask = np.asarray(mask)
    return mask[r] if mask.ndim == 3 else mask


class _Graph:
    """One triple's computation graph: per relation the COO, its real entries and their base values."""

    def __init__(self, adjacency, tr, N, R, dtype):
        self.coo = get_adj_coo(ref_explain.computation_graph(tr[0], tr[2], adjacency), N, R)
        self.real = [np.asarray(v) != 0 for _, v in self.coo]
        self.base = [torch.as_tensor(np.asarray(v), dtype=dtype) for _, v in self.coo]
        self.rel = np.concatenate([np.full(int(k.sum()), r, np.int64) for r, k in enumerate(self.real)])
        self.row = np.concatenate([idx[k, 0] for (idx, _), k in zip(self.coo, self.real)])
        self.col = np.concatenate([idx[k, 1] for (idx, _), k in zip(self.coo, self.real)])

    def logits(self, mask):
        """The mask logits of every stored entry (placeholders included), one float64 array per relation."""
        return [np.asarray(_mask_of(mask, r), np.float64)[idx[:, 0], idx[:, 1]] for r, (idx, _) in enumerate(self.coo)]


def _grads(P, g, tr, logits, before, target_ratios, dtype, cut_alpha=False, drop_ae_layer=None, struct_scale=1.0,
           grad_scale=1.0):
    """d loss / d logits over the real entries (float64 numpy), by autograd in `dtype`."""
    mk = [torch.tensor(x, dtype=dtype, requires_grad=True) for x in logits]
    mv = [b * torch.sigmoid(x) for b, x in zip(g.base, mk)]
    pred = _forward(P, tr, g.coo, mv, cut_alpha, drop_ae_layer)
    loss = -before * torch.log(pred + 1e-5)
    if target_ratios is not None:
        counts = torch.stack([x.sum() for x in mv])
        ratios = counts / counts.sum()
        struct = torch.mean((torch.as_tensor(np.asarray(target_ratios), dtype=dtype) - ratios) ** 2)
        loss = (loss + struct_scale * struct) / 2.0
    grads = torch.autograd.grad(loss, mk)
    return np.concatenate([x.numpy().astype(np.float64)[k] for x, k in zip(grads, g.real)]) * grad_scale


def candidates(adjacency, triple, N, R):
    """(rel, row, col) of the entries the gradients are listed over."""
    g = _Graph(np.asarray(adjacency), np.asarray(triple), N, R, torch.float64)
    return g.rel, g.row, g.col


def mask_grads(params, adjacency, triples, N, R, mask, target_ratios=None, dtype=torch.float64, **mutation):
    """Per triple (d loss / d mask_logit, p_before) at `mask` ((N, N): one logit per (row, col) for every relation, or
    (R, N, N)).  loss = -before log(pred + 1e-5); with ratios, (loss + mean((target - ratios)^2)) / 2."""
    P = _params(params, dtype)
    adjacency = np.asarray(adjacency)
    out = []
    for tr in np.asarray(triples):
        g = _Graph(adjacency, tr, N, R, dtype)
        before = _forward(P, tr, g.coo, g.base).detach()
        out.append((_grads(P, g, tr, g.logits(mask), before, target_ratios, dtype, **mutation), float(before)))
    return out


def trajectory(params, adjacency, triples, N, R, mask, target_ratios, epochs, alphas, b1, b2, eps,
               dtype=torch.float64, **mutation):
    """`epochs` steps per triple of the kernel's Adam form, m += (g - m)(1 - b1), v += (g g - v)(1 - b2),
    mask -= (m alpha) / (sqrt(v) + eps), with the moments shared by all triples (dense: an entry outside the current
    computation graph decays with a zero gradient), alpha = alphas[global step] and the masks reset to `mask` after
    every triple; the optimizer arithmetic runs in `dtype`.  Per triple (the last epoch's gradient, the final masked
    values), float64 numpy over the real entries."""
    P = _params(params, dtype)
    adjacency = np.asarray(adjacency)
    f = np.float64 if dtype == torch.float64 else np.float32
    c1, c2, eps = f(1) - f(b1), f(1) - f(b2), f(eps)
    m, v = np.zeros((R, N, N), f), np.zeros((R, N, N), f)
    step = 0
    out = []
    for tr in np.asarray(triples):
        g = _Graph(adjacency, tr, N, R, dtype)
        before = _forward(P, tr, g.coo, g.base).detach()
        at = (g.rel, g.row, g.col)
        mk = np.concatenate([x[k] for x, k in zip(g.logits(mask), g.real)]).astype(f)
        grad = np.zeros(len(mk))
        for _ in range(epochs):
            logits = g.logits(mask)
            off = 0
            for x, k in zip(logits, g.real):
                x[k] = mk[off:off + int(k.sum())]
                off += int(k.sum())
            grad = _grads(P, g, tr, logits, before, target_ratios, dtype, **mutation)
            dense = np.zeros((R, N, N), f)
            dense[at] = grad.astype(f)
            m = m + (dense - m) * c1
            v = v + (dense * dense - v) * c2
            mk = mk - (m[at] * f(alphas[step])) / (np.sqrt(v[at]) + eps)
            step += 1
        base = np.concatenate([np.asarray(val, f)[k] for (_, val), k in zip(g.coo, g.real)])
        out.append((grad, (base * (f(1) / (f(1) + np.exp(-mk)))).astype(np.float64)))
    return out


def layout(rel, values, R):
    """Final masked values in the oracle's layout: a relation that is empty in the computation graph shows its
    placeholder 0."""
    return np.concatenate([values[rel == r] if (rel == r).any() else np.zeros(1) for r in range(R)])
