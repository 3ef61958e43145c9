"""Deletion / insertion curves restated in torch on the CPU, vectorised over (query, variant) — a test helper.

Every variant's AE rows are built from the query's candidate list (explain.curve_steps' arrays) and pushed through
oracle.ref_explain._layer's op order; oracle.ref_explain.forward_with_values on the edited full COO gives the same
numbers one variant at a time (tests/test_fidelity_host.py holds the two together at 1e-12 in float64)."""
import numpy as np
import torch


def keep_matrix(step, K):
    """(C, 2 (K + 1)) bool: candidate c is kept in variant v.  Variants 0 .. K are the deletion points (drop the
    candidates of step < j), K + 1 .. 2 K + 1 the insertion points (keep only those)."""
    step = np.asarray(step, np.int64)
    j = np.arange(K + 1)
    flipped = (step[:, None] >= 0) & (step[:, None] < j[None, :])
    return np.concatenate([~flipped, flipped], 1)


def curves(params, triples, cand, K, dtype=torch.float64):
    """(deletion, insertion), (Q, K + 1) float64 numpy each, computed in ``dtype``."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    E = P["E"]
    tr = np.asarray(triples, np.int64)
    Q, V = len(tr), 2 * (K + 1)
    R, D = P["rel"].shape
    h, r, t = (torch.as_tensor(tr[:, i]) for i in range(3))
    qptr = np.asarray(cand["qptr"], np.int64)
    q_of = np.repeat(np.arange(Q), np.diff(qptr))
    rel, col, role = (np.asarray(cand[k], np.int64) for k in ("rel", "col", "role"))
    keep = torch.as_tensor(keep_matrix(cand["step"], K)).to(dtype)                  # (C, V)
    val = torch.tensor(np.asarray(cand["val"]), dtype=dtype)
    ecol = E[torch.as_tensor(col)]                                                   # (C, D)
    ae = torch.zeros(Q * 2 * R, V, D, dtype=dtype)
    for side in (0, 1):
        feeds = torch.as_tensor((role >> side) & 1).to(dtype)
        contrib = (keep * (val * feeds)[:, None])[:, :, None] * ecol[:, None, :]     # (C, V, D)
        ae.index_add_(0, torch.as_tensor((q_of * 2 + side) * R + rel), contrib)
    ae = ae.view(Q, 2, R, V, D)
    xh, xt = E[h][:, None, :].expand(Q, V, D), E[t][:, None, :].expand(Q, V, D)
    for l in (1, 2, 3):
        Kl, S, Wa, ba = P[f"K{l}"], P[f"S{l}"], P[f"Wa{l}"], P[f"ba{l}"]
        ho, to = xh @ S, xt @ S
        alpha = torch.softmax(xh @ Wa + ba, dim=-1)
        for i in range(R):
            w = torch.sigmoid(alpha[..., i])[..., None]
            ho = ho + w * (ae[:, 0, i] @ Kl[i])
            to = to + w * (ae[:, 1, i] @ Kl[i])
        xh, xt = torch.sigmoid(ho), torch.sigmoid(to)
    p = torch.sigmoid(torch.sum(xh * P["rel"][r][:, None, :] * xt, dim=-1)).numpy().astype(np.float64)
    return p[:, :K + 1], p[:, K + 1:]


def make_params(N, R, D, rng, saturate=False):
    """tests/test_gpu_explain_batched.py's scaling."""
    p = {"E": rng.standard_normal((N, D)) / 8}
    for l in (1, 2, 3):
        p.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / 8,
                  f"relw{l}": np.zeros(R), f"Wa{l}": rng.standard_normal((D, R)) / 8,
                  f"ba{l}": rng.standard_normal(R) / 8})
    p["rel"] = rng.standard_normal((R, D)) / np.sqrt(D / 64)
    if saturate:      # one-hot softmax rows, sigmoids driven to 0 / 1
        for l in (1, 2, 3):
            p[f"Wa{l}"] = p[f"Wa{l}"] * 60
            p[f"S{l}"] = p[f"S{l}"] * 6
            p[f"K{l}"] = p[f"K{l}"] * 12
    return {k: v.astype(np.float32) for k, v in p.items()}


def model_with(params, N, R, D):
    """An IDDGCN_Model of that size holding ``params`` (make_params' dict)."""
    from iddgcn_amd import get_IDDGCN_Model
    model = get_IDDGCN_Model(N, R, D, D, 123, None, 0, 0)
    model._set_named(params)
    model._invalidate()
    return model


def small_case(d, R, saturate=False, seed=0):
    """N = 50: 400 random triples over nodes 0..48 and the self loop (7, 0, 7); node 49 has no stored entry.  200
    queries with a repeated one, h == t and empty rows on either side.  Returns (N, adjacency triples, params, q)."""
    rng = np.random.default_rng(seed + 17 * d + R)
    N = 50
    tri = np.stack([rng.integers(0, 49, 400), rng.integers(0, R, 400), rng.integers(0, 49, 400)], 1)
    tri = np.concatenate([tri, [[7, 0, 7]]]).astype(np.int64)
    params = make_params(N, R, d, rng, saturate)
    q = np.stack([rng.integers(0, N, 200), rng.integers(0, R, 200), rng.integers(0, N, 200)], 1).astype(np.int64)
    q[1] = q[0]                                   # a repeated query
    q[2] = (7, 0, 7)                              # h == t
    q[3] = (49, R - 1, 3)                         # empty rows on the head side
    q[4] = (5, 0, 49)                             # .. on the tail side
    q[5] = (49, 0, 49)
    return N, tri, params, q


def mixed_explanations(dadj, q, seed=0):
    """One explanation of up to 10 edges per query: seven distinct stored entries of rows h and t (effective), a stored
    entry of which only the column is h or t, an edge that is not stored, and a repeat of the first edge, interleaved;
    every fifth list is cut to 4 edges (a short list), and a query with few candidates gets a short list anyway."""
    from iddgcn_amd import explain as X
    rnd = X.random_explanations(dadj, q, 7, seed)
    row, col, rel, real = X._entry_table(dadj)
    out = []
    for j, (h, _, t) in enumerate(q):
        e = [tuple(x) for x in rnd[j]]
        only_col = np.flatnonzero(real & ((col == h) | (col == t)) & (row != h) & (row != t))
        extra = {2: (row[only_col[0]], rel[only_col[0]], col[only_col[0]]) if len(only_col) else None,
                 4: (49, 0, 49),                  # node 49 has no stored entry
                 6: e[0] if e else None}
        mixed = []
        while e or extra:
            if len(mixed) in extra:
                x = extra.pop(len(mixed))
                if x is not None:
                    mixed.append(x)
                    continue
            if e:
                mixed.append(e.pop(0))
            elif extra:
                x = extra.pop(min(extra))
                if x is not None:
                    mixed.append(x)
        mixed = mixed[:4] if j % 5 == 4 else mixed
        out.append(np.array(mixed, np.int64).reshape(-1, 3))
    return out


def edited_values(dadj, cand, q, variant, K):
    """The full adjacency's value lists (one float64 array per relation, entry order) of variant ``variant`` of query
    ``q``: what oracle.ref_explain.forward_with_values takes."""
    vals = dadj.base_values.cpu().numpy().astype(np.float64)
    a, b = cand["qptr"][q], cand["qptr"][q + 1]
    keep = keep_matrix(cand["step"][a:b], K)[:, variant]
    vals[np.asarray(cand["entry"][a:b], np.int64)] = np.where(keep, cand["val"][a:b].astype(np.float64), 0.0)
    off = dadj.rel_offsets
    return [vals[off[r]:off[r + 1]] for r in range(dadj.num_relations)]
