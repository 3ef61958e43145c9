"""Explanation ground truth and the explainers' Precision / Recall / F1 @ k.

``construct_ground_truth`` is explanation/ground_truth.py:6-76 on the GPU (include/iddgcn_ground_truth.h states the
five steps; csrc/ground_truth.hip runs them, one workgroup per query, in the reference's order and bitwise the same on
every run).  ``ground_truth_table`` lays the result out like the reference's ``gt_all.csv``, ``filter_ground_truth`` is
explanation/gt_process.py:12-22,35-41 (the test triples that have a ground truth, with it), and
``evaluate_explanations`` scores a set of explanations with ``explain.explanation_metrics`` (eval_test.py:15-39).

The reference keeps ONE ``added_combinations`` set for three kinds of pairs: (drug, mutation) of every matched response
row, (drug0, d) of the drug-similarity triples and (mu0, m) of the mutation-similarity triples.  When no id is both a
mutation and a drug the three kinds cannot collide, and the set reduces to "emit (drug0, drug_rel, d) once per distinct
d, (mu0, mu_rel, m) once per distinct m".  That is what the kernel computes, so ``GroundTruthIndex`` checks the
condition and raises when it does not hold (the bundled data: mutations below 661, drugs from 661 up).
"""
import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import IddgcnError
from .graph import _as_triples, _device_triples

LIST_CAPACITY = L.GT_LIST_CAPACITY


def load_similarity_csv(path, reference_header=True):
    """A headerless similarity CSV (``mu_similar0.97.csv`` / ``drug_similar0.78.csv``: rows ``a,rel,b``) as an
    (n, 3) int64 array.  With ``reference_header`` (the default) the FIRST DATA ROW IS DROPPED: the reference reads
    these files with ``pd.read_csv`` and renames the columns (ground_truth.py:81-86), so pandas consumes row 0 as
    the header and the reference's ``gt_all.csv`` was computed without it (16179 of 16180 and 1173 of 1174 rows).
    ``reference_header=False`` keeps every row."""
    rows = np.loadtxt(path, delimiter=",", dtype=np.int64, ndmin=2)
    if rows.shape[1] != 3:
        raise IddgcnError(f"{path}: expected 3 columns, got {rows.shape[1]}")
    return rows[1:] if reference_header else rows


def load_response_csv(path):
    """``triplets_dc.csv`` (a real ``obj,rel,sbj`` header, then ``mu,rel,drug`` rows) as an (M, 3) int64 array."""
    return np.loadtxt(path, delimiter=",", dtype=np.int64, skiprows=1, ndmin=2)


def _triples_tensor(x):
    """(n, 3) int64 tensor on the device the data already lives on (numpy -> CPU)."""
    if isinstance(x, torch.Tensor):
        t = x[0] if x.dim() == 3 and x.shape[0] == 1 else x
        if t.dim() != 2 or t.shape[1] != 3:
            raise IddgcnError(f"triples must be (n, 3), got {tuple(t.shape)}")
        return t.to(torch.int64)
    return torch.as_tensor(_as_triples(x))


def check_id_sets(dc, mu_sim, drug_sim):
    """The mutation side (column 0 of dc, both columns of mu_sim) and the drug side (column 2 of dc, both columns of
    drug_sim) must not share an id (module docstring): raises IddgcnError if they do, or if an id is negative.  Runs
    where the data lives (numpy / CPU tensors on the host).  Returns (number of nodes, number of relations) the
    tables span."""
    dc, mu_sim, drug_sim = (_triples_tensor(x) for x in (dc, mu_sim, drug_sim))
    dev = dc.device
    mu_side = torch.cat([dc[:, 0], mu_sim[:, 0].to(dev), mu_sim[:, 2].to(dev)])
    drug_side = torch.cat([dc[:, 2], drug_sim[:, 0].to(dev), drug_sim[:, 2].to(dev)])
    ids = torch.cat([mu_side, drug_side, dc[:, 1]])
    if ids.numel() and int(ids.min()) < 0:
        raise IddgcnError("ground truth: negative id")
    N = int(torch.cat([mu_side, drug_side]).max()) + 1 if mu_side.numel() + drug_side.numel() else 1
    R = int(dc[:, 1].max()) + 1 if dc.shape[0] else 1
    is_mu = torch.zeros(N, dtype=torch.bool, device=dev)
    is_drug = torch.zeros(N, dtype=torch.bool, device=dev)
    is_mu[mu_side] = True
    is_drug[drug_side] = True
    both = is_mu & is_drug
    if bool(both.any()):
        raise IddgcnError(
            f"ground truth: id {int(both.nonzero()[0])} is both a mutation and a drug; the reference's single "
            "added_combinations set is only a per-value dedup when the two id sets are disjoint")
    return N, R


class GroundTruthIndex:
    """The device tables one ground-truth construction needs (the two similarity-list CSRs and the dc lookup
    table), built once; ``query`` then answers any number of query batches."""

    def __init__(self, dc, mu_sim, drug_sim, device="cuda", num_entities=None, num_relations=None):
        N, R = check_id_sets(dc, mu_sim, drug_sim)
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise IddgcnError("ground truth runs on the GPU (no CPU fallback)")
        self.dc = _device_triples(dc, dev)
        mu_sim, drug_sim = _device_triples(mu_sim, dev), _device_triples(drug_sim, dev)
        self.N = N = max(N, int(num_entities or 0))
        self.R = R = max(R, int(num_relations or 0))
        *self.mu, e0 = ops.gt_sim_lists(mu_sim, N)
        *self.drug, e1 = ops.gt_sim_lists(drug_sim, N)
        *self.table, e2 = ops.gt_dc_table(self.dc, N, R)
        if int(torch.cat([e0, e1, e2]).max()):           # the host check above covers it; the kernels' own flag
            raise IddgcnError("ground truth: id out of range in the table build")

    def query(self, queries=None, drug_rel=2, mu_rel=3):
        """(ptr int64 [Q+1], triples int64 [total, 3]) on the device; ``queries=None`` means the rows of dc."""
        q = self.dc if queries is None else _device_triples(queries, self.device)
        if q.shape[0]:
            lo, hi = int(q[:, [0, 2]].min()), int(q[:, [0, 2]].max())
            rlo, rhi = int(q[:, 1].min()), int(q[:, 1].max())
            if lo < 0 or rlo < 0:
                raise IddgcnError("ground truth: negative id in the queries")
            if hi >= self.N or rhi >= self.R:
                raise IddgcnError("ground truth: a query names an id beyond the tables'; build the index with "
                                  "num_entities / num_relations that cover the queries")
        length, err = ops.ground_truth_count(q, self.mu, self.drug, self.table, self.N, self.R)
        ptr = ops.gt_exclusive_scan(length)
        total, err = (int(v) for v in torch.cat([ptr[-1:], err.to(torch.int64)]).cpu())
        if err:
            raise IddgcnError(f"ground truth: a query's similarity list is longer than {LIST_CAPACITY} entries "
                              "(IDDGCN_GT_LIST_CAPACITY); nothing is truncated")
        tri = ops.ground_truth_fill(q, self.mu, self.drug, self.table, self.N, self.R, ptr, total, drug_rel, mu_rel)
        return ptr, tri


def construct_ground_truth(dc, mu_sim, drug_sim, queries=None, drug_rel=2, mu_rel=3, device="cuda"):
    """ground_truth.construct_ground_truth for every query on the GPU.

    dc: (M, 3) response triples (mu, rel, drug); mu_sim / drug_sim: (n, 3) similarity triples (a, _, b); queries:
    (Q, 3) triples (mu0, rel0, drug0), default the rows of dc (what the reference runs).  numpy arrays or GPU
    tensors.  Returns GPU tensors ``(ptr int64 [Q+1], triples int64 [total, 3])``: query q's ground truth is
    ``triples[ptr[q]:ptr[q+1]]`` in the reference's order.  Raises IddgcnError if an id is both a mutation and a drug
    (module docstring) or a similarity list is longer than LIST_CAPACITY."""
    N = R = None
    if queries is not None:      # a query may name an id that no table mentions (empty lists, no response rows)
        queries = _triples_tensor(queries)
        if queries.shape[0]:
            N, R = int(queries[:, [0, 2]].max()) + 1, int(queries[:, 1].max()) + 1
    return GroundTruthIndex(dc, mu_sim, drug_sim, device, N, R).query(queries, drug_rel, mu_rel)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def ground_truth_table(queries, ptr, triples):
    """The layout of the reference's ``gt_all.csv`` (ground_truth.py:93,108-111): float64 (Q, 3 + 3 * max length),
    row q = the query, then its triples flattened, NaN-padded."""
    queries, ptr, triples = _as_triples(queries), _np(ptr).astype(np.int64), _np(triples).astype(np.int64)
    Q = queries.shape[0]
    if ptr.shape != (Q + 1,):
        raise IddgcnError(f"ptr must have shape ({Q + 1},)")
    lens = np.diff(ptr)
    width = 3 * int(lens.max()) if Q else 0
    out = np.full((Q, 3 + width), np.nan)
    out[:, :3] = queries
    row = np.repeat(np.arange(Q), 3 * lens)
    col = 3 + np.arange(3 * ptr[-1]) - np.repeat(3 * ptr[:-1], 3 * lens)
    out[row, col] = triples.reshape(-1)[:3 * ptr[-1]]
    return out


def filter_ground_truth(test_triples, queries, ptr, triples, min_count=1):
    """gt_process.py:12-22,35-41: left-merge the test triples with the ground truth on (obj, rel, sbj), in test order
    (a test triple matching several queries gives one row per query, in query order, as pandas' merge does), and keep
    the rows with at least ``min_count`` ground-truth triples.  Returns (kept test triples (K, 3) int64, list of K
    int64 (n_k, 3) arrays)."""
    test, queries = _as_triples(test_triples), _as_triples(queries)
    ptr, triples = _np(ptr).astype(np.int64), _np(triples).astype(np.int64)
    where = {}
    for i, k in enumerate(map(tuple, queries)):
        where.setdefault(k, []).append(i)
    kept, gts = [], []
    for row in test:
        for i in where.get(tuple(row), (None,)):
            gt = triples[ptr[i]:ptr[i + 1]] if i is not None else triples[:0]
            if len(gt) >= min_count:
                kept.append(row)
                gts.append(gt)
    return np.asarray(kept, dtype=np.int64).reshape(-1, 3), gts


def evaluate_explanations(preds, gt, top=5, exp_num=10):
    """Precision@top / Recall@top / F1@top of every explanation against its ground truth through
    ``explain.explanation_metrics`` (which keeps the reference's ``list(set)[:top]`` selection).  preds: one (k, 3)
    array per triple; gt: the matching ground-truth arrays.  Returns (per-triple (n, 3) float64, their means (3,))."""
    from .explain import explanation_metrics
    if len(preds) != len(gt):
        raise IddgcnError(f"{len(preds)} explanations for {len(gt)} ground truths")
    per = np.array([explanation_metrics(_np(p), _np(g), top=top, exp_num=exp_num) for p, g in zip(preds, gt)],
                   dtype=np.float64).reshape(-1, 3)
    return per, (per.mean(0) if len(per) else np.zeros(3))
