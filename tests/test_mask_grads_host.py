"""What the mask explainers' tests can and cannot see, on the CPU (tests/ref_mask_grads.py, no GPU).

tests/test_gpu_mask_batched.py compares final masked values after 5 or 10 Adam steps at 1e-5.  Adam's first steps are
close to lr sign(g), so that bar passes a backward whose dynamic-weight path is cut.  The per-query gradient bar
max(4 max|g32 - g64|, 1e-5 max|g64|) (bounds.query_bar; both sides from the reference) rejects it, and every other
mutant tried here.  tests/test_gpu_mask_grads.py holds the kernel to that bar."""
import numpy as np
import pytest
import torch

from iddgcn_amd import explain as X
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from oracle import ref_explain
from tests import ref_mask_grads as RM
from tests.bounds import query_bar
from tests.test_mask_batched_host import EMPTY, make_params, synthetic_case

KINDS = ("gnnexplainer", "iddgcn")
SHAPES = [(32, 3), (64, 4), (64, 8), (32, 8)]
N_SYN = 40


def ratios_of(kind, R):
    """tests/test_gpu_mask_batched.py's kind_kw: descending target ratios for the IDDGCN explainer, none otherwise."""
    if kind == "gnnexplainer":
        return None
    r = np.arange(R, 0, -1, dtype=np.float64)
    return tuple(r / r.sum())


def epochs_of(kind):
    return 5 if kind == "gnnexplainer" else 10


def keras_alphas(count, lr=1e-3, b1=0.9, b2=0.999):
    """explain.mask_adam_alphas in float64."""
    t = np.arange(1, count + 1, dtype=np.float64)
    return lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)


def synthetic(D, R, kind, wa_scale=1.0, saturate=False):
    """synthetic_case as (adjacency, queries, init, params, ratios); the IDDGCN explainer drops the empty triple
    (its relation-ratio loss divides 0 by 0 there)."""
    tri, q, init, params = synthetic_case(R=R, D=D)
    if kind == "iddgcn":
        q = np.delete(q, EMPTY, 0)
    if wa_scale != 1.0:
        params = dict(params, **{f"Wa{l}": params[f"Wa{l}"] * np.float32(wa_scale) for l in (1, 2, 3)})
    if saturate:      # tests/test_gpu_explain_batched.py's make_params(saturate=True) scaling
        params = dict(params)
        for l in (1, 2, 3):
            params[f"Wa{l}"] = params[f"Wa{l}"] * np.float32(60)
            params[f"S{l}"] = params[f"S{l}"] * np.float32(6)
            params[f"K{l}"] = params[f"K{l}"] * np.float32(12)
    return tri, q, init, params, ratios_of(kind, R)


def large_degree_case(D):
    """tests/test_gpu_mask_batched.py::test_large_degrees' graph: N = 320, R = 3 with relation 2 empty, rows of degree
    1, 63, 64, 65 and 300 (twice), a column of degree 290 in both relations; (5, 0, 6) has more than 1024 candidates."""
    rng = np.random.default_rng(3)
    N, R = 320, 3
    rows = []
    for node, deg in ((1, 1), (2, 63), (3, 64), (4, 65)):
        cols = np.sort(rng.choice(np.arange(7, N), deg, replace=False))
        rows.append(np.stack([np.full(deg, node), np.zeros(deg, np.int64), cols], 1))
    for r in (0, 1):
        rows.append(np.stack([np.full(300, 5), np.full(300, r), np.arange(10, 310)], 1))
        rows.append(np.stack([np.arange(10, 300), np.full(290, r), np.full(290, 6)], 1))
    rows.append(np.array([[0, 0, 9], [0, 1, 5], [8, 1, 0], [5, 0, 5]]))
    tri = np.concatenate(rows).astype(np.int64)
    params = make_params(N, R, D, rng)
    init = rng.standard_normal((N, N)).astype(np.float32)
    q = np.array([(1, 0, 2), (2, 1, 3), (3, 0, 4), (4, 1, 5), (5, 0, 6), (6, 1, 5), (5, 0, 5), (3, 1, 1)], np.int64)
    return N, R, tri, q, init, params


def host_candidates(tri, q, N, R):
    """explain.mask_candidates on the host: (dadj, qptr, entry, crel, ccol, crole)."""
    dadj = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
    return (dadj, *X.mask_candidates(dadj, q))


def check_input_conditions(q, qptr, crole, g64, kind):
    """From the candidate lists and the reference alone: some query has candidates that feed the head row (the head
    row's layer-2/3 input then depends on the masks, so the softmax path carries gradient), and some candidate has
    only its column at h or t: under GNNExplainer its gradient is exactly 0."""
    assert any((crole[qptr[j]:qptr[j + 1]] & X.ROLE_HEAD).any() for j in range(len(q)))
    col_only = [crole[qptr[j]:qptr[j + 1]] == 0 for j in range(len(q))]
    assert any(c.any() for c in col_only)
    if kind == "gnnexplainer":
        for j, c in enumerate(col_only):
            assert not g64[j][c].any(), j
            assert g64[j][~c].all(), j           # and nowhere else: the zeros below are the structural ones


def grads_pair(tri, q, N, R, mask, params, ratios):
    """(g64, g32, p64) per query."""
    r64 = RM.mask_grads(params, tri, q, N, R, mask, ratios, torch.float64)
    r32 = RM.mask_grads(params, tri, q, N, R, mask, ratios, torch.float32)
    return [a for a, _ in r64], [a for a, _ in r32], [p for _, p in r64]


# -- the reference is the oracle's ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_reproduces_the_oracle(kind):
    """Keras's hyper-parameters and the float64 step-size table: oracle.ref_explain.mask_explainer's final masked
    values on all twelve (eleven) triples, shared moments included, to 1e-12."""
    D, R = 32, 3
    tri, q, init, params, ratios = synthetic(D, R, kind)
    ep = epochs_of(kind)
    ref = ref_explain.mask_explainer(params, tri, q, N_SYN, R, init, num_epochs=ep, target_ratios=ratios)[2]
    ours = RM.trajectory(params, tri, q, N_SYN, R, init, ratios, ep, keras_alphas(len(q) * ep), 0.9, 0.999, 1e-7)
    worst = 0.0
    for j, tr in enumerate(q):
        rel, row, col = RM.candidates(tri, tr, N_SYN, R)
        lay = RM.layout(rel, ours[j][1], R)
        assert lay.shape == ref[j].shape, j
        if lay.size:
            worst = max(worst, float(np.abs(lay - ref[j]).max()))
    print(f"trajectory vs oracle {kind}: max |final - oracle| {worst:.2e}")
    assert worst <= 1e-12
    # the candidate order is mask_candidates'
    _, qptr, entry, crel, ccol, _ = host_candidates(tri, q, N_SYN, R)
    for j, tr in enumerate(q):
        rel, _, col = RM.candidates(tri, tr, N_SYN, R)
        assert np.array_equal(rel, crel[qptr[j]:qptr[j + 1]]) and np.array_equal(col, ccol[qptr[j]:qptr[j + 1]])


# -- the blind spot of the finals bar ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,R", [(32, 3), (64, 4)])
def test_finals_bar_passes_a_cut_alpha_path(D, R, kind):
    """A backward without the softmax / dynamic-weight path moves the final masked values by less than the 1e-5 bar
    of tests/test_gpu_mask_batched.py: that bar cannot see the path."""
    tri, q, init, params, ratios = synthetic(D, R, kind)
    ep = epochs_of(kind)
    ref = ref_explain.mask_explainer(params, tri, q, N_SYN, R, init, num_epochs=ep, target_ratios=ratios)[2]
    mut = RM.trajectory(params, tri, q, N_SYN, R, init, ratios, ep, keras_alphas(len(q) * ep), 0.9, 0.999, 1e-7,
                        cut_alpha=True)
    worst = 0.0
    for j, tr in enumerate(q):
        rel, _, _ = RM.candidates(tri, tr, N_SYN, R)
        if len(rel):
            worst = max(worst, float(np.abs(RM.layout(rel, mut[j][1], R) - ref[j]).max()))
    print(f"cut alpha path, finals D={D} R={R} {kind}: max |final - oracle| {worst:.2e} (bar 1e-5)")
    assert 0 < worst <= 1e-5


# -- the gradient bar --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,R", SHAPES)
def test_gradient_bar_rejects_every_mutant(D, R, kind):
    """Float64 mutants against max(4 max|g32 - g64|, 1e-5 max|g64|) at the initial mask: every gradient x 1.001 is
    rejected on every query that has a candidate; the cut softmax path, each layer's missing AE gradient and the
    structure loss x 1.01 on at least one."""
    tri, q, init, params, ratios = synthetic(D, R, kind)
    g64, g32, _ = grads_pair(tri, q, N_SYN, R, init, params, ratios)
    _, qptr, _, _, _, crole = host_candidates(tri, q, N_SYN, R)
    check_input_conditions(q, qptr, crole, g64, kind)
    bars = [query_bar(a, b) for a, b in zip(g64, g32)]
    own = max(float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(g64, g32) if a.size)
    mutants = dict(scaled=dict(grad_scale=1.001), cut_alpha=dict(cut_alpha=True), drop_ae1=dict(drop_ae_layer=1),
                   drop_ae2=dict(drop_ae_layer=2), drop_ae3=dict(drop_ae_layer=3))
    if ratios is not None:
        mutants["struct"] = dict(struct_scale=1.01)
    line = []
    for name, kw in mutants.items():
        mut = [a for a, _ in RM.mask_grads(params, tri, q, N_SYN, R, init, ratios, torch.float64, **kw)]
        ratio = [float(np.abs(m_ - a).max() / bar) for m_, a, bar in zip(mut, g64, bars) if a.size]
        line.append(f"{name} {min(ratio):.3g}..{max(ratio):.3g}")
        if name == "scaled":
            assert min(ratio) > 1, (name, ratio)
        else:
            assert max(ratio) > 1, (name, ratio)
    print(f"mutants D={D} R={R} {kind}: fp32 reference within {own:.1e} of max|g|; error / bar " + ", ".join(line))


@pytest.mark.parametrize("kind", KINDS)
def test_single_relation_has_no_alpha_path(kind):
    """R = 1: the softmax has one entry, its backward is an exact zero, and cutting it changes nothing."""
    tri, q, init, params, ratios = synthetic(32, 1, kind)
    ref = RM.mask_grads(params, tri, q, N_SYN, 1, init, ratios)
    mut = RM.mask_grads(params, tri, q, N_SYN, 1, init, ratios, cut_alpha=True)
    assert any(a.any() for a, _ in ref)
    for (a, _), (b, _) in zip(ref, mut):
        assert np.array_equal(a, b)


def test_mask_may_differ_per_relation():
    """An (R, N, N) mask that repeats an (N, N) one gives the same gradients; one that does not, others."""
    tri, q, init, params, ratios = synthetic(32, 3, "iddgcn")
    rng = np.random.default_rng(5)
    a = RM.mask_grads(params, tri, q[:3], N_SYN, 3, init, ratios)
    b = RM.mask_grads(params, tri, q[:3], N_SYN, 3, np.stack([init] * 3), ratios)
    c = RM.mask_grads(params, tri, q[:3], N_SYN, 3, np.stack([init] * 3) + rng.uniform(-3, 3, (3, N_SYN, N_SYN)),
                      ratios)
    for (x, _), (y, _), (z, _) in zip(a, b, c):
        assert np.array_equal(x, y) and np.abs(x - z).max() > 1e-3 * np.abs(x).max()
