"""Integrated gradients, CPU side: the float64 restatement (tests/ref_integrated_gradients.py) against the oracle, the
completeness it must show, proof that the GPU test's bars reject wrong answers, and the host logic of
explain.integrated_gradients_batched.  Inputs: tests/ref_fidelity.small_case, its first 40 queries."""
import types

import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from oracle import ref_explain
from tests import ref_fidelity as RF
from tests import ref_integrated_gradients as RI

NQ = 40
GAUSS32 = X.quadrature_rule(32, "gauss")
_CASES = {}


def case(d, R, saturate=False, exclude_target=False, relations=None, values=False):
    """(params, q, host adjacency, candidates, mats).  ``values``: the stored values are drawn from [0.5, 1.5]."""
    key = (d, R, saturate, exclude_target, None if relations is None else tuple(relations), values)
    if key not in _CASES:
        N, tri, params, q = RF.small_case(d, R, saturate)
        q = q[:NQ]
        mats = get_adj_mats(tri, N, R)
        if values:
            rng = np.random.default_rng(5)
            for m in mats:
                m.values = (m.values * rng.uniform(0.5, 1.5, m.nnz)).astype(np.float32)
        host = DeviceAdjacency(mats, N, "cpu")
        cand = X.counterfactual_candidates(host, q, exclude_target=exclude_target, relations=relations)
        _CASES[key] = (params, q, host, cand, mats)
    return _CASES[key]


# -- the restatement against the oracle --------------------------------------------------------------------------
def test_restatement_gradients_match_the_oracle():
    """g_j(alpha) of the restatement = oracle.ref_explain.value_grads on the full COO with the query's eligible
    candidates scaled by alpha: two nodes, three queries (the h == t query among them), 1e-12 in float64.  The case
    excludes the target edges and relation 1, so candidates of both kinds are on the path."""
    params, q, host, cand, mats = case(64, 4, exclude_target=True, relations=[0, 2, 3], values=True)
    coo = [(np.stack([m.rows, m.cols], 1), m.values) for m in mats]
    assert (q[2, 0] == q[2, 2]) and not cand["eligible"].all() and cand["eligible"].any()
    worst = 0.0
    for alpha in (GAUSS32[0][3], GAUSS32[0][20]):
        p, g = RI.gradients(params, q, cand, alpha)
        for j in (0, 2, 7):
            a, b = cand["qptr"][j], cand["qptr"][j + 1]
            assert b > a
            want_p, grads = ref_explain.value_grads(params, q[j], coo, RI.edited_values(host, cand, j, alpha))
            want = np.concatenate(grads)[cand["entry"][a:b].astype(np.int64)]
            assert abs(p[j] - want_p) <= 1e-12
            assert np.abs(want).max() > 1e-6
            worst = max(worst, float(np.abs(g[a:b] - want).max()))
    print(f"restatement against oracle.ref_explain.value_grads: max |dg| {worst:.3e}")
    assert worst <= 1e-12


# -- completeness ------------------------------------------------------------------------------------------------
def _relations_for(R):
    return [r for r in (0, 2) if r < R]


@pytest.mark.parametrize("d,R,saturate", [(64, 4, False), (32, 2, False), (64, 8, False), (64, 4, True),
                                          (32, 2, True)])
def test_completeness_float64(d, R, saturate):
    """Gauss-Legendre with 32 nodes: |gap| <= 1e-12 on every query, with every candidate eligible and (non-saturated
    cases) with relations=[0, 2] (R = 2 has no relation 2: [0] there) and exclude_target=True; the attributions do
    move: the mean |p - p_base| is far above the bound."""
    variants = [dict()] + ([] if saturate else [dict(relations=_relations_for(R), exclude_target=True)])
    for kw in variants:
        params, q, _, cand, _ = case(d, R, saturate, **kw)
        out = RI.integrate(params, q, cand, *GAUSS32)
        gap = np.abs(out["gap"])
        print(f"completeness d={d} R={R} saturate={saturate} {kw}: max |gap| {gap.max():.2e}, mean |p - p_base| "
              f"{np.abs(out['p_full'] - out['p_base']).mean():.3e}")
        assert gap.max() <= 1e-12
        assert np.abs(out["p_full"] - out["p_base"]).mean() > 1e-6
        assert (out["attr"][~cand["eligible"]] == 0).all()
        empty = np.diff(cand["qptr"]) == 0
        assert empty.sum() >= 1 and (out["total"][empty] == 0).all() and (out["gap"][empty] == 0).all()


@pytest.mark.parametrize("d,R", [(64, 4), (32, 2)])
def test_midpoint_misses_on_saturated_weights(d, R):
    """The textbook midpoint sum with 32 nodes does not meet the bound Gauss meets on the saturated cases: the reason
    the default rule is Gauss."""
    params, q, _, cand, _ = case(d, R, True)
    gap = np.abs(RI.integrate(params, q, cand, *X.quadrature_rule(32, "midpoint"))["gap"]).max()
    print(f"midpoint, 32 nodes, saturated d={d} R={R}: max |gap| {gap:.2e}")
    assert gap > 1e-12


# -- the GPU bars are not vacuous --------------------------------------------------------------------------------
def _refs(params, q, cand, rule=GAUSS32):
    return RI.integrate(params, q, cand, *rule), RI.integrate(params, q, cand, *rule, dtype=torch.float32)


def _broken(wrong, ref64, bar, cand):
    """Per eligible candidate: the wrong answer lies outside its query's bar."""
    q_of = np.repeat(np.arange(len(bar)), np.diff(cand["qptr"]))
    return (np.abs(wrong - ref64["attr"]) > bar[q_of])[cand["eligible"]]


@pytest.mark.parametrize("d,R", [(64, 4), (32, 2), (64, 8)])
def test_gpu_bar_rejects_wrong_answers(d, R):
    """The bar of tests/test_gpu_integrated_gradients.py (per query, max(4 max_j |attr32 - attr64|, 2^-20 max_j
    |attr64|)) is broken by (a) the gradient with the dynamic weights' softmax detached, on at least 25 % of the
    candidates, (b) the weights rolled against the nodes, (c) val_j left out on a graph with non-unit values.  (b) and
    (c) change every attribution by a relative amount of order 0.1 against bars of relative order 1e-6, so they are
    held to the same 25 % (observed: every candidate)."""
    params, q, _, cand, _ = case(d, R)
    ref64, ref32 = _refs(params, q, cand)
    bar = RI.attr_bar(ref64, ref32, cand["qptr"])[0]
    detached = RI.integrate(params, q, cand, *GAUSS32, detach_weights=True)
    share = _broken(detached["attr"], ref64, bar, cand).mean()
    rolled = RI.integrate(params, q, cand, GAUSS32[0], np.roll(GAUSS32[1], 7))
    share_rolled = _broken(rolled["attr"], ref64, bar, cand).mean()
    print(f"d={d} R={R}: bars {bar[bar > 0].min():.2e} .. {bar.max():.2e}; softmax detached: max |d| "
          f"{np.abs(detached['attr'] - ref64['attr']).max():.2e}, outside the bar {share:.3f}; weights rolled: "
          f"outside the bar {share_rolled:.3f}")
    assert share >= 0.25
    assert share_rolled >= 0.25
    params, q, _, cand, _ = case(d, R, values=True)
    assert np.abs(cand["val"] - 1).max() > 0.3
    ref64, ref32 = _refs(params, q, cand)
    bar = RI.attr_bar(ref64, ref32, cand["qptr"])[0]
    noval = RI.integrate(params, q, cand, *GAUSS32, times_val=False)
    share_val = _broken(noval["attr"], ref64, bar, cand).mean()
    print(f"d={d} R={R}: val left out: outside the bar {share_val:.3f}")
    assert share_val >= 0.25


# -- host logic --------------------------------------------------------------------------------------------------
def test_quadrature_rule():
    for name in ("gauss", "midpoint"):
        for m in (1, 5, 256, L.PATH_MAX_STEPS):
            al, om = X.quadrature_rule(m, name)
            assert al.shape == om.shape == (m,) and abs(om.sum() - 1) <= 1e-12
            assert (al > 0).all() and (al < 1).all() and (om > 0).all() and (np.diff(al) > 0).all()
    al, om = X.quadrature_rule(4, "gauss")
    assert abs((om * al ** 7).sum() - 1 / 8) <= 1e-14            # exact up to degree 2 m - 1
    assert np.allclose(X.quadrature_rule(4, "midpoint")[0], [0.125, 0.375, 0.625, 0.875])
    for bad in (0, L.PATH_MAX_STEPS + 1):
        with pytest.raises(L.IddgcnError, match="steps"):
            X.quadrature_rule(bad)
    with pytest.raises(L.IddgcnError, match="quadrature"):
        X.quadrature_rule(8, "simpson")


def _result(cand, q, R, attr, p_full, toward="flip", k=3, **kw):
    n = len(q)
    qp = cand["qptr"]
    q_of = np.repeat(np.arange(n), np.diff(qp))
    total = np.zeros(n)
    np.add.at(total, q_of, attr.astype(np.float64))
    host = dict(attr=attr.astype(np.float32), total=total.astype(np.float32), p_full=p_full.astype(np.float32),
                p_base=np.zeros(n, np.float32), gap=(total - p_full).astype(np.float32))
    rank = lambda s: X._rank_candidates(None, None, cand, n, s, k)  # noqa: E731
    return X._attribution_result(cand, n, R, host, np.full(n, 32), toward, 0.5, rank, **kw)


def test_ranking_direction_ties_and_relation_sums():
    params, q, host, cand, _ = case(64, 4, relations=[0, 1, 3])
    n, R, qp = len(q), 4, cand["qptr"]
    rng = np.random.default_rng(2)
    attr = np.where(cand["eligible"], rng.integers(-3, 4, len(cand["entry"])) / 4.0, 0.0)   # many ties, both signs
    p_full = np.where(np.arange(n) % 2 == 0, 0.9, 0.1)
    row = np.concatenate(host.rows)
    for toward, sign in (("flip", np.where(p_full > 0.5, 1, -1)), ("lower", np.ones(n)), ("raise", -np.ones(n))):
        out = _result(cand, q, R, attr, p_full, toward, return_attributions=True)
        assert np.array_equal(out["direction"], sign.astype(np.int64))
        for j in range(n):
            sl = slice(qp[j], qp[j + 1])
            el = cand["eligible"][sl]
            score = (sign[j] * attr[sl])[el]
            entry = cand["entry"][sl][el]
            o = np.lexsort((entry, -score))[:3]                  # descending, ties by ascending entry id
            assert np.array_equal(out["scores"][j], score[o].astype(np.float32))
            e = entry[o].astype(np.int64)
            want = np.stack([row[e], cand["rel"][sl][el][o], cand["col"][sl][el][o]], 1)
            assert np.array_equal(out["edges"][j], want) and out["edges"][j].dtype == np.int64
            table = out["attributions"][1][j]
            assert np.isnan(table[~el]).all() and np.array_equal(table[el], attr[sl][el].astype(np.float32))
    assert out["relation_attribution"].shape == (n, R) and (out["relation_attribution"][:, 2] == 0).all()
    assert np.abs(out["relation_attribution"].sum(1) - out["total"]).max() <= 1e-6
    assert np.abs(out["relation_attribution"]).sum() > 0
    s = X.integrated_gradients_summary(out, tol=0.5)
    gap = np.abs(out["gap"].astype(np.float64))
    assert s["n"] == n and s["max_abs_gap"] == gap.max() and abs(s["mean_abs_gap"] - gap.mean()) <= 1e-15
    assert s["within_tol"] == (gap <= 0.5).mean() and s["mean_steps"] == 32
    assert abs(sum(s["relation_share"].values()) - 1) <= 1e-12 and s["relation_share"][2] == 0
    assert abs(s["mean_shift"] - np.abs(out["p"].astype(np.float64)).mean()) <= 1e-12
    with pytest.raises(ValueError):
        X.integrated_gradients_summary(dict(out, gap=out["gap"][:3]))


def test_tol_doubling_schedule():
    """A stub engine whose gap is 1 / m for the odd queries and 0 for the even ones: with tol = 1 / 100 and steps = 16
    the odd queries run at 16, 32, 64, 128 and stop there (1 / 128 <= tol); with max_steps = 64 they stop at 64."""
    _, q, _, cand, _ = case(32, 2)
    n, calls = len(q), []

    def run(idx, sub, alpha, omega):
        m = len(alpha)
        calls.append((m, idx.copy()))
        assert len(sub["qptr"]) == len(idx) + 1 and abs(omega.sum() - 1) <= 1e-12
        lens = np.diff(cand["qptr"])[idx]
        assert np.array_equal(np.diff(sub["qptr"]), lens)
        for nm in ("entry", "rel", "col", "eligible"):
            want = np.concatenate([cand[nm][cand["qptr"][j]:cand["qptr"][j + 1]] for j in idx] + [cand[nm][:0]])
            assert np.array_equal(sub[nm], want), nm
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32))  # noqa: E731
        return dict(attr=t(np.repeat(idx * 1000 + m, lens)), total=t(idx), p_full=t(idx), p_base=t(idx),
                    gap=t(np.where(idx % 2 == 1, 1.0 / m, 0.0)))

    out, used, rounds = X._refine_by_gap(run, cand, n, 16, "gauss", 0.01, 1024)
    assert [m for m, _ in calls] == [16, 32, 64, 128] and rounds == 4
    odd = np.arange(n)[np.arange(n) % 2 == 1]
    assert all(np.array_equal(ix, odd) for _, ix in calls[1:]) and len(calls[0][1]) == n
    assert np.array_equal(used, np.where(np.arange(n) % 2 == 1, 128, 16))
    lens = np.diff(cand["qptr"])
    assert np.array_equal(out["attr"].numpy(), np.repeat(np.arange(n) * 1000 + used, lens).astype(np.float32))
    assert np.array_equal(out["gap"].numpy(), np.where(np.arange(n) % 2 == 1, 1 / 128, 0).astype(np.float32))
    calls.clear()
    out, used, rounds = X._refine_by_gap(run, cand, n, 16, "gauss", 0.01, 64)
    assert [m for m, _ in calls] == [16, 32, 64] and used.max() == 64
    calls.clear()
    out, used, rounds = X._refine_by_gap(run, cand, n, 16, "midpoint", None, 1024)
    assert [m for m, _ in calls] == [16] and (used == 16).all() and rounds == 1


def test_refusals_before_any_device_work():
    model = types.SimpleNamespace(num_entities=50, num_relations=4)      # no engine: the refusals come first
    tri = np.array([[0, 0, 1]])
    for kw, match in ((dict(top_k=0), "top_k"), (dict(top_k=65), "top_k"), (dict(quadrature="simpson"), "quadrature"),
                      (dict(steps=2048), "steps"), (dict(toward="sideways"), "toward"),
                      (dict(nodes=([0.5], [1.0]), tol=1e-3), "tol"), (dict(nodes=([0.5, 0.6], [1.0])), "nodes"),
                      (dict(steps=64, tol=1e-3, max_steps=32), "max_steps")):
        with pytest.raises(L.IddgcnError, match=match):
            X.integrated_gradients_batched(model, tri, tri, **kw)
    for bad in ([[0, 4, 1]], [[0, -1, 1]]):
        with pytest.raises(L.IddgcnError, match="relation index"):
            X.integrated_gradients_batched(model, tri, np.array(bad))
    host = DeviceAdjacency(get_adj_mats(tri, 50, 4), 50, "cpu")
    with pytest.raises(L.IddgcnError, match="relations"):
        X.counterfactual_candidates(host, tri, relations=[4])
