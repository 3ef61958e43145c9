"""Integrated-gradients edge attributions on the GPU (ops.explain_path, Engine.integrated_gradients,
explain.integrated_gradients_batched) against the float64 restatement of tests/ref_integrated_gradients.py (held to
oracle.ref_explain.value_grads by tests/test_integrated_gradients_host.py).

Bars.  attr, per query: max(4 max_j |attr32_j - attr64_j|, 2^-20 max_j |attr64_j|), the two restatements run with the
same rule; tests/test_gpu_fidelity.py's 4 x margin over the float32 restatement's own deviation, taken per query
because the kernel's summation order differs from the restatement's (tests/test_integrated_gradients_host.py shows that
three wrong answers break it).  p_full, p_base: max(4 |p32 - p64|, 1e-6).  total: the sum of its candidates' bars; gap:
that plus the two p bars.  A candidate that is not eligible and a query with empty rows give exactly 0.  Batch and
order independence are bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd import get_IDDGCN_Model, ops
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from tests import ref_fidelity as RF
from tests import ref_integrated_gradients as RI

pytestmark = pytest.mark.gpu
CASES = [(d, R, False) for d in (32, 64) for R in (1, 2, 4, 8)] + [(64, 4, True), (32, 2, True)]
NQ = 40
CHUNK = 32                                   # csrc/explain.hip IG_CHUNK: quadrature nodes per workgroup
GAUSS32 = X.quadrature_rule(32, "gauss")
N_ENT, N_REL = 845, 4
_SMALL = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_engine(model, mats, q, cand, alpha, omega, **kw):
    """Engine.integrated_gradients' outputs as host arrays."""
    eng = model._device_state()
    dadj = DeviceAdjacency(mats, model.num_entities, eng.device)
    out = eng.integrated_gradients(model._params, dadj, q, cand, alpha, omega, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def small(d, R, saturate, cuda):
    """The small case: its 200 queries' candidates, the model, and for the first 40 queries with Gauss-32 our outputs
    and both restatements, computed once."""
    key = (d, R, saturate)
    if key not in _SMALL:
        N, tri, params, q = RF.small_case(d, R, saturate)
        mats = get_adj_mats(tri, N, R)
        host = DeviceAdjacency(mats, N, "cpu")
        cand = X.counterfactual_candidates(host, q)
        cand40 = X.counterfactual_candidates(host, q[:NQ])
        model = RF.model_with(params, N, R, d)
        _SMALL[key] = dict(N=N, tri=tri, mats=mats, params=params, q=q, host=host, cand=cand, cand40=cand40,
                           model=model, ours=run_engine(model, mats, q[:NQ], cand40, *GAUSS32),
                           ref64=RI.integrate(params, q[:NQ], cand40, *GAUSS32),
                           ref32=RI.integrate(params, q[:NQ], cand40, *GAUSS32, dtype=torch.float32))
    return _SMALL[key]


def check_against_restatement(ours, ref64, ref32, cand, what):
    """attr, p_full, p_base, total and gap within the bars of the module docstring; exact zeros where they are due.
    Returns the worst error / bar over attr."""
    qp = np.asarray(cand["qptr"], np.int64)
    lens = np.diff(qp)
    q_of = np.repeat(np.arange(len(lens)), lens)
    bar, bar_full, bar_base = RI.attr_bar(ref64, ref32, qp)
    assert ours["attr"].dtype == np.float32 and ours["attr"].shape == ref64["attr"].shape, what
    err = np.abs(ours["attr"].astype(np.float64) - ref64["attr"])
    bad = np.flatnonzero(err > bar[q_of])
    worst = float((err / np.maximum(bar[q_of], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: attr worst error / bar {worst:.3f} (bars {bar[lens > 0].min():.2e} .. {bar.max():.2e}, "
          f"max |attr64| {np.abs(ref64['attr']).max():.2e})")
    assert not len(bad), (what, "attr", bad[:5].tolist(), err[bad[:5]], bar[q_of][bad[:5]])
    for name, b in (("p_full", bar_full), ("p_base", bar_base), ("total", bar * lens),
                    ("gap", bar * lens + bar_full + bar_base)):
        e = np.abs(ours[name].astype(np.float64) - ref64[name])
        print(f"{what}: {name} worst error / bar {float((e / np.maximum(b, 1e-300)).max()):.3f}")
        assert (e <= b).all(), (what, name, np.flatnonzero(e > b)[:5].tolist(), e[e > b][:5], b[e > b][:5])
    assert (bits(ours["attr"])[~np.asarray(cand["eligible"], bool)] == 0).all(), what
    empty = lens == 0
    assert (bits(ours["total"])[empty] == 0).all() and (ours["gap"][empty] == 0).all(), what
    assert np.array_equal(bits(ours["p_full"])[empty], bits(ours["p_base"])[empty]), what
    return worst


# -- 1. float64 parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R,saturate", CASES)
def test_small_against_restatement(d, R, saturate, cuda):
    """40 queries (the repeated one, h == t and the three with empty rows among them), Gauss-Legendre, 32 nodes."""
    c = small(d, R, saturate, cuda)
    q, cand = c["q"][:NQ], c["cand40"]
    lens = np.diff(cand["qptr"])
    assert (q[1] == q[0]).all() and q[2, 0] == q[2, 2] and (lens[3:6] < lens.max()).all() and lens[5] == 0
    assert (lens == 0).sum() >= 1 and lens.max() > 8
    check_against_restatement(c["ours"], c["ref64"], c["ref32"], cand, f"d={d} R={R} saturate={saturate}")
    print(f"  max |gap| ours {np.abs(c['ours']['gap']).max():.2e}, float64 {np.abs(c['ref64']['gap']).max():.2e}, "
          f"mean |p - p_base| {np.abs(c['ref64']['p_full'] - c['ref64']['p_base']).mean():.2e}")
    assert np.abs(c["ref64"]["p_full"] - c["ref64"]["p_base"]).mean() > 1e-4        # the attributions do carry something


# -- 2. an arbitrary rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
@pytest.mark.parametrize("m", [5, CHUNK + 5])
def test_arbitrary_rule(d, R, m, cuda):
    """Random nodes in [0, 1] and random weights that do not sum to 1 (both fp32 values): m = 5, and one chunk plus 5
    so that the second chunk is ragged.  Any mix-up of nodes, weights or chunks shows here."""
    c = small(d, R, False, cuda)
    rng = np.random.default_rng(m)
    alpha = rng.random(m).astype(np.float32).astype(np.float64)
    omega = rng.uniform(0.1, 2.0, m).astype(np.float32).astype(np.float64)
    assert abs(omega.sum() - 1) > 0.5
    q, cand = c["q"][:NQ], c["cand40"]
    ours = run_engine(c["model"], c["mats"], q, cand, alpha, omega)
    ref64 = RI.integrate(c["params"], q, cand, alpha, omega)
    ref32 = RI.integrate(c["params"], q, cand, alpha, omega, dtype=torch.float32)
    check_against_restatement(ours, ref64, ref32, cand, f"random rule m={m} d={d} R={R}")


@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
def test_one_node_is_explaine(d, R, cuda):
    """m = 1, alpha = 1, omega = 1: attr_j = val_j x explaiNE's gradient (Engine.value_grads_batch), within the bar of
    that rule."""
    c = small(d, R, False, cuda)
    q, cand, model = c["q"][:NQ], c["cand40"], c["model"]
    ours = run_engine(model, c["mats"], q, cand, [1.0], [1.0])
    eng = model._device_state()
    vg = eng.value_grads_batch(model._params, DeviceAdjacency(c["mats"], c["N"], eng.device), q)
    vq, ve, vgrad = (vg[k].cpu().numpy() for k in ("qptr", "entry", "grad"))
    ref64 = RI.integrate(c["params"], q, cand, [1.0], [1.0])
    ref32 = RI.integrate(c["params"], q, cand, [1.0], [1.0], dtype=torch.float32)
    bar = RI.attr_bar(ref64, ref32, cand["qptr"])[0]
    worst = 0.0
    for j in range(NQ):
        a, b = cand["qptr"][j], cand["qptr"][j + 1]
        e, g = ve[vq[j]:vq[j + 1]], vgrad[vq[j]:vq[j + 1]]
        o = np.argsort(e, kind="stable")
        assert np.array_equal(e[o], cand["entry"][a:b])
        err = np.abs(ours["attr"][a:b].astype(np.float64) - cand["val"][a:b].astype(np.float64) * g[o])
        worst = max(worst, float((err / bar[j]).max()) if b > a else 0.0)
    print(f"m = 1 against value_grads_batch d={d} R={R}: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    assert np.abs(ours["p_full"] - vg["p"].cpu().numpy()).max() <= 1e-6


# -- 3. eligibility ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 2)])
def test_eligibility(d, R, cuda):
    """The graph stores every query's own edge in both directions; exclude_target=True and relations=[0]: the target
    edges and the other relations stay in the graph along the path and get exactly 0."""
    c = small(d, R, False, cuda)
    q = c["q"][:NQ]
    tri = np.concatenate([c["tri"], q, q[:, ::-1]])
    mats = get_adj_mats(tri, c["N"], R)
    host = DeviceAdjacency(mats, c["N"], "cpu")
    cand = X.counterfactual_candidates(host, q, exclude_target=True, relations=[0])
    el = cand["eligible"]
    assert 0.1 < el.mean() < 0.9 and (~el & (cand["rel"] == 0)).sum() >= 10        # target edges of relation 0
    ours = run_engine(c["model"], mats, q, cand, *GAUSS32)
    ref64 = RI.integrate(c["params"], q, cand, *GAUSS32)
    ref32 = RI.integrate(c["params"], q, cand, *GAUSS32, dtype=torch.float32)
    check_against_restatement(ours, ref64, ref32, cand, f"eligibility d={d} R={R}")
    res = X.integrated_gradients_batched(c["model"], tri, q, 5, steps=32, exclude_target=True, relations=[0],
                                         fused=True, return_attributions=True)
    table = np.concatenate(res["attributions"][1])
    assert np.isnan(table[~el]).all() and np.array_equal(bits(table[el]), bits(ours["attr"][el]))
    assert all((e[:, 1] == 0).all() for e in res["edges"]) and (res["relation_attribution"][:, 1:] == 0).all()
    assert np.abs(res["relation_attribution"].sum(1) - res["total"]).max() <= 1e-6


# -- 4. long rows ------------------------------------------------------------------------------------------------
def test_long_rows(cuda):
    """tests/test_gpu_fidelity.py's large-degree graph: N = 320, R = 3 with relation 2 empty, rows of degree 1, 63, 64,
    65 and 300 (twice); up to 666 candidates per query, more than 512 and more than any staging buffer of the
    explainer kernels holds."""
    rng = np.random.default_rng(3)
    N, R, D = 320, 3, 64
    rows = []
    for node, deg in ((1, 1), (2, 63), (3, 64), (4, 65)):
        cols = np.sort(rng.choice(np.arange(7, N), deg, replace=False))
        rows.append(np.stack([np.full(deg, node), np.zeros(deg, np.int64), cols], 1))
    for r in (0, 1):
        rows.append(np.stack([np.full(300, 5), np.full(300, r), np.arange(10, 310)], 1))
        rows.append(np.stack([np.arange(10, 300), np.full(290, r), np.full(290, 6)], 1))
    rows.append(np.array([[0, 0, 9], [0, 1, 5], [8, 1, 0], [5, 0, 5]]))
    tri = np.concatenate(rows).astype(np.int64)
    mats = get_adj_mats(tri, N, R)
    params = RF.make_params(N, R, D, rng)
    q = np.array([(1, 0, 2), (2, 1, 3), (3, 0, 4), (4, 1, 5), (5, 0, 6), (6, 1, 5), (5, 0, 5), (3, 1, 1)], np.int64)
    cand = X.counterfactual_candidates(DeviceAdjacency(mats, N, "cpu"), q)
    deg = np.diff(cand["qptr"])
    assert deg.tolist() == [64, 127, 129, 666, 601, 601, 601, 65] and (cand["rel"] < 2).all()
    ours = run_engine(RF.model_with(params, N, R, D), mats, q, cand, *GAUSS32)
    ref64 = RI.integrate(params, q, cand, *GAUSS32)
    ref32 = RI.integrate(params, q, cand, *GAUSS32, dtype=torch.float32)
    check_against_restatement(ours, ref64, ref32, cand, "long rows")
    assert (np.abs(ref64["p_full"] - ref64["p_base"]) > 1e-3).sum() >= 6


# -- 5. repeatability --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
def test_batch_and_order_independence(d, R, cuda):
    """All 200 queries at once, 40 at a time, in reversed order, and one call twice: bitwise equal per query; the
    repeated query equals its twin.  The rule is one chunk plus 5 nodes, so two workgroups share every query."""
    c = small(d, R, False, cuda)
    model, mats, q, cand, host = c["model"], c["mats"], c["q"], c["cand"], c["host"]
    rule = X.quadrature_rule(CHUNK + 5, "gauss")
    full = run_engine(model, mats, q, cand, *rule)
    again = run_engine(model, mats, q, cand, *rule)
    qp = cand["qptr"]
    names = ("total", "p_full", "p_base", "gap")
    for nm in names + ("attr",):
        assert np.array_equal(bits(full[nm]), bits(again[nm])), nm
    assert np.array_equal(bits(full["attr"][qp[0]:qp[1]]), bits(full["attr"][qp[1]:qp[2]]))
    assert all(bits(full[nm])[0] == bits(full[nm])[1] for nm in names)
    for a in range(0, len(q), NQ):
        part = run_engine(model, mats, q[a:a + NQ], X.counterfactual_candidates(host, q[a:a + NQ]), *rule)
        for nm in names:
            assert np.array_equal(bits(part[nm]), bits(full[nm][a:a + NQ])), (a, nm)
        assert np.array_equal(bits(part["attr"]), bits(full["attr"][qp[a]:qp[a + NQ]])), a
    rev = run_engine(model, mats, q[::-1], X.counterfactual_candidates(host, q[::-1]), *rule)
    for nm in names:
        assert np.array_equal(bits(rev[nm]), bits(full[nm][::-1])), nm
    segs = [full["attr"][qp[j]:qp[j + 1]] for j in range(len(q))][::-1]
    assert np.array_equal(bits(rev["attr"]), bits(np.concatenate(segs)))
    # chunks of queries inside one call (max_entries) change nothing either
    parts = run_engine(model, mats, q, cand, *rule, max_entries=300)
    for nm in names + ("attr",):
        assert np.array_equal(bits(parts[nm]), bits(full[nm])), nm
    assert np.abs(full["attr"]).max() > 0


# -- 6. routes ---------------------------------------------------------------------------------------------------
def test_routes(cuda):
    """fused=False (one set_values + value_grads per (triple, node)) on 8 queries within the fused route's bars;
    D = 128: fused=True raises, fused=None takes the per-node route."""
    c = small(64, 4, False, cuda)
    q = c["q"][:8]
    cand = X.counterfactual_candidates(c["host"], q)
    kw = dict(steps=32, return_attributions=True)
    stats = {}
    fused = X.integrated_gradients_batched(c["model"], c["tri"], q, 10, fused=True, stats=stats, **kw)
    assert stats["fused"] is True and stats["rounds"] == 1 and "launch_events" in stats
    layered = X.integrated_gradients_batched(c["model"], c["tri"], q, 10, fused=False, stats=stats, **kw)
    assert stats["fused"] is False
    ref64 = RI.integrate(c["params"], q, cand, *GAUSS32)
    ref32 = RI.integrate(c["params"], q, cand, *GAUSS32, dtype=torch.float32)
    for name, res in (("fused", fused), ("per-node", layered)):
        ours = dict(attr=np.nan_to_num(np.concatenate(res["attributions"][1])), total=res["total"], gap=res["gap"],
                    p_full=res["p"], p_base=res["p_baseline"])
        check_against_restatement(ours, ref64, ref32, cand, f"route {name}")
        assert (res["steps_used"] == 32).all() and len(res["edges"]) == 8
    for a, b in zip(fused["edges"], layered["edges"]):
        assert a.shape == b.shape
    N, tri = c["N"], c["tri"]
    model = RF.model_with(RF.make_params(N, 2, 128, np.random.default_rng(9)), N, 2, 128)
    tri2 = tri[tri[:, 1] < 2]
    q2 = np.array([(7, 0, 7), (5, 0, 49), (3, 1, 8)], np.int64)
    with pytest.raises(L.IddgcnError, match="fused=False"):
        X.integrated_gradients_batched(model, tri2, q2, fused=True)
    stats = {}
    o = X.integrated_gradients_batched(model, tri2, q2, 3, steps=4, stats=stats)
    assert stats["fused"] is False
    cand2 = X.counterfactual_candidates(DeviceAdjacency(get_adj_mats(tri2, N, 2), N, "cpu"), q2)
    ref = RI.integrate(RF.make_params(N, 2, 128, np.random.default_rng(9)), q2, cand2, *X.quadrature_rule(4))
    assert np.abs(o["total"] - ref["total"]).max() <= 1e-4 and np.abs(o["gap"] - ref["gap"]).max() <= 1e-4
    assert np.abs(ref["total"]).max() > 1e-3


# -- 7. fold 4, bundled weights ----------------------------------------------------------------------------------
def test_fold4(golden, cuda):
    """16 test triples, Gauss-Legendre with 256 nodes, saturated weights: per-element bar max(1e-4, 2 |x32 - x64|) as
    tests/test_gpu_fidelity.py::test_fold4; the kernel's |gap| within |gap64| plus the bars' sum; the top-10 lists go
    through fidelity_curves."""
    d, ex, w = golden("fold4_data.npz"), golden("explain_fold4.npz"), golden("weights_fold4.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    test = ex["test_triples"].astype(np.int64)[:16]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"].astype(np.int64)])
    mats = get_adj_mats(adjacency, N_ENT, N_REL)
    cand = X.counterfactual_candidates(DeviceAdjacency(mats, N_ENT, "cpu"), test)
    stats = {}
    res = X.integrated_gradients_batched(model, adjacency, test, 10, steps=256, stats=stats, return_attributions=True)
    assert stats["fused"] is True and (res["steps_used"] == 256).all()
    rule = X.quadrature_rule(256)
    ref64, ref32 = RI.integrate(w, test, cand, *rule), RI.integrate(w, test, cand, *rule, dtype=torch.float32)
    attr = np.concatenate(res["attributions"][1]).astype(np.float64)
    bar = np.maximum(1e-4, 2 * np.abs(ref32["attr"] - ref64["attr"]))
    err = np.abs(attr - ref64["attr"])
    print(f"fold 4: attr worst error / bar {(err / bar).max():.3f}, max |attr64| {np.abs(ref64['attr']).max():.3f}")
    assert (err <= bar).all()
    pbar = sum(np.maximum(1e-4, 2 * np.abs(ref32[k] - ref64[k])) for k in ("p_full", "p_base"))
    q_of = np.repeat(np.arange(16), np.diff(cand["qptr"]))
    gbar = np.bincount(q_of, bar, 16) + pbar
    print(f"fold 4: |gap| ours {np.abs(res['gap']).max():.2e}, float64 {np.abs(ref64['gap']).max():.2e}, float32 "
          f"{np.abs(ref32['gap']).max():.2e}; mean |p - p_base| {np.abs(res['p'] - res['p_baseline']).mean():.3f}")
    assert (np.abs(res["gap"]) <= np.abs(ref64["gap"]) + gbar).all()
    assert np.abs(res["p"] - ref64["p_full"]).max() <= 1e-4 and np.abs(res["p_baseline"] - ref64["p_base"]).max() <= 1e-4
    curves = X.fidelity_curves(model, adjacency, test, res["edges"])
    s = X.fidelity_summary(curves)
    print("fold 4 integrated gradients top 10: deletion drop (fidelity_plus) " + f"{s['mean']['fidelity_plus']:.4f}, " +
          ", ".join(f"{k} {v:.4f}" for k, v in s["mean"].items()))
    assert curves["deletion"].shape == (16, 11) and np.abs(curves["p"] - res["p"]).max() <= 1e-4


# -- 8. refusals -------------------------------------------------------------------------------------------------
def _args(cuda, N=8, R=2, D=32, m=4):
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=cuda)           # noqa: E731
    ints = lambda vals, dtype=torch.int32: torch.tensor(vals, dtype=dtype, device=cuda)             # noqa: E731
    return dict(E=z(N, D), K=[z(R, D, D) for _ in range(3)], S=[z(D, D) for _ in range(3)],
                Wa=[z(D, R) for _ in range(3)], ba=[z(R) for _ in range(3)], rel=z(R, D), h=ints([0, 1]),
                r=ints([0, 1]), t=ints([2, 3]), qptr=ints([0, 2, 5], torch.int64), crel=ints([0, 1, 0, 1, 1]),
                ccol=ints([1, 2, 3, 4, 5]), crole=ints([1, 1, 2, 3, 1]), celig=ints([1, 0, 1, 1, 1]), cval=z(5),
                alpha=z(m), omega=z(m))


def test_ops_refusals(cuda):
    """ops.explain_path refuses before anything is launched; a good call of the same arguments goes through."""
    good = _args(cuda)
    out = ops.explain_path(**good)
    torch.cuda.synchronize()
    assert out["attr"].shape == (5,) and (out["attr"] == 0).all() and (out["gap"] == 0).all()
    misaligned = torch.zeros(8 * 32 + 1, device=cuda)[1:].view(8, 32)
    none_layer = [good["S"][0], None, good["S"][2]]
    for kw, match in ((dict(E=misaligned), "16-byte aligned"), (dict(S=none_layer), "every layer's K, S, Wa, ba"),
                      (dict(alpha=good["alpha"][:0], omega=good["omega"][:0]), "m in"),
                      (dict(alpha=torch.zeros(1025, device=cuda), omega=torch.zeros(1025, device=cuda)), "m in"),
                      (dict(omega=good["omega"][:3].contiguous()), "omega: expected shape"),
                      (dict(celig=good["celig"].long()), "celig: expected"),
                      (dict(scratch=torch.zeros(8, device=cuda)), "scratch holds"),
                      (dict(gap=torch.zeros(3, device=cuda)), "gap: expected shape")):
        with pytest.raises(L.IddgcnError, match=match):
            ops.explain_path(**{**good, **kw})
    with pytest.raises(L.IddgcnError, match="feature width"):
        ops.explain_path(**_args(cuda, D=48))
    with pytest.raises(L.IddgcnError, match="relation count"):
        ops.explain_path(**_args(cuda, R=9))


def test_entry_refusals(cuda):
    """The C entry itself: a misaligned E, a null layer pointer, m = 0, m > 1024 (IDDGCN_E_BAD_ARG), d = 48
    (IDDGCN_E_BAD_DIM), R = 9 (IDDGCN_E_BAD_REL); Q = 0 launches nothing and succeeds whatever the pointers."""
    g = _args(cuda)
    keep = dict(out=[torch.zeros(8, device=cuda) for _ in range(5)], scratch=torch.zeros(4096, device=cuda),
                KT=[x.clone() for x in g["K"]], ST=[x.clone() for x in g["S"]])

    def call(**edit):
        a = L.ExplainPathArgs()
        a.N, a.d, a.R, a.Q, a.m = 8, 32, 2, 2, 4
        attr, total, p_full, p_base, gap = keep["out"]
        ops._set_ptrs(a, **g, KT=keep["KT"], ST=keep["ST"], attr=attr, total=total, p_full=p_full, p_base=p_base,
                      gap=gap, scratch=keep["scratch"])
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return L.lib().iddgcn_explain_path_f32(None, ctypes.byref(a))

    assert call() == 0
    assert call(E=g["E"].data_ptr() + 4) == -3
    for field in ("K", "KT", "S", "ST", "Wa", "ba"):
        assert call(**{field: (1, None)}) == -3, field
    assert call(m=0) == -3 and call(m=1025) == -3 and call(m=1024 + 1) == -3
    assert call(d=48) == -1 and call(R=9) == -2 and call(R=0) == -2
    assert call(alpha=None) == -3 and call(gap=None) == -3 and call(scratch=None) == -3 and call(Q=-1) == -3
    assert call(Q=0, h=None, scratch=None) == 0
    torch.cuda.synchronize()
    lib = L.lib()
    assert lib.iddgcn_explain_path_scratch_floats(2, 4, 32, 2) == 2 * 1 * 6 * 2 * 32
    assert lib.iddgcn_explain_path_scratch_floats(3, 33, 64, 8) == 3 * 2 * 6 * 8 * 64
    assert lib.iddgcn_explain_path_scratch_floats(3, 1025, 64, 8) == 0
