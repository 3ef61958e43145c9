"""Deletion / insertion curves on the GPU (ops.explain_curves, Engine.edit_curves, explain.fidelity_curves) against the
float64 restatement of tests/ref_fidelity.py (held to oracle.ref_explain.forward_with_values by
tests/test_fidelity_host.py).

Bar (tests/test_gpu_explain_batched.py's for p): a point may deviate from float64 by max(4 x the float32 restatement's
own deviation, 1e-6).  Batch, length and order independence are bitwise."""
import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd import get_IDDGCN_Model
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from oracle import ref_explain
from oracle.ref_model import to_torch_params
from tests import ref_fidelity as RF

pytestmark = pytest.mark.gpu
K = 10
CASES = [(d, R, False) for d in (32, 64) for R in (1, 2, 4, 8)] + [(64, 4, True), (32, 2, True)]
QS = (1, 2, 63, 64, 65, 200)
N_ENT, N_REL = 845, 4
_SMALL = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def small(d, R, saturate, cuda):
    """The small case with its mixed explanations, our curves and both restatements, computed once."""
    key = (d, R, saturate)
    if key not in _SMALL:
        N, tri, params, q = RF.small_case(d, R, saturate)
        host = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
        preds = RF.mixed_explanations(host, q)
        preds[1] = preds[0]                           # the repeated query, explained the same way
        cand = X.curve_steps(host, q, preds)
        assert cand["K"] == K
        model = RF.model_with(params, N, R, d)
        stats = {}
        ours = X.fidelity_curves(model, tri, q, preds, fused=True, stats=stats)
        assert stats["fused"] is True
        _SMALL[key] = dict(N=N, tri=tri, params=params, q=q, host=host, preds=preds, cand=cand, model=model, ours=ours,
                           ref64=RF.curves(params, q, cand, K), ref32=RF.curves(params, q, cand, K, torch.float32))
    return _SMALL[key]


def check_against_restatement(ours, ref64, ref32, what):
    """Every point of both curves within max(4 |p32 - p64|, 1e-6); returns the worst error / bar."""
    worst = 0.0
    for name, o, r64, r32 in (("deletion", ours["deletion"], ref64[0], ref32[0]),
                              ("insertion", ours["insertion"], ref64[1], ref32[1])):
        assert o.shape == r64.shape and o.dtype == np.float32, (what, name)
        err = np.abs(o.astype(np.float64) - r64)
        bar = np.maximum(4 * np.abs(r32 - r64), 1e-6)
        bad = np.argwhere(err > bar)
        assert not len(bad), (what, name, bad[:5].tolist(), err[err > bar][:5], bar[err > bar][:5])
        worst = max(worst, float((err / bar).max()) if err.size else 0.0)
    return worst


# -- 1. oracle parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R,saturate", CASES)
def test_small_against_restatement(d, R, saturate, cuda):
    """200 queries x 22 variants.  The explanations mix effective edges of both rows, column-only edges, non-stored
    edges, a duplicate and short lists; the test is only honest if the steps it checks move the prediction by far more
    than the bar, which it asserts: at least 90 % of the effective steps move p64 by more than 10 x the bar."""
    c = small(d, R, saturate, cuda)
    ours, (d64, i64), (d32, i32) = c["ours"], c["ref64"], c["ref32"]
    eff = c["cand"]["effective"]
    assert np.array_equal(ours["effective"], eff) and 0.3 < eff.mean() < 0.9       # effective and inert steps both
    assert np.array_equal(bits(ours["p"]), bits(ours["deletion"][:, 0]))
    worst = check_against_restatement(ours, c["ref64"], c["ref32"], f"d={d} R={R} saturate={saturate}")
    moved = total = 0
    for c64, c32 in ((d64, d32), (i64, i32)):
        bar = np.maximum(4 * np.abs(c32 - c64), 1e-6)
        bar = np.maximum(bar[:, 1:], bar[:, :-1])
        move = np.abs(np.diff(c64, axis=1))
        moved += int((move[eff] > 10 * bar[eff]).sum())
        total += int(eff.sum())
    print(f"curves d={d} R={R} saturate={saturate}: worst error / bar {worst:.3f}; {moved} of {total} effective steps "
          f"move p64 by more than 10 x the bar ({moved / total:.3f})")
    assert moved >= 0.9 * total
    # (2a) an inert or padded step repeats the previous point, bit for bit
    for name in ("deletion", "insertion"):
        b = bits(ours[name])
        assert np.array_equal(b[:, 1:][~eff], b[:, :-1][~eff]), name
    assert np.array_equal(bits(ours["deletion"][0]), bits(ours["deletion"][1]))     # the repeated query


# -- 2. exactness ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
def test_batch_length_and_order_independence(d, R, cuda):
    """(b) prefixes of the batch and a permuted batch, (c) K = 5 against the first 6 points of K = 10, (d) a permuted
    explanation at j = K, (e) K = 64 with every candidate listed: insertion ends at the unedited prediction, deletion
    at the empty-row prediction.  All bitwise."""
    c = small(d, R, False, cuda)
    model, tri, q, preds, ours = c["model"], c["tri"], c["q"], c["preds"], c["ours"]
    run = lambda qq, pp: X.fidelity_curves(model, tri, qq, pp, fused=True)  # noqa: E731
    for Q in QS[:-1]:
        o = run(q[:Q], preds[:Q])
        for name in ("p", "deletion", "insertion"):
            # a prefix's longest list may be shorter than K: the points it has are the same
            n = o[name].shape[-1] if name != "p" else None
            assert np.array_equal(bits(o[name]), bits(ours[name][:Q] if n is None else ours[name][:Q, :n])), (Q, name)
    perm = np.random.default_rng(1).permutation(len(q))
    o = run(q[perm], [preds[j] for j in perm])
    for name in ("deletion", "insertion"):
        assert np.array_equal(bits(o[name]), bits(ours[name][perm])), name
    o = run(q, [p[:5] for p in preds])                                              # (c)
    for name in ("deletion", "insertion"):
        assert o[name].shape == (len(q), 6) and np.array_equal(bits(o[name]), bits(ours[name][:, :6])), name
    o = run(q, [p[::-1] for p in preds])                                            # (d)
    for name in ("deletion", "insertion"):
        assert np.array_equal(bits(o[name][:, K]), bits(ours[name][:, K])), name
        assert not np.array_equal(bits(o[name][:, 1:K]), bits(ours[name][:, 1:K]))  # the order matters before the end
    cand = c["cand"]                                                                # (e)
    row = np.concatenate(c["host"].rows)
    every = np.full((len(q), L.TOPK_MAX, 3), -1, np.int64)
    deg = np.diff(cand["qptr"])
    assert deg.max() <= 28 and deg.min() == 0
    for j in range(len(q)):
        sl = slice(cand["qptr"][j], cand["qptr"][j + 1])
        every[j, :deg[j]] = np.stack([row[cand["entry"][sl]], cand["rel"][sl], cand["col"][sl]], 1)
    o = run(q, every)
    assert o["deletion"].shape == (len(q), L.TOPK_MAX + 1) and o["effective"].sum() == deg.sum()
    assert np.array_equal(bits(o["insertion"][:, -1]), bits(o["deletion"][:, 0]))
    assert np.array_equal(bits(o["deletion"][:, -1]), bits(o["insertion"][:, 0]))
    assert np.array_equal(bits(o["deletion"][:, 0]), bits(ours["deletion"][:, 0]))
    assert np.array_equal(bits(o["insertion"][:, 0]), bits(ours["insertion"][:, 0]))
    assert (o["deletion"][:, -1] != o["deletion"][:, 0]).sum() > 150                # the curves do go somewhere


# -- 3. large degrees --------------------------------------------------------------------------------------------
def test_large_degrees(cuda):
    """tests/test_gpu_mask_batched.py's graph: N = 320, R = 3 with relation 2 empty, rows of degree 1, 63, 64, 65 and
    300 (twice: relations 0 and 1).  K = 64 random explanations; rows 5's 601 candidates exceed the 320 E rows the
    kernel stages in LDS at D = 64, the others come from global memory."""
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
    assert mats[2].nnz == 1 and mats[2].values[0] == 0
    params = RF.make_params(N, R, D, rng)
    q = np.array([(1, 0, 2), (2, 1, 3), (3, 0, 4), (4, 1, 5), (5, 0, 6), (6, 1, 5), (5, 0, 5), (3, 1, 1)], np.int64)
    host = DeviceAdjacency(mats, N, "cpu")
    preds = X.random_explanations(host, q, L.TOPK_MAX, seed=5)
    cand = X.curve_steps(host, q, preds)
    deg = np.diff(cand["qptr"])
    assert cand["K"] == L.TOPK_MAX and deg.tolist() == [64, 127, 129, 666, 601, 601, 601, 65] and deg.max() > 320
    assert (cand["rel"] < 2).all()                                    # the placeholder is no candidate
    ours = X.fidelity_curves(RF.model_with(params, N, R, D), tri, q, preds, fused=True)
    ref64 = RF.curves(params, q, cand, L.TOPK_MAX)
    ref32 = RF.curves(params, q, cand, L.TOPK_MAX, torch.float32)
    worst = check_against_restatement(ours, ref64, ref32, "large degrees")
    spread = np.abs(ref64[0][:, -1] - ref64[0][:, 0])
    print(f"large degrees: candidates {deg.tolist()}, worst error / bar {worst:.3f}, |del[K] - del[0]| {spread}")
    assert (spread > 1e-3).sum() >= 6


# -- 4. fold 4, bundled weights ------------------------------------------------------------------------------------
def test_fold4(golden, cuda):
    """All 288 test triples with explaiNE's bundled explanations through the fused path; 8 of them against the
    per-variant route and the float64 restatement (itself tied to forward_with_values at four points here)."""
    d, ex, w = golden("fold4_data.npz"), golden("explain_fold4.npz"), golden("weights_fold4.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    test, preds = ex["test_triples"].astype(np.int64), ex["explaine_preds"]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), test])
    mats = get_adj_mats(adjacency, N_ENT, N_REL)
    stats = {}
    ours = X.fidelity_curves(model, adjacency, test, preds, stats=stats)
    assert stats["fused"] is True and ours["deletion"].shape == (288, K + 1)
    p = model.predict(x=[np.arange(N_ENT)[None], test[None, :, 0], test[None, :, 1], test[None, :, 2], mats])[0]
    assert np.abs(ours["p"] - p).max() <= 1e-4
    layered = X.fidelity_curves(model, adjacency, test[:8], preds[:8], fused=False)
    host = DeviceAdjacency(mats, N_ENT, "cpu")
    cand = X.curve_steps(host, test[:8], preds[:8])
    ref64, ref32 = RF.curves(w, test[:8], cand, K), RF.curves(w, test[:8], cand, K, torch.float32)
    for i, name in enumerate(("deletion", "insertion")):
        assert np.abs(ours[name][:8] - layered[name]).max() <= 1e-4, name
        bar = np.maximum(1e-4, 2 * np.abs(ref32[i] - ref64[i]))
        assert (np.abs(ours[name][:8] - ref64[i]) <= bar).all(), name
        assert (np.abs(layered[name] - ref64[i]) <= bar).all(), name
    assert np.array_equal(ours["effective"][:8], layered["effective"])
    coo = [(np.stack([m.rows, m.cols], 1), m.values) for m in mats]
    P = to_torch_params(w, torch.float64, requires_grad=False)
    for j, v in ((0, 0), (3, K), (5, K + 1), (7, 2 * K + 1)):
        vals = [torch.as_tensor(x) for x in RF.edited_values(host, cand, j, v, K)]
        want = float(ref_explain.forward_with_values(P, test[j][None], coo, vals)[0])
        assert abs((ref64[0][j, v] if v <= K else ref64[1][j, v - K - 1]) - want) <= 1e-12
    rnd = X.fidelity_curves(model, adjacency, test, X.random_explanations(host, test, K, seed=0))
    for name, cv in (("explaiNE", ours), ("random", rnd)):
        s = X.fidelity_summary(cv)
        print(f"fold 4 {name}: " + ", ".join(f"{k} {v:.4f}" for k, v in s["mean"].items()) +
              f", effective share {s['effective_share']:.3f}")


# -- 5. outside the envelope -----------------------------------------------------------------------------------------
def test_outside_the_envelope(cuda):
    """D = 128: fused=True raises, fused=None takes the per-variant route and agrees with the restatement (1e-4)."""
    N, tri, _, q = RF.small_case(64, 2)
    params = RF.make_params(N, 2, 128, np.random.default_rng(9))
    host = DeviceAdjacency(get_adj_mats(tri, N, 2), N, "cpu")
    q = q[2:6]                                                        # h == t and the empty rows
    preds = RF.mixed_explanations(host, q)
    model = RF.model_with(params, N, 2, 128)
    with pytest.raises(L.IddgcnError, match="fused=False"):
        X.fidelity_curves(model, tri, q, preds, fused=True)
    stats = {}
    o = X.fidelity_curves(model, tri, q, preds, stats=stats)
    assert stats["fused"] is False
    cand = X.curve_steps(host, q, preds)
    ref = RF.curves(params, q, cand, cand["K"])
    assert np.abs(o["deletion"] - ref[0]).max() <= 1e-4 and np.abs(o["insertion"] - ref[1]).max() <= 1e-4
    assert np.abs(ref[0][:, -1] - ref[0][:, 0]).max() > 1e-3
    model = RF.model_with(RF.make_params(N, 2, 64, np.random.default_rng(9)), N, 2, 64)
    eng = model._device_state()
    eng.features = "bf16"
    with pytest.raises(L.IddgcnError):
        X.fidelity_curves(model, tri, q, preds, fused=True)
    eng.features = "f32"
    for attr in ("node_shard", "spmm_shard", "row_shard"):
        setattr(eng, attr, object())
        with pytest.raises(L.IddgcnError):
            X.fidelity_curves(model, tri, q, preds, fused=True)
        setattr(eng, attr, None)
    for bad in ([[N, 0, 1]], [[0, 2, 1]], [[0, 0, -1]]):
        with pytest.raises(L.IddgcnError):
            X.fidelity_curves(model, tri, np.array(bad), preds[:1])
    e = X.fidelity_curves(model, tri, np.zeros((0, 3), np.int64), np.zeros((0, K, 3), np.int64))
    assert e["deletion"].shape == (0, K + 1) and e["p"].shape == (0,)
