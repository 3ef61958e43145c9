"""Host side of the fidelity curves (no GPU): the torch restatement against the explainer oracle, the candidate steps,
the summary, the random baseline and the C entry's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import iddgcn_amd
from iddgcn_amd import _lib
from iddgcn_amd import explain as X
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from oracle import ref_explain
from oracle.ref_model import to_torch_params
from tests import ref_fidelity as RF

CURVES = "iddgcn_explain_curves_f32"


def test_helper_equals_forward_with_values():
    """About 40 (query, variant) pairs of the small case, h == t and the empty rows among them: the vectorised helper
    and forward_with_values on the edited full COO agree to 1e-12 in float64."""
    N, tri, params, q = RF.small_case(32, 3)
    mats = get_adj_mats(tri, N, 3)
    dadj = DeviceAdjacency(mats, N, "cpu")
    q = q[:12]
    cand = X.curve_steps(dadj, q, RF.mixed_explanations(dadj, q))
    K = cand["K"]
    assert K == 10
    dele, ins = RF.curves(params, q, cand, K)
    coo = [(np.stack([m.rows, m.cols], 1), m.values) for m in mats]
    P = to_torch_params(params, torch.float64, requires_grad=False)
    rng = np.random.default_rng(0)
    pairs = [(j, v) for j in (2, 3, 4, 5) for v in (0, K, K + 1, 2 * K + 1)]
    pairs += [(int(j), int(v)) for j, v in zip(rng.integers(0, 12, 24), rng.integers(0, 2 * K + 2, 24))]
    moved = 0
    for j, v in pairs:
        vals = [torch.as_tensor(x) for x in RF.edited_values(dadj, cand, j, v, K)]
        want = float(ref_explain.forward_with_values(P, q[j][None], coo, vals)[0])
        got = dele[j, v] if v <= K else ins[j, v - K - 1]
        assert abs(got - want) <= 1e-12, (j, v, got, want)
        moved += abs(got - dele[j, 0]) > 1e-6
    assert moved > 10                                   # the edits are seen by both sides
    assert dele[3, 0] != dele[3, K] and dele[5, 0] == dele[5, K] == ins[5, 0]     # (49, 0, 49): nothing to edit


def _graph():
    """N = 12, R = 2.  Row 3: (3,0,1) (3,0,4) (3,1,4) (3,1,3); row 4: (4,0,3) (4,0,9); others: (1,0,3) (9,1,4) (7,0,7)
    (5,1,6)."""
    tri = np.array([(3, 0, 1), (3, 0, 4), (3, 1, 4), (3, 1, 3), (4, 0, 3), (4, 0, 9), (1, 0, 3), (9, 1, 4), (7, 0, 7),
                    (5, 1, 6)], np.int64)
    return tri, DeviceAdjacency(get_adj_mats(tri, 12, 2), 12, "cpu")


def _steps(dadj, c, q):
    """{(row, rel, col): step} of query q's candidates."""
    row = np.concatenate(dadj.rows)
    sl = slice(c["qptr"][q], c["qptr"][q + 1])
    return {(int(row[e]), int(r), int(cl)): int(s) for e, r, cl, s in zip(c["entry"][sl], c["rel"][sl], c["col"][sl],
                                                                          c["step"][sl])}


def test_curve_steps_rules():
    tri, dadj = _graph()
    q = np.array([(3, 0, 4), (3, 1, 3), (7, 0, 7), (11, 0, 5)], np.int64)
    preds = [np.array([(4, 0, 9),       # a row-t entry
                       (1, 0, 3),       # stored, but only its column is h: inert
                       (3, 1, 4),       # a row-h entry
                       (2, 0, 2),       # not stored: inert
                       (4, 0, 9),       # a duplicate: inert
                       (3, 0, 1)]),
             np.array([(3, 1, 3), (3, 0, 4)]),            # a short list; h == t
             np.array([(7, 0, 7)]),
             np.zeros((0, 3), np.int64)]                  # no edge at all: padding only
    c = X.curve_steps(dadj, q, preds)
    assert c["K"] == 6 and c["qptr"].dtype == np.int64 and c["qptr"].tolist() == [0, 6, 10, 11, 12]
    assert all(c[k].dtype == np.int32 for k in ("entry", "rel", "col", "role", "step")) and c["val"].dtype == np.float32
    assert (c["val"] == 1).all()
    # the candidates are mask_candidates' with role != 0, in its order
    qptr, entry, crel, ccol, crole = X.mask_candidates(dadj, q)
    keep = crole != 0
    assert np.array_equal(c["entry"], entry[keep]) and np.array_equal(c["role"], crole[keep])
    assert np.array_equal(c["rel"], crel[keep]) and np.array_equal(c["col"], ccol[keep])
    assert _steps(dadj, c, 0) == {(3, 0, 1): 5, (3, 0, 4): -1, (4, 0, 3): -1, (4, 0, 9): 0, (3, 1, 3): -1, (3, 1, 4): 2}
    assert c["effective"][0].tolist() == [True, False, True, False, False, True]
    sl = slice(c["qptr"][1], c["qptr"][2])
    assert (c["role"][sl] == X.ROLE_HEAD | X.ROLE_TAIL).all()                 # h == t: both bits
    assert _steps(dadj, c, 1) == {(3, 0, 1): -1, (3, 0, 4): 1, (3, 1, 3): 0, (3, 1, 4): -1}
    assert c["effective"][1].tolist() == [True, True, False, False, False, False]
    assert _steps(dadj, c, 2) == {(7, 0, 7): 0}
    # (11, 0, 5): row 5 holds (5, 1, 6), the list is empty
    assert _steps(dadj, c, 3) == {(5, 1, 6): -1} and not c["effective"][3].any()
    # the same lists as one padded array
    arr = np.full((4, 6, 3), -1, np.int64)
    for j, p in enumerate(preds):
        arr[j, :len(p)] = p
    c2 = X.curve_steps(dadj, q, arr)
    assert all(np.array_equal(c[k], c2[k]) for k in ("qptr", "entry", "step", "effective"))
    for bad in ([np.zeros((65, 3), np.int64)] * 4, preds[:3], np.zeros((4, 0, 3), np.int64)):
        with pytest.raises(X.IddgcnError):
            X.curve_steps(dadj, q, bad)


def test_curve_steps_undirected():
    """(3, 0, 4) and (4, 0, 3) are both stored: one undirected edge flips both at its step; an orientation that an
    earlier edge already flipped keeps the earlier step."""
    tri, dadj = _graph()
    q = np.array([(3, 0, 4)], np.int64)
    preds = [np.array([(4, 0, 3), (9, 0, 4), (3, 0, 4)])]
    c = X.curve_steps(dadj, q, preds)
    s = _steps(dadj, c, 0)
    assert s[(4, 0, 3)] == 0 and s[(3, 0, 4)] == 2 and s[(4, 0, 9)] == -1
    assert c["effective"][0].tolist() == [True, False, True]
    c = X.curve_steps(dadj, q, preds, undirected=True)
    s = _steps(dadj, c, 0)
    assert s[(4, 0, 3)] == 0 and s[(3, 0, 4)] == 0 and s[(4, 0, 9)] == 1      # (9, 0, 4) read as (4, 0, 9)
    assert c["effective"][0].tolist() == [True, True, False]


def test_fidelity_summary_by_hand():
    curves = dict(p=np.array([0.8, 0.5], np.float32),
                  deletion=np.array([[0.8, 0.6, 0.2], [0.5, 0.5, 0.5]], np.float32),
                  insertion=np.array([[0.1, 0.5, 0.7], [0.3, 0.3, 0.5]], np.float32),
                  effective=np.array([[True, True], [False, True]]))
    s = X.fidelity_summary(curves)
    np.testing.assert_allclose(s["fidelity_plus"], [0.6, 0.0], atol=1e-7)
    np.testing.assert_allclose(s["fidelity_minus"], [0.1, 0.0], atol=1e-7)
    np.testing.assert_allclose(s["deletion_auc"], [(0.8 + 2 * 0.6 + 0.2) / 4, 0.5], atol=1e-7)
    np.testing.assert_allclose(s["insertion_auc"], [(0.1 + 2 * 0.5 + 0.7) / 4, (0.3 + 2 * 0.3 + 0.5) / 4], atol=1e-7)
    assert s["effective_share"] == 0.75
    assert abs(s["mean"]["fidelity_plus"] - 0.3) < 1e-7 and abs(s["mean"]["fidelity_minus"] - 0.05) < 1e-7
    assert set(s["mean"]) == {"fidelity_plus", "fidelity_minus", "deletion_auc", "insertion_auc"}
    with pytest.raises(ValueError):
        X.fidelity_summary(dict(curves, deletion=curves["deletion"][:, :1], insertion=curves["insertion"][:, :1]))


def test_random_explanations():
    N, tri, _, q = RF.small_case(32, 3)
    dadj = DeviceAdjacency(get_adj_mats(tri, N, 3), N, "cpu")
    a, b, c = (X.random_explanations(dadj, q, 5, seed) for seed in (1, 1, 2))
    stored = set(map(tuple, tri))
    deg = np.bincount(np.unique(tri, axis=0)[:, 0], minlength=N)
    differs = False
    for j, (h, _, t) in enumerate(q):
        assert a[j].dtype == np.int64 and np.array_equal(a[j], b[j])                  # seeded
        differs |= not np.array_equal(a[j], c[j])
        assert len(a[j]) == min(5, deg[h] + (deg[t] if t != h else 0))
        assert len(set(map(tuple, a[j]))) == len(a[j])                                # distinct
        assert all(tuple(e) in stored and e[0] in (h, t) for e in a[j])               # inside the candidate rows
    assert differs and len(a[5]) == 0                                                 # (49, 0, 49)
    eff = X.curve_steps(dadj, q, [x if len(x) else np.array([(0, 0, 0)]) for x in a])["effective"]
    assert all(eff[j, :len(a[j])].all() for j in range(len(q)) if len(a[j]))


def test_public_names():
    for name in ("fidelity_curves", "fidelity_summary", "random_explanations"):
        assert getattr(iddgcn_amd, name) is getattr(X, name)


def _args(d=64, R=2, k=10, Q=1, N=10, ptr=None):
    a = _lib.ExplainCurvesArgs()
    a.N, a.d, a.R, a.k, a.Q = N, d, R, k, Q
    for f, _ in _lib.ExplainCurvesArgs._fields_[5:]:
        if f in ("K", "S", "Wa", "ba"):
            setattr(a, f, (ctypes.c_void_p * 3)(ptr, ptr, ptr))
        else:
            setattr(a, f, ptr)
    return a


def test_symbol_and_rejections_before_launch():
    """Null stream, null or stand-in pointers: every return below happens on the host, before any launch."""
    lib = _lib.load()
    assert CURVES in _lib.SIGNATURES and hasattr(lib, CURVES)
    assert lib.iddgcn_abi_version() == _lib.ABI_VERSION == 13              # added symbol only
    call = lambda **kw: lib.iddgcn_explain_curves_f32(None, ctypes.byref(_args(**kw)))  # noqa: E731
    ok = 4096                                                              # a stand-in address, never read
    for d in (16, 48, 128):
        assert call(d=d, ptr=ok) == -1
    for R in (0, 9):
        assert call(R=R, ptr=ok) == -2
    assert call(d=16, R=9, k=0) == -1 and call(R=9, k=0) == -2             # BAD_DIM before BAD_REL before BAD_ARG
    for k in (0, _lib.TOPK_MAX + 1):
        assert call(k=k, ptr=ok) == -3
    assert call(Q=-1, ptr=ok) == -3 and call(N=0, ptr=ok) == -3
    assert call(Q=0) == 0 and call(Q=0, k=_lib.TOPK_MAX) == 0              # nothing to do, nothing read
    assert call() == -3                                                    # null pointers
    assert lib.iddgcn_explain_curves_f32(None, None) == -3
    a = _args(ptr=ok)
    a.E = ok + 4                                                           # a misaligned E
    assert lib.iddgcn_explain_curves_f32(None, ctypes.byref(a)) == -3
    a = _args(ptr=ok)
    a.S[1] = None
    assert lib.iddgcn_explain_curves_f32(None, ctypes.byref(a)) == -3
