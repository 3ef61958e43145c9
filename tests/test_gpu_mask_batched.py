"""Batched mask explainers on the GPU (ops.mask_explain, explain.mask_explainer_batched) against the float64 explainer
oracle (oracle/ref_explain.mask_explainer: dense masks, one shared Adam).

Bar (tests/test_gpu_explain.py's): final masked values within 1e-5 absolute of the oracle, top-k scores within 1e-5 and
triples identical where the oracle's scores are separated by more than that.  Two fp32 paths that are each within the
bar of the oracle are within 2e-5 of each other.  The schedule and run-to-run properties are bitwise.  Adam's first
steps say little about the size of a gradient: the kernel's gradient itself is held to the float64 autograd in
tests/test_gpu_mask_grads.py."""
import numpy as np
import pytest

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd import get_IDDGCN_Model
from iddgcn_amd.graph import get_adj_mats
from oracle import ref_explain
from tests import ref_fidelity as RF
from tests.test_mask_batched_host import EMPTY, N_ENT, N_REL, fold4_case, make_params, synthetic_case

pytestmark = pytest.mark.gpu
BAR = 1e-5
KINDS = ("gnnexplainer", "iddgcn")


def _check_topk(our_p, our_s, ref_p, ref_s, tol):
    """tests/test_gpu_explain.py's rule."""
    np.testing.assert_allclose(np.sort(our_s)[::-1], np.sort(ref_s)[::-1], rtol=0, atol=tol)
    sep = np.ones(len(ref_s), bool)
    gaps = np.abs(np.diff(ref_s)) > tol
    sep[:-1] &= gaps
    sep[1:] &= gaps
    assert np.array_equal(our_p[sep], ref_p[sep])


def kind_kw(kind, R):
    if kind == "gnnexplainer":
        return dict(num_epochs=5, threshold=0.2)
    ratios = np.arange(R, 0, -1, dtype=np.float64)
    return dict(num_epochs=10, threshold=0.15, target_ratios=tuple(ratios / ratios.sum()))


def check_against_oracle(ours, ref, what=""):
    """(preds, scores, finals) of both sides, triple by triple; returns the largest deviation of a masked value."""
    worst = 0.0
    assert len(ours[0]) == len(ref[0])
    for j in range(len(ref[0])):
        assert ours[2][j].shape == ref[2][j].shape, (what, j)
        if len(ref[2][j]):
            worst = max(worst, float(np.abs(ours[2][j] - ref[2][j]).max()))
        np.testing.assert_allclose(ours[2][j], ref[2][j], rtol=0, atol=BAR, err_msg=f"{what} triple {j}")
        assert ours[0][j].dtype == np.int64 and ours[1][j].dtype == np.float32
        assert ours[0][j].shape == (len(ours[1][j]), 3) and len(ours[1][j]) == len(ref[1][j]), (what, j)
        _check_topk(ours[0][j], ours[1][j], ref[0][j], ref[1][j], BAR)
    return worst


def same_bits(a, b):
    return all(len(x) == len(y) and all(np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                                                        v.view(np.int32) if v.dtype == np.float32 else v)
                                        for u, v in zip(x, y)) for x, y in zip(a, b))


# -- synthetic: N = 40, triples in a row that share heads and tails ---------------------------------------------------
SHAPES = [(32, 3), (64, 4), (64, 1), (32, 8), (64, 8), (64, 5)]
_SYN = {}


def synthetic_run(D, R, kind, cuda):
    """The batched result and the oracle's for one (D, R, kind), computed once."""
    key = (D, R, kind)
    if key not in _SYN:
        N = 40
        tri, q, init, params = synthetic_case(R=R, D=D)
        if kind == "iddgcn":
            q = np.delete(q, EMPTY, 0)
        kw = kind_kw(kind, R)
        ref = ref_explain.mask_explainer(params, tri, q, N, R, init, **kw)
        model = RF.model_with(params, N, R, D)
        stats = {}
        ours = X.mask_explainer_batched(model, tri, q, init_value=init, return_masks=True, stats=stats, **kw)
        _SYN[key] = dict(model=model, tri=tri, q=q, init=init, kw=kw, ref=ref, ours=ours, stats=stats)
    return _SYN[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,R", SHAPES)
def test_synthetic_against_oracle(D, R, kind, cuda):
    """h == t, the (0,0)-only relation (kept by the threshold, then skipped), a triple with no candidate (GNNExplainer
    only: empty lists, placeholder zeros) and carried-over optimizer state, at every kernel width and at R = 1, 8."""
    c = synthetic_run(D, R, kind, cuda)
    worst = check_against_oracle(c["ours"], c["ref"], f"D={D} R={R} {kind}")
    print(f"synthetic D={D} R={R} {kind}: {c['stats']['levels']} levels for {len(c['q'])} triples, "
          f"max |masked value - oracle| {worst:.2e}")
    assert 1 < c["stats"]["levels"] < len(c["q"])
    if kind == "gnnexplainer":
        assert len(c["ours"][0][EMPTY]) == 0 and np.array_equal(c["ours"][2][EMPTY], np.zeros(R, np.float32))


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_bitwise_schedule_and_rerun(kind, cuda):
    """schedule="levels" == schedule="sequential" bitwise (levels never run two dependent triples together), a rerun
    is bitwise equal, and top_k beyond the kernel's 64 (completed on the host) agrees with the device selection."""
    c = synthetic_run(32, 3, kind, cuda)
    run = lambda **k: X.mask_explainer_batched(c["model"], c["tri"], c["q"], init_value=c["init"],  # noqa: E731
                                               return_masks=True, **c["kw"], **k)
    seq, again = run(schedule="sequential"), run()
    assert same_bits(seq, c["ours"]) and same_bits(again, c["ours"])
    big = run(top_k=100)
    ref = ref_explain.mask_explainer(c["model"]._named(), c["tri"], c["q"], 40, 3, c["init"], top_k=100, **c["kw"])
    check_against_oracle(big, ref, "top_k=100")
    for j in range(len(c["q"])):
        assert np.array_equal(big[0][j][:10], c["ours"][0][j]) and np.array_equal(big[1][j][:10], c["ours"][1][j])


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_against_per_triple_and_carry_over(kind, cuda):
    """The per-triple mask_explainer on the same triples is within 2e-5; triple 2 run alone (fresh optimizer) differs
    from its place in the batch by more than 1e-4: the shared state matters."""
    c = synthetic_run(32, 3, kind, cuda)
    per = X.mask_explainer(c["model"], c["tri"], c["q"], init_value=c["init"], return_masks=True, **c["kw"])
    for j in range(len(c["q"])):
        np.testing.assert_allclose(c["ours"][2][j], per[2][j], rtol=0, atol=2 * BAR)
        _check_topk(c["ours"][0][j], c["ours"][1][j], per[0][j], per[1][j], 2 * BAR)
    alone = X.mask_explainer_batched(c["model"], c["tri"], c["q"][1:2], init_value=c["init"], return_masks=True,
                                     **c["kw"])
    diff = np.abs(alone[2][0] - c["ours"][2][1]).max()
    print(f"carry-over {kind}: triple 2 alone vs in the batch {diff:.2e}")
    assert diff > 1e-4


# -- large degrees ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_large_degrees(kind, cuda):
    """N = 320, R = 3 with relation 2 empty (its placeholder is stored, never a candidate): rows of degree 1, 63, 64,
    65 and 300 (twice: relations 0 and 1), a column of degree 290 in both relations; the triple (5, 0, 6) has more
    than 1024 candidates (three staging passes), (6, 1, 5) and (5, 0, 5) follow on the same entries."""
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
    deg_r = np.bincount(np.concatenate([m.rows for m in mats[:2]]), minlength=N)
    deg_c = np.bincount(np.concatenate([m.cols for m in mats[:2]]), minlength=N)
    assert [deg_r[n] for n in (1, 2, 3, 4)] == [1, 63, 64, 65] and deg_r[5] > 600 and deg_c[6] > 256
    params = make_params(N, R, D, rng)
    init = rng.standard_normal((N, N)).astype(np.float32)
    q = np.array([(1, 0, 2), (2, 1, 3), (3, 0, 4), (4, 1, 5), (5, 0, 6), (6, 1, 5), (5, 0, 5), (3, 1, 1)], np.int64)
    kw = kind_kw(kind, R)
    ref = ref_explain.mask_explainer(params, tri, q, N, R, init, **kw)
    model = RF.model_with(params, N, R, D)
    stats = {}
    ours = X.mask_explainer_batched(model, tri, q, init_value=init, return_masks=True, stats=stats, **kw)
    worst = check_against_oracle(ours, ref, f"large degrees {kind}")
    n = [len(f) for f in ref[2]]
    assert max(n) > 1024
    print(f"large degrees {kind}: candidates {n}, {stats['levels']} levels, max deviation {worst:.2e}")
    seq = X.mask_explainer_batched(model, tri, q, init_value=init, return_masks=True, schedule="sequential", **kw)
    assert same_bits(seq, ours)


# -- fold 4, bundled weights --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold4(golden, cuda):
    adjacency, test = fold4_case(golden)
    w = golden("weights_fold4.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    init = np.random.default_rng(123).standard_normal((N_ENT, N_ENT)).astype(np.float32)
    oracle = {}

    def ref(kind):
        if kind not in oracle:
            oracle[kind] = ref_explain.mask_explainer(w, adjacency, test[:8], N_ENT, N_REL, init,
                                                      **kind_kw_fold4(kind))
        return oracle[kind]
    return model, adjacency, test[:8], init, ref


def kind_kw_fold4(kind):
    return dict(num_epochs=5, threshold=0.2) if kind == "gnnexplainer" else dict(
        num_epochs=10, threshold=0.15, target_ratios=(0.4, 0.4, 0.1, 0.1))


@pytest.mark.parametrize("kind", KINDS)
def test_fold4_against_oracle(kind, fold4):
    """The first 8 test triples (levels 1 2 2 3 4 1 3 5: carry-over and two-triple levels) through the public
    wrappers with the reference's defaults."""
    model, adjacency, test, init, ref = fold4
    fn = X.gnn_explainer_batched if kind == "gnnexplainer" else X.iddgcn_explainer_batched
    stats = {}
    ours = fn(model, adjacency, test, init_value=init, return_masks=True, stats=stats)
    assert stats["levels"] == 5
    worst = check_against_oracle(ours, ref(kind), f"fold 4 {kind}")
    print(f"fold 4 {kind}: max |masked value - oracle| {worst:.2e}")
    alone = fn(model, adjacency, test[1:2], init_value=init, return_masks=True)
    assert np.abs(alone[2][0] - ours[2][1]).max() > 1e-4


@pytest.mark.parametrize("first", ["per_triple", "batched"])
@pytest.mark.parametrize("kind", KINDS)
def test_fold4_optimizer_hand_over(kind, first, fold4):
    """4 triples on one path, then 4 on the other, with one MaskAdam: the 8-triple oracle run, within the bar."""
    model, adjacency, test, init, ref = fold4
    kw = kind_kw_fold4(kind)
    opt = X.MaskAdam((N_REL, N_ENT, N_ENT), model._device_state().device, 1e-3)
    paths = (X.mask_explainer, X.mask_explainer_batched)
    a, b = paths if first == "per_triple" else paths[::-1]
    one = a(model, adjacency, test[:4], init_value=init, return_masks=True, optimizer=opt, **kw)
    assert opt.iterations == 4 * kw["num_epochs"]
    two = b(model, adjacency, test[4:], init_value=init, return_masks=True, optimizer=opt, **kw)
    assert opt.iterations == 8 * kw["num_epochs"]
    both = tuple(x + y for x, y in zip(one, two))
    worst = check_against_oracle(both, ref(kind), f"hand-over {kind} {first} first")
    print(f"hand-over {kind}, {first} first: max deviation {worst:.2e}")


# -- envelope -----------------------------------------------------------------------------------------------------
def test_outside_the_envelope_raises(cuda):
    N, R = 40, 3
    tri, q, init, _ = synthetic_case(R=R)
    kw = dict(num_epochs=2, init_value=init)
    model = get_IDDGCN_Model(N, R, 256, 256, 123, None, 0, 0)
    with pytest.raises(L.IddgcnError, match="mask_explainer"):
        X.mask_explainer_batched(model, tri, q[:2], **kw)
    model = get_IDDGCN_Model(N, R, 64, 64, 123, None, 0, 0)
    eng = model._device_state()
    eng.features = "bf16"
    with pytest.raises(L.IddgcnError, match="mask_explainer"):
        X.mask_explainer_batched(model, tri, q[:2], **kw)
    eng.features = "f32"
    for attr in ("node_shard", "spmm_shard", "row_shard"):
        setattr(eng, attr, object())
        with pytest.raises(L.IddgcnError, match="mask_explainer"):
            X.mask_explainer_batched(model, tri, q[:2], **kw)
        setattr(eng, attr, None)
    with pytest.raises(L.IddgcnError, match="no entry"):               # 0 / 0 in the relation-ratio loss
        X.mask_explainer_batched(model, tri, q, target_ratios=(0.5, 0.3, 0.2), **kw)
    with pytest.raises(L.IddgcnError):
        X.mask_explainer_batched(model, tri, q[:2], target_ratios=(0.5, 0.5), **kw)
    for bad in ([[N, 0, 1]], [[0, R, 1]], [[0, 0, -1]]):
        with pytest.raises(L.IddgcnError):
            X.mask_explainer_batched(model, tri, np.array(bad), **kw)
    p_, s_ = X.mask_explainer_batched(model, tri, np.zeros((0, 3), np.int64), **kw)
    assert p_ == [] and s_ == []
