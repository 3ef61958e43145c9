"""Explanation ground truth on the GPU (csrc/ground_truth.hip through ground_truth.construct_ground_truth).

Every comparison is exact equality of ``ptr`` and ``triples``: against the reference's bundled gt_all.csv for the
bundled tables, against the CPU restatement (tests/ref_ground_truth.py) for small synthetic tables built around the
places the kernel can go wrong: empty lists, the 256-probe chunk boundary, ordered compaction across lanes / waves /
chunks with repeated cells, repeated and mirrored similarity pairs, 64-bit keys, the list capacity."""
import numpy as np
import pytest
import torch

from iddgcn_amd import IddgcnError
from iddgcn_amd import _lib as L
from iddgcn_amd import get_IDDGCN_Model
from iddgcn_amd import ground_truth as G
from iddgcn_amd.explain import explaine_batched, explanation_metrics
from tests import ref_ground_truth as ref
from tests.ref_ground_truth import bundled, fixture

pytestmark = pytest.mark.gpu
CHUNK = 256                                # probes per chunk = threads of the query workgroup (ground_truth.hip NT)
E = np.zeros((0, 3), np.int64)


def device_gt(cuda, dc, mu, drug, queries=None, **kw):
    ptr, tri = G.construct_ground_truth(np.asarray(dc), np.asarray(mu), np.asarray(drug), queries, device=cuda, **kw)
    assert ptr.is_cuda and tri.is_cuda and ptr.dtype == torch.int64 and tri.dtype == torch.int64
    ptr, tri = ptr.cpu().numpy(), tri.cpu().numpy()
    nq = len(dc) if queries is None else len(queries)
    assert ptr.shape == (nq + 1,) and tri.shape == (ptr[-1], 3) and ptr[0] == 0
    return ptr, tri


def check(cuda, dc, mu, drug, queries=None, **kw):
    """Device result == restatement, exactly; returns the per-query lengths."""
    ptr, tri = device_gt(cuda, dc, mu, drug, queries, **kw)
    rptr, rtri = ref.as_csr(ref.ground_truth(dc, mu, drug, queries, **kw))
    assert np.array_equal(ptr, rptr)
    assert np.array_equal(tri, rtri)
    return np.diff(ptr)


def star(center, others, rel):
    """Similarity rows (center, rel, o): the list of `center` is `others` in this order."""
    return np.array([[center, rel, o] for o in others], np.int64).reshape(-1, 3)


def dense(mus, drugs, rels=(0,)):
    return np.array([[m, r, d] for r in rels for d in drugs for m in mus], np.int64)


# ---- the bundled data -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled_device(cuda):
    return device_gt(cuda, *bundled())


def test_bundled_gt_all_exact(bundled_device):
    ptr, tri = bundled_device
    queries, want = ref.fixture_lists(fixture()["gt_all"])
    wptr, wtri = ref.as_csr(want)
    assert np.array_equal(queries, bundled()[0])
    assert np.array_equal(ptr, wptr) and np.array_equal(tri, wtri)
    lens = np.diff(ptr)
    assert (lens == 0).sum() == 317 and lens.max() == 125 and len(lens) == 1754
    table = G.ground_truth_table(queries, ptr, tri)
    assert np.array_equal(np.where(np.isnan(table), -1, table), fixture()["gt_all"])


def test_bundled_fold4_filter(bundled_device):
    ptr, tri = bundled_device
    kept, gts = G.filter_ground_truth(fixture()["fold4_X_test"], bundled()[0], ptr, tri)
    assert np.array_equal(kept, fixture()["test_filtered_fold4"]) and len(gts) == 288


# ---- small synthetic tables -----------------------------------------------------------------------------------------
def test_empty_lists_and_absent_queries(cuda):
    # mutations 0..5, drugs 10..15; mutation 4 and drug 14 have no similarity row
    mu = np.array([[0, 3, 1], [2, 3, 0], [1, 3, 2]])
    drug = np.array([[10, 2, 11], [12, 2, 10]])
    dc = np.array([[0, 0, 10], [1, 0, 10], [2, 0, 11], [0, 0, 12], [4, 0, 10], [4, 0, 14], [0, 0, 14], [1, 0, 12]])
    lens = check(cuda, dc, mu, drug)
    assert lens[5] == 0 and lens[0] > 0                       # (4, 0, 14): both lists empty
    queries = np.array([[4, 0, 10],       # empty SM
                        [0, 0, 14],       # empty SD
                        [4, 0, 14],       # both empty
                        [2, 0, 12],       # not a row of dc, lists not empty
                        [5, 0, 15],       # ids no table mentions
                        [0, 1, 10],       # a relation dc does not have
                        [30, 0, 40]])     # ids beyond every table
    lens = check(cuda, dc, mu, drug, queries)
    assert lens[2] == 0 and lens[3] > 0 and lens[4] == lens[5] == lens[6] == 0
    # empty tables
    assert check(cuda, dc, E, E).sum() == 0
    assert check(cuda, dc, mu, E).sum() > 0 and check(cuda, dc, E, drug).sum() > 0
    assert check(cuda, E, mu, drug, queries[:2]).sum() == 0
    ptr, tri = device_gt(cuda, dc, mu, drug, E)
    assert ptr.tolist() == [0] and tri.shape == (0, 3)


@pytest.mark.parametrize("nm,nd", [(15, 15), (0, 256), (256, 0), (5, 42), (26, 18), (40, 50)])
def test_chunk_boundaries_dense(nm, nd, cuda):
    """|SM| + |SD| + |SD| |SM| = 255, 256 (either list alone), 257, 512 and 2090 probes over a dc in which EVERY probe
    hits: the ordered compaction is exercised across every lane, wave and chunk boundary."""
    total = nm + nd + nm * nd
    assert total in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2090)
    D0 = 1000
    mu, drug = star(0, range(1, nm + 1), 3), star(D0, range(D0 + 1, D0 + nd + 1), 2)
    dc = dense(range(nm + 1), range(D0, D0 + nd + 1))
    lens = check(cuda, dc, mu, drug, [[0, 0, D0], [nm, 0, D0 + nd]])
    assert lens[0] == total + nd + nm


@pytest.mark.parametrize("seed", [0, 1])
def test_multiplicity_and_sparse_hits(seed, cuda):
    """dc rows repeated 1-3 times (a cell takes c slots: the shuffle-scan path) and, in the second half of the grid,
    thinned so that waves with no hit, one-slot hits only and repeated cells all occur; several chunks."""
    rng = np.random.default_rng(seed)
    nm, nd, D0 = 37, 29, 500
    mu, drug = star(0, rng.permutation(np.arange(1, nm + 1)), 3), star(D0, D0 + 1 + rng.permutation(nd), 2)
    dc = dense(range(nm + 1), range(D0, D0 + nd + 1))
    keep = (dc[:, 2] < D0 + nd // 2) | (rng.random(len(dc)) < 0.1)
    dc = dc[keep]
    dc = np.repeat(dc, rng.integers(1, 4, len(dc)), axis=0)
    dc = dc[rng.permutation(len(dc))]
    lens = check(cuda, dc, mu, drug)
    assert lens.max() > 3 * CHUNK
    check(cuda, dc, mu, drug, [[0, 0, D0]])


def test_repeated_mirrored_and_self_pairs(cuda):
    """A pair listed twice, as (a, b) and (b, a), and self-pairs: steps 1-3 emit once per list entry, steps 4-5 once
    per distinct value, at its first position."""
    mu = np.array([[0, 3, 1], [0, 3, 1], [1, 3, 0], [0, 3, 0], [2, 3, 0], [0, 3, 2], [3, 3, 3], [1, 3, 2]])
    drug = np.array([[10, 2, 11], [11, 2, 10], [10, 2, 11], [10, 2, 10], [12, 2, 12], [11, 2, 12]])
    dc = dense(range(4), range(10, 13))
    lens = check(cuda, dc, mu, drug)
    rows = ref.ground_truth(dc, mu, drug, [[0, 0, 10]])[0]
    sm, sd = [1, 1, 0, 2, 1, 0, 2], [11, 11, 10, 11, 10]       # forward rows in table order, then the reversed ones
    assert len(rows) == len(sm) + len(sd) + len(sm) * len(sd) + 2 + 3
    assert rows[-5:].tolist() == [[10, 2, 11], [10, 2, 10], [0, 3, 1], [0, 3, 0], [0, 3, 2]]
    assert lens.max() == len(rows)
    # a node whose only similarity rows are self-pairs: its list holds itself twice (forward + reversed)
    check(cuda, dc, mu, drug, [[3, 0, 12]])


@pytest.mark.parametrize("R", [1, 2, 4])
def test_same_pair_under_several_relations(R, cuda):
    rng = np.random.default_rng(R)
    NM, ND = 30, 20
    mu = np.stack([rng.integers(0, NM, 90), np.full(90, 3), rng.integers(0, NM, 90)], 1)
    drug = np.stack([rng.integers(NM, NM + ND, 50), np.full(50, 2), rng.integers(NM, NM + ND, 50)], 1)
    pairs = np.stack([rng.integers(0, NM, 150), rng.integers(NM, NM + ND, 150)], 1)
    dc = np.concatenate([np.stack([pairs[:, 0], np.full(150, r), pairs[:, 1]], 1)[rng.random(150) < 0.7]
                         for r in range(R)])
    if R > 1:        # the very same (mu, drug) under relations 0 and R-1, other relations between
        assert len({(m, d) for m, r, d in dc.tolist() if r == 0} & {(m, d) for m, r, d in dc.tolist() if r == R - 1})
    lens = check(cuda, dc, mu, drug)
    assert lens.max() > 0
    check(cuda, dc, mu, drug, dc[::-1][:40])


def test_keys_beyond_32_bits(cuda):
    """N = 70000, R = 2: (rel N + drug) N + mu reaches 9.8e9 > 2^32 on tables of a few rows."""
    N = 70000
    mus, drugs = [0, 1, 34000, 34999, 3], [35000, 65536, 69998, N - 1]
    mu = np.array([[0, 3, 34999], [34000, 3, 0], [1, 3, 0], [3, 3, 34999]])
    drug = np.array([[N - 1, 2, 35000], [65536, 2, N - 1], [69998, 2, N - 1]])
    dc = dense(mus, drugs, rels=(0, 1))
    dc = dc[np.random.default_rng(5).random(len(dc)) < 0.7]
    assert ((dc[:, 1] * N + dc[:, 2]) * N + dc[:, 0]).max() > 2 ** 32
    assert check(cuda, dc, mu, drug).max() > 0
    # two cells whose keys agree modulo 2^32 must not be confused: (m, 0, d) and (m', r', d') with the same low word
    k = (0 * N + 35000) * N + 3
    k2 = k + 2 ** 32
    m2, d2, r2 = k2 % N, (k2 // N) % N, k2 // N // N
    assert r2 < 2 and not {m2, 0, 3} & {d2, N - 1, 35000}
    lens = check(cuda, np.array([[m2, r2, d2]]), np.array([[0, 3, 3]]), np.array([[N - 1, 2, 35000]]),
                 [[0, 0, N - 1]])
    assert lens[0] == 0


def test_long_lists_and_capacity(cuda):
    """A 4096-entry list on each side works; one entry beyond IDDGCN_GT_LIST_CAPACITY raises, on either side."""
    cap = L.GT_LIST_CAPACITY
    assert cap >= 4096
    rng = np.random.default_rng(3)
    D0 = 20000
    mu = star(0, rng.integers(1, 3000, 4096), 3)                   # with repeats
    drug = star(D0, D0 + 1 + np.arange(4), 2)
    dc = np.stack([rng.integers(0, 3000, 6000), np.zeros(6000, np.int64), D0 + rng.integers(0, 5, 6000)], 1)
    assert check(cuda, dc, mu, drug, [[0, 0, D0]])[0] > 4096
    mu2, drug2 = star(0, [1, 2, 3], 3), star(D0, D0 + 1 + rng.integers(0, 3000, 4096), 2)
    dc2 = np.stack([rng.integers(0, 4, 6000), np.zeros(6000, np.int64), D0 + rng.integers(0, 3001, 6000)], 1)
    assert check(cuda, dc2, mu2, drug2, [[0, 0, D0]])[0] > 4096
    # exactly the capacity works, one more raises and nothing is returned
    full = star(0, 1 + np.arange(cap) % 50, 3)
    assert check(cuda, dc, full, drug, [[0, 0, D0], [1, 0, D0]])[0] > 0
    over = star(0, 1 + np.arange(cap + 1) % 50, 3)
    with pytest.raises(IddgcnError, match="longer than"):
        G.construct_ground_truth(dc, over, drug, [[1, 0, D0], [0, 0, D0]], device=cuda)
    with pytest.raises(IddgcnError, match="longer than"):
        G.construct_ground_truth(dc, mu, star(D0, D0 + 1 + np.arange(cap + 1) % 7, 2), [[0, 0, D0]], device=cuda)
    # the long list only matters for the queries that use it
    check(cuda, dc, over, drug, [[1, 0, D0], [5, 0, D0 + 1]])


def test_similarity_relation_ids(cuda):
    dc, mu, drug = bundled()
    q = dc[np.flatnonzero(fixture()["gt_all"][:, 3] >= 0)[[0, 50, 400, 900]]]
    a = check(cuda, dc, mu, drug, q, drug_rel=7, mu_rel=9)
    b = check(cuda, dc, mu, drug, q)
    assert np.array_equal(a, b)
    _, tri = device_gt(cuda, dc, mu, drug, q, drug_rel=7, mu_rel=9)
    assert set(np.unique(tri[:, 1])) <= {0, 1, 7, 9} and (tri[:, 1] == 7).any() and (tri[:, 1] == 9).any()


def test_device_tensors_in(cuda):
    dc, mu, drug = (torch.as_tensor(x, device=cuda) for x in bundled())
    ptr, tri = G.construct_ground_truth(dc, mu, drug, dc[:50])
    rptr, rtri = ref.as_csr(ref.ground_truth(*bundled(), bundled()[0][:50]))
    assert np.array_equal(ptr.cpu().numpy(), rptr) and np.array_equal(tri.cpu().numpy(), rtri)


# ---- determinism ----------------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_chunked(bundled_device, cuda):
    ptr, tri = bundled_device
    ptr2, tri2 = device_gt(cuda, *bundled())
    assert np.array_equal(ptr, ptr2) and np.array_equal(tri, tri2)
    dc = bundled()[0]
    index = G.GroundTruthIndex(*bundled(), device=cuda)
    parts = [index.query(dc[a:b]) for a, b in ((0, 1), (1, 600), (600, 601), (601, 1754))]
    lens = np.concatenate([np.diff(p.cpu().numpy()) for p, _ in parts])
    assert np.array_equal(np.concatenate([[0], np.cumsum(lens)]), ptr)
    assert np.array_equal(np.concatenate([t.cpu().numpy() for _, t in parts]), tri)


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_explaine_batched_scored_against_device_ground_truth(bundled_device, golden, cuda):
    ptr, tri = bundled_device
    kept, gts = G.filter_ground_truth(fixture()["fold4_X_test"], bundled()[0], ptr, tri)
    d = golden("fold4_data.npz")
    model = get_IDDGCN_Model(845, 4, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    adjacency = np.concatenate([d["X_train"].astype(np.int64), kept])
    preds, _ = explaine_batched(model, adjacency, kept[:32], top_k=10)
    per, mean = G.evaluate_explanations(preds, gts[:32], top=5, exp_num=10)
    want = np.array([explanation_metrics(p, g, top=5, exp_num=10) for p, g in zip(preds, gts[:32])])
    assert per.shape == (32, 3) and np.array_equal(per, want) and np.array_equal(mean, want.mean(0))
