"""Explanation ground truth, host side (no GPU): the CPU restatement against the reference's bundled gt_all.csv, the
gt_all.csv layout, the gt_process.py filter, evaluate_explanations, the similarity loader's dropped row and the
disjoint-id check of the public call."""
import functools
import os

import numpy as np
import pytest

from iddgcn_amd import IddgcnError
from iddgcn_amd import ground_truth as G
from iddgcn_amd.explain import explanation_metrics
from tests import ref_ground_truth as ref
from tests.conftest import REFERENCE
from tests.ref_ground_truth import bundled, fixture


@functools.lru_cache(maxsize=None)
def restated():
    return ref.ground_truth(*bundled())


def test_loader_drops_the_first_row_by_default():
    for name, rows in (("mu_similar0.97.csv", 16180), ("drug_similar0.78.csv", 1174)):
        path = os.path.join(REFERENCE, name)
        kept, full = G.load_similarity_csv(path), G.load_similarity_csv(path, reference_header=False)
        assert full.shape == (rows, 3) and kept.shape == (rows - 1, 3) and full.dtype == np.int64
        assert np.array_equal(kept, full[1:])
        assert full[0].tolist() == [int(v) for v in open(path).readline().split(",")]
    assert bundled()[0].shape == (1754, 3)


def test_restatement_reproduces_gt_all():
    queries, want = ref.fixture_lists(fixture()["gt_all"])
    got = restated()
    assert np.array_equal(queries, bundled()[0]) and len(got) == 1754
    for q, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), q
    lens = np.array([len(g) for g in got])
    assert (lens == 0).sum() == 317 and lens.max() == 125 and fixture()["gt_all"].shape == (1754, 3 + 3 * 125)


def test_restatement_needs_the_dropped_row():
    """With every similarity row kept the result differs from gt_all.csv: the loading quirk is real."""
    dc = bundled()[0]
    full = [G.load_similarity_csv(os.path.join(REFERENCE, f), reference_header=False)
            for f in ("mu_similar0.97.csv", "drug_similar0.78.csv")]
    _, want = ref.fixture_lists(fixture()["gt_all"])
    got = ref.ground_truth(dc, *full)
    assert any(not np.array_equal(g, w) for g, w in zip(got, want))


def test_ground_truth_table_matches_the_csv_layout():
    ptr, tri = ref.as_csr(restated())
    table = G.ground_truth_table(bundled()[0], ptr, tri)
    want = fixture()["gt_all"]
    assert table.dtype == np.float64 and table.shape == want.shape
    assert np.array_equal(np.isnan(table), want == -1)
    assert np.array_equal(np.where(np.isnan(table), -1, table), want)
    # no query at all, and queries without any ground truth
    assert G.ground_truth_table(np.zeros((0, 3), np.int64), np.zeros(1, np.int64), np.zeros((0, 3))).shape == (0, 3)
    assert G.ground_truth_table(bundled()[0][:2], np.zeros(3, np.int64), np.zeros((0, 3))).shape == (2, 3)


def test_filter_gives_the_reference_test_triples():
    ptr, tri = ref.as_csr(restated())
    f = fixture()
    kept, gts = G.filter_ground_truth(f["fold4_X_test"], bundled()[0], ptr, tri)
    assert f["fold4_X_test"].shape == (700, 3) and kept.shape == (288, 3) and kept.dtype == np.int64
    assert np.array_equal(kept, f["test_filtered_fold4"])
    where = {tuple(q): i for i, q in enumerate(bundled()[0].tolist())}
    for row, g in zip(kept.tolist(), gts):
        assert len(g) >= 1 and np.array_equal(g, restated()[where[tuple(row)]])
    kept10, gts10 = G.filter_ground_truth(f["fold4_X_test"], bundled()[0], ptr, tri, min_count=10)
    assert 0 < len(kept10) < 288 and all(len(g) >= 10 for g in gts10)
    assert [r for r, g in zip(kept.tolist(), gts) if len(g) >= 10] == kept10.tolist()
    # a test triple the ground truth does not know is dropped; with min_count = 0 it stays, empty
    k0, g0 = G.filter_ground_truth([[5, 0, 700], [0, 0, 661]], bundled()[0], ptr, tri, min_count=0)
    assert k0.tolist() == [[5, 0, 700], [0, 0, 661]] and len(g0[0]) == 0
    assert len(G.filter_ground_truth([[99999, 0, 99999]], bundled()[0], ptr, tri)[0]) == 0


def test_filter_repeats_a_test_triple_per_matching_query():
    queries = np.array([[1, 0, 9], [2, 0, 9], [1, 0, 9]])
    ptr, tri = np.array([0, 1, 1, 3]), np.array([[4, 0, 9], [5, 0, 9], [1, 2, 3]])
    kept, gts = G.filter_ground_truth([[2, 0, 9], [1, 0, 9]], queries, ptr, tri)
    assert kept.tolist() == [[1, 0, 9], [1, 0, 9]]
    assert [g.tolist() for g in gts] == [[[4, 0, 9]], [[5, 0, 9], [1, 2, 3]]]


def test_evaluate_explanations_is_a_loop_over_explanation_metrics(golden):
    ptr, tri = ref.as_csr(restated())
    kept, gts = G.filter_ground_truth(fixture()["fold4_X_test"], bundled()[0], ptr, tri)
    ex = golden("explain_fold4.npz")
    assert np.array_equal(ex["test_triples"], kept)
    preds = ex["explaine_preds"]
    for top, exp_num in ((5, 10), (1, 10), (10, 10), (3, 5)):
        per, mean = G.evaluate_explanations(preds, gts, top=top, exp_num=exp_num)
        want = np.array([explanation_metrics(p, g, top=top, exp_num=exp_num) for p, g in zip(preds, gts)])
        assert per.shape == (288, 3) and per.dtype == np.float64
        assert np.array_equal(per, want) and np.array_equal(mean, want.mean(0))
    assert G.evaluate_explanations(preds, gts)[0].max() > 0      # the bundled explanations do hit the ground truth
    with pytest.raises(IddgcnError):
        G.evaluate_explanations(preds[:3], gts[:2])


def test_overlapping_id_sets_raise():
    dc = np.array([[0, 0, 10], [1, 0, 11]])
    mu, drug = np.array([[0, 3, 1]]), np.array([[10, 2, 11]])
    assert G.check_id_sets(dc, mu, drug) == (12, 1)
    for bad in ((np.array([[0, 0, 10], [10, 0, 11]]), mu, drug),          # a dc mutation that is a drug
                (dc, np.array([[0, 3, 11]]), drug),                      # a similar "mutation" that is a drug
                (dc, mu, np.array([[10, 2, 1]])),                        # a similar "drug" that is a mutation
                (dc, np.array([[5, 3, 6]]), np.array([[6, 2, 7]]))):     # only the similarity tables overlap
        with pytest.raises(IddgcnError, match="both a mutation and a drug"):
            G.check_id_sets(*bad)
        with pytest.raises(IddgcnError, match="both a mutation and a drug"):   # the public call checks first
            G.construct_ground_truth(*bad)
    with pytest.raises(IddgcnError, match="negative"):
        G.check_id_sets(np.array([[0, 0, -1]]), mu, drug)


def test_general_added_set_differs_only_when_ids_overlap():
    """The restatement keeps the reference's single set of pairs; with overlapping ids a (drug, mutation) pair of
    step 3 can suppress a similarity triple of step 4, which the per-value dedup would emit: why the public call
    refuses such input."""
    # drug0 = 5 is also a mutation: step 3 adds (d, m) = (5, 6)... build the collision (drug0, d) == (d', m)
    dc = np.array([[1, 0, 5], [6, 0, 5], [6, 0, 6]])
    mu_sim, drug_sim = np.array([[1, 3, 6]]), np.array([[5, 2, 6], [5, 2, 5]])
    got = ref.ground_truth(dc, mu_sim, drug_sim, queries=[[1, 0, 5]])[0].tolist()
    # SM = [6], SD = [6, 5]; step 3 hits (6, 0, 6) and (6, 0, 5) and adds the pairs (6, 6) and (5, 6);
    # step 4 would emit (5, 2, 6) but the pair (5, 6) is already in the set
    assert [5, 2, 6] not in got and [5, 2, 5] in got
