"""Host side of batched explaiNE (no GPU): the new C-ABI symbols, their rejections before launch, and the numpy merge
that completes a query's top-k from its candidate list (explain.rank_sparse_gradient) against the oracle's get_pred
on the full gradient vector."""
import ctypes

import numpy as np
import pytest

from iddgcn_amd import _lib
from iddgcn_amd.explain import rank_sparse_gradient
from oracle import ref_explain

SEEDS, ROWS, TOPK = "iddgcn_explain_seeds_f32", "iddgcn_explain_row_grads_f32", "iddgcn_explain_topk_f32"


def test_new_symbols_are_bound():
    lib = _lib.load()
    for name in (SEEDS, ROWS, TOPK):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert getattr(lib, SEEDS).argtypes == _lib.SIGNATURES[SEEDS][1]


# Null stream, null or made-up pointers: every call below must be rejected on the host, before any launch (the
# addresses are never dereferenced).
A = ctypes.c_void_p(1 << 20)          # 16-byte aligned
MIS = ctypes.c_void_p((1 << 20) + 4)  # float-aligned only


def _seeds(lib, Q=1, N=10, d=64, R=2, ptr=None, ES1=None, P=None, G=None, pls=0, prs=0):
    p = ptr
    return lib.iddgcn_explain_seeds_f32(None, Q, N, d, R, p, p, p, 1.0, ES1 or p, P or p, pls, prs, p, p, 0, p, 0,
                                        p, p, p, p, p, p, p, p, G or p, p)


def _rows(lib, Q=1, N=10, d=64, R=2, ptr=None, G=None, E=None):
    p = ptr
    return lib.iddgcn_explain_row_grads_f32(None, Q, N, d, R, p, p, p, p, None, G or p, E or p, p, p, p)


def _topk(lib, Q=1, k=10, ptr=None):
    p = ptr
    return lib.iddgcn_explain_topk_f32(None, Q, k, p, p, p, p, p, p)


def test_rejections_before_launch():
    lib = _lib.load()
    for call in (_seeds, _rows):
        assert call(lib, d=48) == -1
        assert call(lib, d=128) == -1
        assert call(lib, d=256) == -1
        assert call(lib, R=0) == -2
        assert call(lib, R=9) == -2
        assert call(lib, N=0) == -3
        assert call(lib, Q=-1) == -3
        assert call(lib) == -3                       # null tables
        assert call(lib, Q=0) == 0                   # nothing to do, nothing launched
    # misaligned tables: every pointer given, one of the 16-byte-read tables off by a float
    assert _seeds(lib, ptr=A, ES1=MIS) == -3
    assert _seeds(lib, ptr=A, P=MIS) == -3
    assert _seeds(lib, ptr=A, G=MIS) == -3
    assert _seeds(lib, ptr=A, pls=6) == -3
    assert _seeds(lib, ptr=A, prs=2) == -3
    assert _seeds(lib, ptr=A, prs=-4) == -3
    assert _rows(lib, ptr=A, E=MIS) == -3
    assert _rows(lib, ptr=A, G=MIS) == -3
    assert _topk(lib, k=0) == -3
    assert _topk(lib, k=65) == -3
    assert _topk(lib, Q=-1) == -3
    assert _topk(lib) == -3                          # null qptr / outputs
    assert _topk(lib, Q=0) == 0


# -- the merge helper ------------------------------------------------------------------------------
def _oracle(nnz, entry, grad, k):
    """ref_explain.get_pred on the dense per-relation gradient lists; the flat entry id of (idx, rel) is
    offsets[rel] + idx, recovered from the triples it returns (coo rows encode it)."""
    total = int(sum(nnz))
    dense = np.zeros(total, np.float32)
    dense[entry] = grad
    off = np.concatenate([[0], np.cumsum(nnz)])
    # coo rows [flat id, 0]: the returned triple's head is the flat entry id
    coo = [(np.stack([np.arange(off[r], off[r + 1]), np.zeros(nnz[r], np.int64)], 1), None) for r in range(len(nnz))]
    trip, sc = ref_explain.get_pred(coo, [dense[off[r]:off[r + 1]] for r in range(len(nnz))], k)
    return trip[:, 0], np.asarray(sc, np.float32)


def _check(nnz, entry, grad, k):
    entry, grad = np.asarray(entry, np.int64), np.asarray(grad, np.float32)
    ids, sc = rank_sparse_gradient(entry, grad, int(sum(nnz)), k)
    ref_ids, ref_sc = _oracle(nnz, entry, grad, k)
    assert len(ids) == min(k, int(sum(nnz)))
    assert np.array_equal(ids, ref_ids), (ids, ref_ids)
    assert np.array_equal(sc, ref_sc)
    assert sc.dtype == np.float32


def test_merge_fewer_than_k_positives():
    # 3 positives, k = 10: positives, then zero-class ids ascending skipping the non-zero candidates
    _check([20, 20], [5, 17, 30, 2, 33], [0.5, 2.0, 1.0, -1.0, -3.0], 10)


def test_merge_zero_valued_candidates_stay_in_the_zero_class():
    _check([15, 15], [0, 3, 4, 9, 20], [0.0, 1.0, -0.0, 0.0, -2.0], 12)
    # a zero-valued candidate keeps its stored sign in the scores
    ids, sc = rank_sparse_gradient([1, 2], [-0.0, 3.0], 5, 4)
    assert ids.tolist() == [2, 0, 1, 3] and np.signbit(sc).tolist() == [False, False, True, False]


def test_merge_candidates_at_the_first_entry_ids():
    # non-zero candidates occupy ids 0..m: the zero class starts after them
    m = 7
    _check([30], list(range(m + 1)), [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0], 10)
    _check([30], list(range(m + 1)), [-1.0] * (m + 1), 10)


def test_merge_negatives_only_when_nnz_is_small():
    entry, grad = [0, 2, 4, 5], [-1.0, 2.0, -0.5, -0.5]
    _check([3, 3], entry, grad, 5)                   # 1 positive + 2 zeros + 2 of the 3 negatives, tie by id
    _check([3, 3], entry, grad, 3)                   # negatives not reached
    _check([40, 40], entry, grad, 10)                # large nnz: zeros fill, no negative


def test_merge_top_k_larger_than_nnz():
    _check([2, 3], [4, 1, 0], [1.0, -1.0, 1.0], 64)
    _check([1], [], [], 3)


def test_merge_ties_and_random_cases():
    rng = np.random.default_rng(11)
    for _ in range(60):
        nnz = [int(x) for x in rng.integers(1, 15, int(rng.integers(1, 5)))]
        total = sum(nnz)
        m = int(rng.integers(0, total + 1))
        entry = rng.permutation(total)[:m]
        grad = np.round(rng.standard_normal(m), 1).astype(np.float32)       # many ties and exact zeros
        _check(nnz, entry, grad, int(rng.integers(1, total + 5)))


def test_merge_rejects_mismatched_lengths():
    with pytest.raises(ValueError):
        rank_sparse_gradient([0, 1], [1.0], 5, 2)    # entry / grad of different lengths
