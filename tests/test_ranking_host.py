"""Host side of all-candidate ranking (no GPU): the metrics, the filter-CSR builder, the new C-ABI symbols and
their rejections before launch."""
import numpy as np
import pytest

from iddgcn_amd import _lib, classification_metrics, ranking_metrics
from iddgcn_amd.utils import filter_csr


def test_ranking_metrics_hand_written():
    m = ranking_metrics([1, 2, 4, 10, 20])
    assert m["n"] == 5
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 4 + 1 / 10 + 1 / 20) / 5, abs=1e-15)
    assert m["mean_rank"] == pytest.approx(37 / 5, abs=1e-15)
    assert m["hits@1"] == 0.2 and m["hits@3"] == 0.4 and m["hits@10"] == 0.8
    # a tied target's fractional rank counts as it is
    m = ranking_metrics([1.5, 3.0], ks=(1, 2, 3))
    assert m["mrr"] == pytest.approx((1 / 1.5 + 1 / 3) / 2, abs=1e-15)
    assert (m["hits@1"], m["hits@2"], m["hits@3"]) == (0.0, 0.5, 1.0)
    with pytest.raises(ValueError):
        ranking_metrics([])
    with pytest.raises(ValueError):
        ranking_metrics([0, 1])


def test_classification_metrics_match_reference_block(golden):
    """IDDGCN_eval.py:71-84 through sklearn (oracle.ref_model.eval_metrics) on the fold-0 evaluation fixture."""
    from oracle.ref_model import eval_metrics
    ev = golden("fold0_eval.npz")
    ours, ref = classification_metrics(ev["y_true"], ev["probs"]), eval_metrics(ev["y_true"], ev["probs"])
    assert set(ours) == set(ref)
    for name, v in ref.items():
        assert abs(ours[name] - v) <= 1e-12, (name, ours[name], v)
    # tied scores: one ROC / PR point per distinct score
    y = np.array([1, 0, 1, 1, 0, 0, 1, 0])
    p = np.array([0.9, 0.9, 0.7, 0.7, 0.7, 0.2, 0.2, 0.1])
    ours, ref = classification_metrics(y, p, threshold=0.6), eval_metrics(y, p, threshold=0.6)
    for name, v in ref.items():
        assert abs(ours[name] - v) <= 1e-12, (name, ours[name], v)
    with pytest.raises(ValueError):
        classification_metrics([1, 1], [0.3, 0.4])


@pytest.mark.parametrize("side", ["tail", "head"])
def test_filter_csr_against_brute_force(side):
    rng = np.random.default_rng(5)
    N, R = 23, 3
    f = np.stack([rng.integers(0, N, 400), rng.integers(0, R, 400), rng.integers(0, N, 400)], 1)
    f = np.concatenate([f, f[:50]])                                 # duplicates in the filter
    q = f[rng.integers(0, len(f), 30)].copy()                       # targets inside the filter
    # a query with no filter entries: a (relation, node) pair no filter triple has
    fixed, cand = (0, 2) if side == "tail" else (2, 0)
    f = f[~((f[:, 1] == 1) & (f[:, fixed] == 7))]
    q[3] = (7, 1, 7)
    fptr, fidx = filter_csr(q, side, f, N)
    assert fptr.dtype == np.int32 and fidx.dtype == np.int32 and fptr.shape == (len(q) + 1,)
    assert fptr[0] == 0 and fptr[-1] == len(fidx)
    known = {}
    for tr in f:
        known.setdefault((int(tr[1]), int(tr[fixed])), set()).add(int(tr[cand]))
    n_target = 0
    for i, tr in enumerate(q):
        want = sorted(known.get((int(tr[1]), int(tr[fixed])), set()))
        got = fidx[fptr[i]:fptr[i + 1]].tolist()
        assert got == want, (i, got, want)                          # ascending, unique
        n_target += int(tr[cand]) in got
    assert fptr[4] - fptr[3] == 0
    assert n_target >= 20                                           # the targets really are among the entries
    with pytest.raises(ValueError):
        filter_csr(q, "both", f, N)


def test_new_symbols_are_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 13 and lib.iddgcn_abi_version() == 13
    for name in ("iddgcn_screen_chain_f32", "iddgcn_rank_topk_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def _chain(lib, Q=1, N=10, d=64, R=2, side=0):
    # null stream, null pointers: every rejection below happens on the host, before any launch
    return lib.iddgcn_screen_chain_f32(None, Q, N, d, R, side, *[None] * 4, 0, 0, None, 0, *[None] * 5)


def _topk(lib, Q=1, N=10, k=10):
    return lib.iddgcn_rank_topk_f32(None, Q, N, k, *[None] * 8)


def test_rejections_before_launch():
    lib = _lib.load()
    assert _chain(lib, d=48) == -1
    assert _chain(lib, d=128) == -1
    assert _chain(lib, R=9) == -2
    assert _chain(lib, R=0) == -2
    assert _chain(lib, N=0) == -3
    assert _chain(lib, side=2) == -3
    assert _chain(lib) == -3                    # null tables
    assert _topk(lib, k=0) == -3
    assert _topk(lib, k=65) == -3
    assert _topk(lib, N=0) == -3
    assert _topk(lib) == -3                     # null s
    assert _topk(lib, Q=-1) == -3
