"""Device classification metrics (iddgcn_clf_metrics, iddgcn_keep_best_f32), IDDGCN_Model.evaluate and the validation
inside fit, on the GPU.

The reference of every case is computed here with numpy: the integers (confusion counts, P, N_neg, the number of
distinct scores and auc_num2 = sum_g fp_g (2 TP_before_g + tp_g)) from a stable argsort of the float32 bit pattern
and bincount, the doubles from the host classification_metrics.  Bars: integers exact; roc_auc bitwise
auc_num2 / (2 P N_neg); aupr within 4 n_thresholds 2^-53 (any-order fp64 summation of at most n_thresholds terms
whose sum is at most 1); bce within n 2^-50 relative (at most 2 ulp per log plus the summation)."""
import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import classification_metrics, classification_metrics_device, get_IDDGCN_Model, ops
from iddgcn_amd.graph import get_adj_mats
from iddgcn_amd.model import Callback
from iddgcn_amd.utils import synthetic_graph

pytestmark = pytest.mark.gpu
N_ENT, N_REL = 845, 4
INT_KEYS = ("tp", "tn", "fp", "fn", "n_pos", "n_neg", "n_thresholds", "auc_num2")
SMALL = L.CLF_SMALL_MAX


# ---- numpy reference ------------------------------------------------------------------------------
def ref_ints(y, p32, threshold=0.5):
    y = np.asarray(y).astype(np.int64)
    p32 = np.asarray(p32, np.float32)
    bits = p32.view(np.uint32).astype(np.int64)
    bits[bits == 0x80000000] = 0                                  # -0.0 ranks as +0.0
    order = np.argsort(bits, kind="stable")[::-1]
    b, ys = bits[order], y[order]
    gid = np.cumsum(np.r_[0, np.diff(b) != 0])                    # tie group of every element, scores descending
    ng = int(gid[-1]) + 1
    tp_g = np.bincount(gid[ys == 1], minlength=ng).astype(np.int64)
    fp_g = np.bincount(gid[ys != 1], minlength=ng).astype(np.int64)
    tp_before = np.cumsum(tp_g) - tp_g
    pred = p32.astype(np.float64) > threshold
    P = int((y == 1).sum())
    return {"tp": int((pred & (y == 1)).sum()), "tn": int((~pred & (y != 1)).sum()),
            "fp": int((pred & (y != 1)).sum()), "fn": int((~pred & (y == 1)).sum()),
            "n_pos": P, "n_neg": int(y.size - P), "n_thresholds": ng,
            "auc_num2": int(np.sum(fp_g * (2 * tp_before + tp_g))), "tie_mix": int(np.sum(tp_g * fp_g))}


def ref_bce(y, p32):
    q = np.clip(np.asarray(p32, np.float32).astype(np.float64), 1e-7, 1 - 1e-7)
    return float(np.mean(-np.where(np.asarray(y) == 1, np.log(q + 1e-7), np.log(1 - q + 1e-7))))


def device(y, p32, dev, threshold=0.5, groups=None, G=0):
    return classification_metrics_device(torch.as_tensor(np.asarray(y, np.float32), device=dev),
                                         torch.as_tensor(np.asarray(p32, np.float32), device=dev), threshold,
                                         None if groups is None else torch.as_tensor(groups, device=dev), G)


def check_slot(got, y, p32, threshold=0.5):
    """One slot's dict against the numpy reference of (y, p32) at the module's bars."""
    y, p32 = np.asarray(y), np.asarray(p32, np.float32)
    ri = ref_ints(y, p32, threshold)
    for k in INT_KEYS:
        assert got[k] == ri[k], (k, got[k], ri[k])
    P, N, n = ri["n_pos"], ri["n_neg"], y.size
    assert got["status"] == (0 if P else L.CLF_ST_NO_POS) | (0 if N else L.CLF_ST_NO_NEG), got["status"]
    bce = ref_bce(y, p32)
    print(f"n={n} thresholds={ri['n_thresholds']} bce device {got['bce']!r} numpy {bce!r}")
    assert abs(got["bce"] - bce) <= n * 2.0 ** -50 * abs(bce)
    if P == 0 or N == 0:
        assert np.isnan(got["roc_auc"])
        assert np.isnan(got["recall"]) == (P == 0) and np.isnan(got["specificity"]) == (N == 0)
        assert np.isnan(got["aupr"]) == (P == 0)
        return ri
    assert got["roc_auc"] == ri["auc_num2"] / (2 * P * N)                      # one fp64 division: bitwise
    rd = classification_metrics(y, p32, threshold)
    print(f"  roc_auc device {got['roc_auc']!r} host {rd['roc_auc']!r}")
    print(f"  aupr device {got['aupr']!r} host {rd['aupr']!r}")
    assert abs(got["roc_auc"] - rd["roc_auc"]) <= 4 * 2.0 ** -53 * ri["n_thresholds"]   # the host's trapezoid sum
    assert abs(got["aupr"] - rd["aupr"]) <= 4 * ri["n_thresholds"] * 2.0 ** -53
    for k in ("accuracy", "recall", "precision", "specificity", "f1"):
        if np.isnan(rd[k]):
            assert np.isnan(got[k]), k
        else:
            assert got[k] == rd[k], (k, got[k], rd[k])                         # single divisions of exact integers
    return ri


# ---- 1. the bundled evaluations ---------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_bundled_evaluations(k, golden, cuda):
    ev = golden(f"fold{k}_eval.npz")
    y, p = ev["y_true"], ev["probs32"]
    assert p.dtype == np.float32 and p.size in (1050, 1053)
    got = device(y, p, cuda)
    ri = check_slot(got, y, p)
    assert 1045 <= ri["n_thresholds"] <= 1051 and ri["n_thresholds"] < p.size          # tie groups are in there
    assert abs(got["roc_auc"] - float(ev["roc_auc"])) <= 2.0 ** -52


# ---- 2. saturation ties -------------------------------------------------------------------------------
def test_saturation_ties(cuda):
    rng = np.random.default_rng(0)
    n = 4000
    y = rng.random(n) < 0.6
    p = (1.0 / (1.0 + np.exp(-12.0 * rng.standard_normal(n)))).astype(np.float32)
    ones = p == np.float32(1.0)
    assert ones.sum() > 100 and 0 < y[ones].sum() < ones.sum()                  # saturated, both labels among them
    ri = ref_ints(y, p)
    assert ri["tie_mix"] > 0                # a strict or an optimistic tie rule would change auc_num2
    assert ri["n_thresholds"] < n
    check_slot(device(y, p, cuda), y, p)


# ---- 3. boundaries ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quantised():
    """20001 scores on 16 levels (k / 16: 0.0 and the threshold 0.5 among them), a -0.0 beside the +0.0s."""
    rng = np.random.default_rng(7)
    n = 20001
    p = (np.floor(rng.random(n) * 16) / 16).astype(np.float32)
    y = (rng.random(n) < 0.25 + 0.5 * p).astype(np.int64)
    p[5] = np.float32(-0.0)
    p[6] = np.float32(0.0)
    p[7] = np.float32(0.5)
    y[5], y[6], y[7] = 1, 0, 1
    return y, p


@pytest.mark.parametrize("n", [20001, SMALL, SMALL + 1, 1025, 1024])
def test_tie_runs_across_boundaries(n, quantised, cuda):
    """Long tie runs across every workgroup boundary of the general path (n = 20001: tiles of 1024), and the two
    sides of the path threshold on one input's prefix: both paths give numpy's integers."""
    y, p = quantised[0][:n], quantised[1][:n]
    got = device(y, p, cuda)
    ri = check_slot(got, y, p)
    assert ri["n_thresholds"] == 16 and ri["tie_mix"] > 0          # -0.0 and +0.0 are one threshold
    assert np.signbit(p[5]) and p[7] == 0.5
    # p == threshold is predicted negative: element 7 (label 1, p = 0.5) is a false negative
    at = ref_ints(y, p, 0.5)
    above = ref_ints(y, np.where(p == 0.5, np.float32(0.5625), p), 0.5)
    assert above["tp"] > at["tp"] == got["tp"]


def test_general_path_more_tiles_than_one_scan_pass(cuda):
    """n = 1.1M: more than 1024 tiles, so the scan of the tile aggregates carries across its own passes, and every
    thread of the last reduction adds several tile partials."""
    rng = np.random.default_rng(13)
    n = 1_100_000
    p = (np.floor(rng.random(n) * 3000) / 3000).astype(np.float32)
    y = (rng.random(n) < p).astype(np.int64)
    ri = check_slot(device(y, p, cuda), y, p)
    assert ri["n_thresholds"] == 3000 and ri["tie_mix"] > 0 and ri["auc_num2"] > 2 ** 32


def test_tiny_inputs(cuda):
    got = device([1], [0.75], cuda)
    check_slot(got, [1], [0.75])
    assert got["status"] == L.CLF_ST_NO_NEG and got["tp"] == 1 and got["n_thresholds"] == 1
    got = device([0], [0.75], cuda)
    assert got["status"] == L.CLF_ST_NO_POS and got["fp"] == 1
    got = device([1, 0], [0.25, 0.25], cuda)                        # one tie group: half a pair
    check_slot(got, [1, 0], [0.25, 0.25])
    assert got["auc_num2"] == 1 and got["roc_auc"] == 0.5
    got = device([0, 1], [0.25, 0.75], cuda)
    check_slot(got, [0, 1], [0.25, 0.75])
    assert got["auc_num2"] == 2 and got["roc_auc"] == 1.0
    got = device([1, 0], [0.25, 0.75], cuda)
    assert got["auc_num2"] == 0 and got["roc_auc"] == 0.0


# ---- 4. slots -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3000, 6000])
def test_slots(n, cuda):
    rng = np.random.default_rng(11)
    p = (np.round(rng.random(n) * 200) / 200).astype(np.float32)          # ties inside and across the slots
    y = (rng.random(n) < p).astype(np.int64)
    g = rng.integers(0, 4, n).astype(np.int32)                            # ids 2 and 3: slot 0 only
    slots = device(y, p, cuda, groups=g, G=2)
    assert len(slots) == 3
    check_slot(slots[0], y, p)
    for s in (0, 1):
        check_slot(slots[1 + s], y[g == s], p[g == s])
    assert slots[1]["n_pos"] + slots[1]["n_neg"] + slots[2]["n_pos"] + slots[2]["n_neg"] < n
    # a slot with one class only: counts still right, roc_auc NaN, the status bit says why
    y1 = y.copy()
    y1[g == 1] = 1
    slots = device(y1, p, cuda, groups=g, G=2)
    check_slot(slots[0], y1, p)
    check_slot(slots[1], y1[g == 0], p[g == 0])
    check_slot(slots[2], y1[g == 1], p[g == 1])
    assert slots[2]["status"] == L.CLF_ST_NO_NEG and np.isnan(slots[2]["roc_auc"]) and slots[2]["n_neg"] == 0
    assert slots[0]["status"] == 0 and slots[1]["status"] == 0
    # an empty slot
    slots = device(y, p, cuda, groups=np.where(g == 1, 3, g).astype(np.int32), G=2)
    assert slots[2]["n_pos"] == slots[2]["n_neg"] == 0 and slots[2]["status"] == L.CLF_ST_NO_POS | L.CLF_ST_NO_NEG
    check_slot(slots[1], y[g == 0], p[g == 0])
    # a NaN probability, a probability outside [0, 1] and a label outside {0, 1} each set bit 2, in their slots
    for bad_p, bad_y in ((np.float32("nan"), 1), (np.float32(1.5), 0), (np.float32(0.5), 2)):
        pb, yb = p.copy(), y.copy()
        i = int(np.flatnonzero(g == 0)[3])
        pb[i], yb[i] = bad_p, bad_y
        slots = device(yb, pb, cuda, groups=g, G=2)
        assert slots[0]["status"] & L.CLF_ST_BAD_INPUT and slots[1]["status"] & L.CLF_ST_BAD_INPUT
        assert not slots[2]["status"] & L.CLF_ST_BAD_INPUT
        check_slot(slots[2], y[g == 1], p[g == 1])


# ---- 5. repeatability -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, 20001])
def test_two_calls_are_bitwise_equal(n, quantised, cuda):
    rng = np.random.default_rng(3)
    p = torch.as_tensor(rng.random(n).astype(np.float32), device=cuda)
    y = torch.as_tensor(quantised[0][:n].astype(np.float32), device=cuda)
    g = torch.as_tensor(rng.integers(0, 3, n).astype(np.int32), device=cuda)
    c1, v1 = ops.clf_metrics(p, y, g, 2)
    c2, v2 = ops.clf_metrics(p, y, g, 2)
    assert torch.equal(c1, c2)
    assert torch.equal(v1.view(torch.int64), v2.view(torch.int64))        # the bits, NaN or not
    assert not torch.isnan(v1).any()


# ---- keep_best kernel -----------------------------------------------------------------------------------
def test_keep_best_kernel(cuda):
    """Strict improvement, the first occurrence wins, a NaN never improves; the copy follows the flag."""
    n = 5000
    f64 = dict(dtype=torch.float64, device=cuda)
    i32 = dict(dtype=torch.int32, device=cuda)
    for mode, seq, want in ((0, [float("nan"), 0.5, 0.5, 0.7, float("nan"), 0.7, 0.6], [0, 1, 0, 1, 0, 0, 0]),
                            (1, [0.5, float("nan"), 0.4, 0.4, 0.45, 0.1], [1, 0, 1, 0, 0, 1])):
        best = torch.zeros(n, device=cuda)
        bv, be, imp = torch.full((1,), float("nan"), **f64), torch.full((1,), -1, **i32), torch.zeros(1, **i32)
        kept = None
        for e, (v, w) in enumerate(zip(seq, want)):
            params = torch.full((n,), float(e + 1), device=cuda)
            ops.keep_best(params, best, torch.tensor([v], **f64), mode, bv, be, torch.tensor([e], **i32), imp)
            assert int(imp.item()) == w, (mode, e)
            if w:
                kept = e
            assert int(be.item()) == (-1 if kept is None else kept)
            assert torch.equal(best, torch.full((n,), 0.0 if kept is None else float(kept + 1), device=cuda))
        assert float(bv.item()) == seq[kept]


# ---- 6. evaluate ----------------------------------------------------------------------------------------
def test_evaluate_fold0(golden, cuda):
    d, ev = golden("fold0_data.npz"), golden("fold0_eval.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 0)
    model.load_weights("tests/golden/weights_fold0.npz")
    adj = get_adj_mats(np.concatenate([d["X_train"], d["X_test"]]), N_ENT, N_REL)      # IDDGCN_eval.py:49-50
    Xt = np.concatenate([d["X_test"], d["neg_X_test"]])[None]
    x = [np.arange(N_ENT)[None], Xt[:, :, 0], Xt[:, :, 1], Xt[:, :, 2], adj]
    y = ev["y_true"]
    preds = model.predict(x)[0]
    assert preds.dtype == np.float32
    got = model.evaluate(x, y[None], per_relation=True)
    check_slot(got, y, preds)
    assert abs(got["roc_auc"] - float(ev["roc_auc"])) <= 1e-4           # the parity bar on the probabilities
    rel = Xt[0, :, 1]
    assert set(np.unique(rel)) == {0, 1}
    for r in range(N_REL):
        sl = got[f"relation_{r}"]
        if r < 2:
            check_slot(sl, y[rel == r], preds[rel == r])
            host = classification_metrics(y[rel == r], preds[rel == r])
            assert all(sl[k] == host[k] for k in ("tp", "tn", "fp", "fn"))
        else:
            assert sl["n_pos"] == sl["n_neg"] == 0 and sl["status"] == L.CLF_ST_NO_POS | L.CLF_ST_NO_NEG
    plain = model.evaluate(x, y)
    assert "relation_0" not in plain and all(plain[k] == got[k] for k in plain)


# ---- 7 / 8. validation inside fit, keep_best --------------------------------------------------------------
EPOCHS = 8
N_SYN, R_SYN = 600, 2


def _syn_model():
    return get_IDDGCN_Model(N_SYN, R_SYN, 64, 64, 5, None, 0, 0, init="independent")


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


@pytest.fixture(scope="module")
def syn(cuda):
    """The synthetic graph split into training edges and 300 held-out scored pairs, and model B's trajectory: eight
    fit(epochs=1) calls, each followed by evaluate on the held-out pairs (the reference every fit below is held to)."""
    pos, neg = synthetic_graph(N_SYN, R_SYN, 3000, seed=3)
    rng = np.random.default_rng(1)
    vp, vn = rng.permutation(len(pos))[:150], rng.permutation(len(neg))[:150]
    tr_pos, tr_neg = np.delete(pos, vp, 0), np.delete(neg, vn, 0)
    val = np.concatenate([pos[vp], neg[vn]])
    y_val = np.r_[np.ones(150), np.zeros(150)]
    ids = np.arange(N_SYN)[None]
    x = [ids, tr_pos[None, :, 0], tr_pos[None, :, 1], tr_pos[None, :, 2], get_adj_mats(tr_pos, N_SYN, R_SYN)]
    x_val = [ids, val[None, :, 0], val[None, :, 1], val[None, :, 2], get_adj_mats(pos, N_SYN, R_SYN)]
    b = _syn_model()
    b.neg_triples = tr_neg
    evals, weights, losses = [], [], []
    for _ in range(EPOCHS):
        losses += b.fit(x, None, epochs=1, verbose=0).history["loss"]
        evals.append(b.evaluate(x_val, y_val))
        weights.append(b.get_weights())
    return {"x": x, "x_val": x_val, "y_val": y_val, "neg": tr_neg, "evals": evals, "weights": weights,
            "losses": losses}


def _fit(syn, **kw):
    m = _syn_model()
    m.neg_triples = syn["neg"]
    assert m.use_graph
    return m, m.fit(syn["x"], None, epochs=EPOCHS, verbose=0, **kw).history


def _weights_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_fit_validation_equals_evaluate_per_epoch(syn, cuda):
    a, ha = _fit(syn, validation_data=(syn["x_val"], syn["y_val"]))
    keys = set(syn["evals"][0])
    assert {"roc_auc", "aupr", "accuracy", "f1", "bce", "auc_num2", "tp"} <= keys
    for k in keys:
        assert len(ha[f"val_{k}"]) == EPOCHS
        for e in range(EPOCHS):
            assert _same(ha[f"val_{k}"][e], syn["evals"][e][k]), (k, e, ha[f"val_{k}"][e], syn["evals"][e][k])
    assert ha["val_loss"] == ha["val_bce"]
    assert not any(np.isnan(v) for v in ha["val_roc_auc"])
    # validation changes nothing of the training: weights and losses are bitwise those of a fit without it
    c, hc = _fit(syn)
    assert set(hc) == {"loss"}
    assert ha["loss"] == hc["loss"] == syn["losses"]
    assert _weights_equal(a.get_weights(), c.get_weights())
    assert _weights_equal(a.get_weights(), syn["weights"][-1])


def test_fit_validation_freq(syn, cuda):
    _, h = _fit(syn, validation_data=(syn["x_val"], syn["y_val"]), validation_freq=3)
    assert len(h["loss"]) == EPOCHS
    for k in ("roc_auc", "aupr", "bce", "auc_num2", "tp"):
        assert len(h[f"val_{k}"]) == 2
        assert _same(h[f"val_{k}"][0], syn["evals"][2][k]) and _same(h[f"val_{k}"][1], syn["evals"][5][k]), k


def test_fit_validation_logs_reach_callbacks(syn, cuda):
    """With a user callback the val_* logs are floats each validating epoch, and it can stop the training."""
    seen = []

    class Stop(Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))
            if epoch == 3:
                self.model.stop_training = True

    _, h = _fit(syn, validation_data=(syn["x_val"], syn["y_val"]), validation_freq=2, callbacks=[Stop()])
    assert len(seen) == 4 and len(h["loss"]) == 4
    assert "val_roc_auc" not in seen[0] and "val_roc_auc" not in seen[2]
    for i, e in ((1, 1), (3, 3)):
        assert isinstance(seen[i]["val_roc_auc"], float) and isinstance(seen[i]["val_loss"], float)
        for k in ("roc_auc", "aupr", "bce", "auc_num2"):
            assert _same(seen[i][f"val_{k}"], syn["evals"][e][k]), (k, e)


@pytest.mark.parametrize("key,metric,pick", [("val_roc_auc", "roc_auc", np.argmax), ("val_loss", "bce", np.argmin)])
def test_keep_best(key, metric, pick, syn, cuda):
    a, h = _fit(syn, validation_data=(syn["x_val"], syn["y_val"]), keep_best=key)
    series = [e[metric] for e in syn["evals"]]
    best = int(pick(series))                                       # numpy's argmax / argmin: the first occurrence
    print(key, series, "best epoch", best + 1)
    assert a.best_epoch == best + 1 and a.best_value == series[best]
    assert _weights_equal(a.get_weights(), syn["weights"][best])
    assert h[key] == [e[metric] for e in syn["evals"]]


def test_keep_best_restores_an_earlier_epoch(syn, cuda):
    """The two keys above may well peak at the last epoch, where keeping nothing would pass too: take the keys
    whose best epoch in B's trajectory is NOT the last one (chosen from B, the reference) and hold the final weights
    to B's weights after that epoch, which differ from the last epoch's."""
    picked = []
    for name in L.CLF_VALUES:
        series = [e[name] for e in syn["evals"]]
        if any(np.isnan(series)):
            continue
        best = int(np.argmin(series) if name == "bce" else np.argmax(series))
        print(name, series, "best epoch", best + 1)
        if best < EPOCHS - 1 and len(picked) < 2:
            picked.append((name, best, series[best]))
    assert picked, "no metric of B's trajectory peaks before the last epoch"
    for name, best, value in picked:
        a, _ = _fit(syn, validation_data=(syn["x_val"], syn["y_val"]), keep_best=f"val_{name}")
        assert a.best_epoch == best + 1 and a.best_value == value, (name, a.best_epoch, best + 1)
        assert _weights_equal(a.get_weights(), syn["weights"][best]), name
        assert not _weights_equal(a.get_weights(), syn["weights"][-1]), name
