"""The CPU oracle against the reference's own bundled files (pinning)."""
import numpy as np
import pytest
import torch

from oracle.ref_model import KerasAdam, eval_metrics, predict, train_step_grads
from oracle.ref_utils import generate_reverse_triplets, get_adj_coo, get_y_true, make_fold_files
from tests.conftest import REFERENCE

N_ENT, N_REL = 845, 4


@pytest.mark.parametrize("k", range(5))
def test_split_restatement_reproduces_bundled_folds(k, golden):
    """IDDGCN.py:312-373 + utils1.py:741-867 restated -> the bundled fold files, bit for bit."""
    f = make_fold_files(REFERENCE, k)
    g = golden(f"fold{k}_data.npz")
    for name in ("X_train", "X_test", "neg_X_test"):
        assert np.array_equal(f[name].astype(np.int64), g[name].astype(np.int64)), name
    assert np.array_equal(f["X_train_neg"][0].astype(np.int64), g["X_train_neg"].astype(np.int64))


@pytest.mark.parametrize("k", range(5))
def test_oracle_eval_on_bundled_weights(k, golden):
    """IDDGCN_eval.py with fold=k on the reference's trained weights: oracle probs == fixture."""
    d, w, ev = golden(f"fold{k}_data.npz"), golden(f"weights_fold{k}.npz"), golden(f"fold{k}_eval.npz")
    adj = get_adj_coo(np.concatenate([d["X_train"], d["X_test"]]), N_ENT, N_REL)
    Xt = np.concatenate([d["X_test"], d["neg_X_test"]]).astype(np.int64)
    p = predict(w, Xt, adj, N_ENT)
    np.testing.assert_allclose(p, ev["probs"], rtol=0, atol=1e-12)
    y = get_y_true(d["X_test"], Xt)
    assert np.array_equal(y, ev["y_true"])
    m = eval_metrics(y, p)
    assert abs(m["roc_auc"] - float(ev["roc_auc"])) < 1e-12
    # trained weights give a real classifier: only a correct forward restatement does
    assert m["roc_auc"] > 0.87


def test_fold0_auc_value(golden):
    ev = golden("fold0_eval.npz")
    assert abs(float(ev["roc_auc"]) - 0.9072) < 5e-4


def test_reverse_triplets_and_adjacency_order():
    tr = np.array([[3, 0, 1], [1, 0, 3], [2, 1, 2], [0, 0, 5], [3, 0, 1]])
    rev = generate_reverse_triplets(tr)
    assert rev.tolist() == [[1, 0, 3], [3, 0, 1], [5, 0, 0], [1, 0, 3]]
    adj = get_adj_coo(tr, 6, 3)
    assert adj[0][0].tolist() == [[0, 5], [1, 3], [3, 1]]          # sorted unique, duplicates merged
    assert adj[1][0].tolist() == [[2, 2]]
    assert adj[2][0].tolist() == [[0, 0]] and adj[2][1].tolist() == [0.0]   # empty relation placeholder


def test_fold0_step_fixture_consistency(golden):
    """Re-derive a few gradients of the fold-0 step fixture (float64 autograd)."""
    g = golden("fold0_step.npz")
    d, w = golden("fold0_data.npz"), golden("weights_fold0.npz")
    adj = get_adj_coo(d["X_train"], N_ENT, N_REL)
    loss, scores, grads = train_step_grads(w, d["X_train"][:4000], d["X_train_neg"][:300], adj, N_ENT)
    assert np.isfinite(loss) and scores.shape == (4300,)
    assert float(g["loss"]) > 0 and g["grad_E"].shape == (845, 64)
    assert "grad_relw1" not in g  # relation_weights receive no gradient (unused in call)


def test_keras_adam_matches_formula():
    opt = KerasAdam()
    p = {"S1": np.ones(3), "E": np.ones(3)}
    g = {"S1": np.array([0.1, -0.2, 0.0]), "E": np.array([0.1, -0.2, 0.0])}
    out = opt.step(p, g)
    # first step: m = 0.1 g, v = 0.001 g^2, alpha = lr sqrt(.001)/.1 -> update = lr * g/|g| (eps-damped)
    upd = 1 - out["S1"]
    np.testing.assert_allclose(upd[:2], 1e-3 * np.sign(g["S1"][:2]), rtol=1e-4)
    assert upd[2] == 0.0
    np.testing.assert_allclose(out["E"], out["S1"], rtol=1e-12)


def test_synth_fixture_grads_torch_consistency(golden):
    s = golden("synth_small.npz")
    params = {k[6:]: v for k, v in s.items() if k.startswith("param_")}
    adj = get_adj_coo(s["triples"], int(s["N"]), int(s["R"]))
    loss, scores, grads = train_step_grads(params, s["triples"], s["neg"], adj, int(s["N"]))
    assert abs(loss - float(s["loss"])) < 1e-12
    for k, v in grads.items():
        np.testing.assert_allclose(v, s[f"grad_{k}"], rtol=1e-10, atol=1e-15)


def test_similarity_oracle_reproduces_reference_outputs(golden):
    """oracle/ref_similarity.py against the reference's own mu_similar0.97.csv / drug_similar0.78.csv
    (as committed in tests/golden/similarity.npz, and as the csv files under tests/golden/prediction_datasets)."""
    import pandas as pd

    from oracle.ref_similarity import similar_triples
    g = golden("similarity.npz")
    assert np.array_equal(similar_triples(g["mu_feat"], 0.97, 3, 0), g["mu_triples"])
    assert np.array_equal(similar_triples(g["drug_feat"], 0.78, 2, 661), g["drug_triples"])
    ref = REFERENCE
    assert np.array_equal(pd.read_csv(f"{ref}/mu_similar0.97.csv", header=None).to_numpy(), g["mu_triples"])
    assert np.array_equal(pd.read_csv(f"{ref}/drug_similar0.78.csv", header=None).to_numpy(), g["drug_triples"])
