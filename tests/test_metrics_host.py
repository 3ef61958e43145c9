"""Host side of the device classification metrics (no GPU): the symbols of include/iddgcn_metrics.h, the workspace
query, the rejections before any launch, and the argument checks of IDDGCN_Model.evaluate / fit(validation_data=...)."""
import os
import re

import numpy as np
import pytest

from iddgcn_amd import _lib, classification_metrics_device, get_IDDGCN_Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iddgcn_metrics.h")


def test_header_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 13 and lib.iddgcn_abi_version() == 13       # added symbols only: no bump
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(iddgcn_\w+)\s*\(", text))
    assert declared == {"iddgcn_clf_metrics_workspace", "iddgcn_clf_metrics", "iddgcn_keep_best_f32",
                        "iddgcn_clf_history_append"}
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the constants mirrored in _lib are the header's
    defs = dict(re.findall(r"#define\s+(IDDGCN_CLF_\w+)\s+(\d+)", text))
    assert int(defs["IDDGCN_CLF_SMALL_MAX"]) == _lib.CLF_SMALL_MAX >= 4096
    assert int(defs["IDDGCN_CLF_MAX_GROUPS"]) == _lib.CLF_MAX_GROUPS
    assert int(defs["IDDGCN_CLF_N_COUNTS"]) == len(_lib.CLF_COUNTS)
    assert int(defs["IDDGCN_CLF_N_VALUES"]) == len(_lib.CLF_VALUES)
    for i, k in enumerate(("TP", "TN", "FP", "FN", "P", "N_NEG", "AUC_NUM2", "N_THRESHOLDS", "STATUS")):
        assert int(defs[f"IDDGCN_CLF_{k}"]) == i
    for i, k in enumerate(_lib.CLF_VALUES):
        assert int(defs[f"IDDGCN_CLF_V_{k.upper()}"]) == i


def test_workspace_query():
    ws = _lib.load().iddgcn_clf_metrics_workspace
    assert ws(-1, 0) < 0 and ws(10, -1) < 0 and ws(-5, -5) < 0
    assert ws(1 << 31, 0) < 0 and ws(10, _lib.CLF_MAX_GROUPS + 1) < 0
    ns = [0, 1, 2, 1053, _lib.CLF_SMALL_MAX, _lib.CLF_SMALL_MAX + 1, 5000, 20001, 10 ** 6, 4 * 10 ** 6, (1 << 31) - 1]
    for G in (0, 2, _lib.CLF_MAX_GROUPS):
        sizes = [ws(n, G) for n in ns]
        assert all(s >= 0 for s in sizes), (G, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (G, sizes)           # monotone in n
        assert sizes[ns.index(_lib.CLF_SMALL_MAX)] == 0 < sizes[ns.index(_lib.CLF_SMALL_MAX + 1)]
    assert ws(20001, 2) > ws(20001, 0)
    # the general path holds the radix sort's own workspace
    assert ws(20001, 0) > _lib.load().iddgcn_radix_sort_workspace(20001, 8)


def test_rejections_before_launch():
    lib = _lib.load()
    # null stream, null pointers: every rejection happens on the host, before any launch
    assert lib.iddgcn_clf_metrics(None, 10, 0, None, None, None, 0.5, None, None, None, 0) == -3
    assert lib.iddgcn_clf_metrics(None, -1, 0, None, None, None, 0.5, None, None, None, 0) == -3
    assert lib.iddgcn_clf_metrics(None, 10, -1, None, None, None, 0.5, None, None, None, 0) == -3
    assert lib.iddgcn_keep_best_f32(None, 10, None, None, None, 0, None, None, None, None) == -3
    assert lib.iddgcn_keep_best_f32(None, -1, None, None, None, 0, None, None, None, None) == -3
    assert lib.iddgcn_clf_history_append(None, 9, 8, None, None, None, None, 4, None) == -3


def _model_and_x(B=6):
    model = get_IDDGCN_Model(20, 2, 32, 32, 1, None, 0, 0, init="independent")
    rng = np.random.default_rng(0)
    h, r, t = rng.integers(0, 20, B), rng.integers(0, 2, B), rng.integers(0, 20, B)
    return model, [np.arange(20)[None], h[None], r[None], t[None], []]


def test_evaluate_and_fit_validate_their_arguments():
    """Refused on the host, before the model asks for a GPU (none is needed to get these errors)."""
    model, x = _model_and_x(6)
    with pytest.raises(ValueError, match="one label per scored triple"):
        model.evaluate(x, np.ones((1, 5)))
    with pytest.raises(ValueError, match="one label per scored triple"):
        model.evaluate(x, np.ones(7))
    with pytest.raises(ValueError, match="one label per scored triple"):
        model.evaluate(x, np.ones((2, 3)))
    with pytest.raises(ValueError, match="keep_best must be one of"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, validation_data=(x, np.ones(6)), keep_best="val_auc")
    with pytest.raises(ValueError, match="keep_best must be one of"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, validation_data=(x, np.ones(6)), keep_best="roc_auc")
    with pytest.raises(ValueError, match="keep_best needs validation_data"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, keep_best="val_roc_auc")
    with pytest.raises(ValueError, match="one label per scored triple"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, validation_data=(x, np.ones(5)))
    with pytest.raises(ValueError, match="validation_freq"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, validation_data=(x, np.ones(6)), validation_freq=0)
    with pytest.raises(ValueError, match="x_val, y_val"):
        model.fit(x, np.ones((1, 6)), epochs=1, verbose=0, validation_data=(x,))


def test_keep_best_keys():
    model, _ = _model_and_x()
    assert model._keep_best_key("val_roc_auc") == (_lib.CLF_VALUES.index("roc_auc"), 0)
    assert model._keep_best_key("val_aupr") == (_lib.CLF_VALUES.index("aupr"), 0)
    assert model._keep_best_key("val_loss") == (_lib.CLF_VALUES.index("bce"), 1)      # the smallest loss
    assert model._keep_best_key("val_bce") == model._keep_best_key("val_loss")
    assert model.best_epoch is None and model.best_value is None


def test_device_function_refuses_host_arrays():
    with pytest.raises(ValueError, match="CUDA tensor"):
        classification_metrics_device(np.ones(4), np.ones(4, np.float32))
