"""Evaluation metrics: on the host (numpy only), and the classification block on the GPU.

``classification_metrics_device`` is ``classification_metrics`` computed by iddgcn_clf_metrics on tensors that stay
on the device (what IDDGCN_Model.evaluate and fit's validation run); torch is imported only there.
``ranking_metrics`` summarises the ranks Engine.rank_candidates / IDDGCN_Model.rank_candidates return (MRR, mean
rank, Hits@k); ``classification_metrics`` is the reference's evaluation block (IDDGCN_eval.py:71-84: confusion
counts at a threshold, accuracy, recall, precision, specificity, F1, ROC-AUC, and AUPR as the trapezoid over the
precision-recall curve), computed as sklearn computes them.
"""
import numpy as np


def ranking_metrics(ranks, ks=(1, 3, 10)):
    """{"mrr", "mean_rank", "hits@k" for k in ks, "n"} of 1-based ranks (fractional ranks, the mean of the
    optimistic and pessimistic rank of a tied target, count as they are: hits@k is rank <= k)."""
    r = np.asarray(ranks, dtype=np.float64).ravel()
    if r.size == 0:
        raise ValueError("ranking_metrics: no ranks")
    if not np.all(r >= 1):
        raise ValueError("ranking_metrics: ranks are 1-based")
    out = {"mrr": float(np.mean(1.0 / r)), "mean_rank": float(np.mean(r)), "n": int(r.size)}
    for k in ks:
        out[f"hits@{int(k)}"] = float(np.mean(r <= k))
    return out


def _clf_curve(y_true, y_score):
    """Cumulative false / true positive counts at every distinct score, scores descending."""
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y, s = y_true[order], y_score[order]
    idx = np.r_[np.flatnonzero(np.diff(s)), y.size - 1]
    tps = np.cumsum(y, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps


def _trapezoid(x, y):
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def classification_metrics(y_true, y_prob, threshold=0.5):
    """IDDGCN_eval.py:71-84 on labels in {0, 1} and predicted probabilities: tp, tn, fp, fn at
    ``y_prob > threshold``, accuracy, recall, precision, specificity, f1, roc_auc and aupr (the area under the
    precision-recall curve by the trapezoid rule, as sklearn.metrics.auc(recall, precision))."""
    y = np.asarray(y_true).ravel().astype(np.int64)
    p = np.asarray(y_prob, dtype=np.float64).ravel()
    if y.shape != p.shape or y.size == 0:
        raise ValueError("classification_metrics: y_true and y_prob must be non-empty and of one length")
    if not np.all((y == 0) | (y == 1)) or y.min() == y.max():
        raise ValueError("classification_metrics: labels must be 0 / 1 with both classes present")
    pred = p > threshold
    tp, tn = int(np.sum(pred & (y == 1))), int(np.sum(~pred & (y == 0)))
    fp, fn = int(np.sum(pred & (y == 0))), int(np.sum(~pred & (y == 1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        recall, precision = np.float64(tp) / (tp + fn), np.float64(tp) / (tp + fp)
        f1 = 2 * precision * recall / (precision + recall)
    fps, tps = _clf_curve(y, p)
    # ROC: (0, 0) first, rates by the totals
    roc_auc = _trapezoid(np.r_[0.0, fps] / fps[-1], np.r_[0.0, tps] / tps[-1])
    # precision-recall: thresholds ascending (recall descending), closed by (recall 0, precision 1)
    prec = np.r_[(tps / (tps + fps))[::-1], 1.0]
    reca = np.r_[(tps / tps[-1])[::-1], 0.0]
    return {"tp": tp, "tn": tn, "fp": fp, "fn": fn,
            "accuracy": (tn + tp) / (tn + fp + fn + tp),
            "recall": float(recall), "precision": float(precision),
            "specificity": tn / (tn + fp), "f1": float(f1),
            "roc_auc": roc_auc, "aupr": -_trapezoid(reca, prec)}


def slot_dicts(counts, values):
    """The (slots, 9) integer and (slots, 8) double outputs of iddgcn_clf_metrics (host arrays or lists) as one dict
    per slot: classification_metrics' keys plus bce, auc_num2, n_thresholds, n_pos, n_neg and status."""
    from ._lib import CLF_COUNTS, CLF_VALUES
    out = []
    for c, v in zip(counts, values):
        d = {k: int(x) for k, x in zip(CLF_COUNTS, c)}
        d.update({k: float(x) for k, x in zip(CLF_VALUES, v)})
        out.append(d)
    return out


def classification_metrics_device(y_true, y_prob, threshold=0.5, groups=None, num_groups=0):
    """classification_metrics on the GPU (iddgcn_clf_metrics): ``y_prob`` a float32 CUDA tensor, ``y_true`` a CUDA
    tensor of 0 / 1 labels, both left on the device; the one host read is the result.  Returns the dict of every
    element: classification_metrics' keys, plus ``bce`` (the mean Keras binary cross-entropy), ``auc_num2`` (the
    exact integer with roc_auc = auc_num2 / (2 n_pos n_neg)), ``n_thresholds`` (distinct scores), ``n_pos``,
    ``n_neg`` and ``status``.  With ``groups`` (int CUDA tensor) and ``num_groups`` = G it returns a list of 1 + G such
    dicts: every element, then the elements of group 0 .. G - 1 (an id outside [0, G) counts in the first only).

    Scores are ranked by their float32 bits, as the reference ranks model.predict's output.  Unlike the host
    function this does not raise on a set with one class only: the ratios without a denominator are NaN and
    ``status`` says why (1: no positives, 2: no negatives, 4: a NaN / out-of-range probability or a label outside
    {0, 1} was seen)."""
    import torch

    from . import ops
    if not (isinstance(y_prob, torch.Tensor) and y_prob.is_cuda and y_prob.dtype == torch.float32):
        raise ValueError("classification_metrics_device: y_prob must be a float32 CUDA tensor")
    if not (isinstance(y_true, torch.Tensor) and y_true.is_cuda):
        raise ValueError("classification_metrics_device: y_true must be a CUDA tensor")
    p = y_prob.reshape(-1).contiguous()
    y = y_true.reshape(-1).to(torch.float32).contiguous()
    if p.numel() == 0 or p.numel() != y.numel():
        raise ValueError("classification_metrics_device: y_true and y_prob must be non-empty and of one length")
    G = int(num_groups) if groups is not None else 0
    g = None
    if groups is not None:
        if G < 1:
            raise ValueError("classification_metrics_device: groups needs num_groups >= 1")
        g = groups.reshape(-1).to(torch.int32).contiguous()
        if g.numel() != p.numel():
            raise ValueError("classification_metrics_device: groups must be as long as y_prob")
    counts, values = ops.clf_metrics(p, y, g, G, threshold)
    d = slot_dicts(counts.cpu().tolist(), values.cpu().tolist())
    return d if groups is not None else d[0]
