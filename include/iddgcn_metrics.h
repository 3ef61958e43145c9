/*
 * iddgcn_metrics.h — binary-classification metrics of libiddgcn_hip.so on the device.
 *
 * The reference's evaluation block (IDDGCN_eval.py:58-122: confusion counts at a threshold, accuracy,
 * recall, precision, specificity, F1, ROC-AUC, AUPR, overall and per relation) computed where the
 * forward leaves its probabilities, so a validation pass inside a captured training loop never
 * touches the host: a sort by score, tie-aware cumulative counts, ROC-AUC as an exact 64-bit
 * integer and AUPR / BCE as fp64 sums in a fixed order.  iddgcn_keep_best_f32 keeps the parameters
 * of the best validating epoch, iddgcn_clf_history_append records one result per validating epoch.
 *
 * Conventions as in iddgcn.h / iddgcn_graph.h: device pointers, caller-owned outputs and workspace
 * (size from the *_workspace query, a pure host function), `stream` = hipStream_t as void*, return
 * 0 / a positive hipError_t / a negative IDDGCN_E_* (nothing launched).  Nothing here allocates or
 * synchronises, everything is capturable in a HIP graph, and no float atomics are used: two calls
 * on the same input give bitwise the same output.
 */
#ifndef IDDGCN_METRICS_H_
#define IDDGCN_METRICS_H_

#ifdef __cplusplus
extern "C" {
#endif

/* n <= IDDGCN_CLF_SMALL_MAX: one launch of 1 + G workgroups, sort and scans in LDS. */
#define IDDGCN_CLF_SMALL_MAX 4096
/* Largest G (slots beyond "all elements"). */
#define IDDGCN_CLF_MAX_GROUPS 64

/* Per slot: counts[slot * IDDGCN_CLF_N_COUNTS + IDDGCN_CLF_*], values[slot * IDDGCN_CLF_N_VALUES + IDDGCN_CLF_V_*]. */
#define IDDGCN_CLF_N_COUNTS 9
#define IDDGCN_CLF_TP 0
#define IDDGCN_CLF_TN 1
#define IDDGCN_CLF_FP 2
#define IDDGCN_CLF_FN 3
#define IDDGCN_CLF_P 4             /* labels == 1 */
#define IDDGCN_CLF_N_NEG 5         /* the others */
#define IDDGCN_CLF_AUC_NUM2 6      /* sum over tie groups of fp_g * (2 * TP_before_g + tp_g) */
#define IDDGCN_CLF_N_THRESHOLDS 7  /* distinct scores */
#define IDDGCN_CLF_STATUS 8        /* IDDGCN_CLF_ST_* bits */

#define IDDGCN_CLF_ST_NO_POS 1     /* P == 0 */
#define IDDGCN_CLF_ST_NO_NEG 2     /* N_neg == 0 */
#define IDDGCN_CLF_ST_BAD_INPUT 4  /* a NaN probability, one outside [0, 1], or a label not in {0, 1} */

#define IDDGCN_CLF_N_VALUES 8
#define IDDGCN_CLF_V_ACCURACY 0
#define IDDGCN_CLF_V_RECALL 1
#define IDDGCN_CLF_V_PRECISION 2
#define IDDGCN_CLF_V_SPECIFICITY 3
#define IDDGCN_CLF_V_F1 4
#define IDDGCN_CLF_V_ROC_AUC 5
#define IDDGCN_CLF_V_AUPR 6
#define IDDGCN_CLF_V_BCE 7

/* Workspace bytes for iddgcn_clf_metrics on n elements and G groups; < 0 if n < 0, n >= 2^31, G < 0 or
 * G > IDDGCN_CLF_MAX_GROUPS.  Monotone in n. */
long long iddgcn_clf_metrics_workspace(long long n, int G);

/* The evaluation block of IDDGCN_eval.py:71-84 (sklearn's confusion counts, roc_auc_score and
 * auc(recall, precision)) on n float32 probabilities and float labels, for 1 + G slots: slot 0 is every
 * element, slot g + 1 the elements with group[i] == g; an element whose group is outside [0, G) counts in
 * slot 0 only.  group may be NULL if G == 0.
 *
 * Scores are ranked by the float32 bit pattern (-0.0 as +0.0); elements of equal score form one
 * threshold.  With the groups of equal score in descending order, tp_g / fp_g their positive /
 * negative counts and TP_before_g the positives strictly above group g,
 *   auc_num2 = sum_g fp_g * (2 * TP_before_g + tp_g)          (an exact integer)
 *   roc_auc  = auc_num2 / (2 * P * N_neg)                     (one fp64 division: the ROC trapezoid,
 *                                                              ties counted as half)
 *   aupr     = (sum_g tp_g * (prec_g + prec_{g-1}) / 2) / P,  prec_g = TP_g / (TP_g + FP_g) on inclusive
 *                                                              cumulative counts, prec_{-1} = 1
 *   bce      = mean of -[y log(q + 1e-7) + (1 - y) log(1 - q + 1e-7)], q = clip(p, 1e-7, 1 - 1e-7) in fp64
 * tp / tn / fp / fn count (double)prob > threshold as predicted positive.  The fp64 sums run in a fixed
 * order (a fixed tree inside a workgroup, workgroup partials in index order by one workgroup).  A value
 * whose denominator is zero is NaN; the status bits say why.  The integers do not depend on the path
 * (n <= IDDGCN_CLF_SMALL_MAX or above).
 *
 * counts: (1 + G) * IDDGCN_CLF_N_COUNTS long long; values: (1 + G) * IDDGCN_CLF_N_VALUES double.  n >= 1. */
int iddgcn_clf_metrics(void* stream, long long n, int G, const float* prob, const float* label,
                       const int* group, double threshold, long long* counts, double* values,
                       void* workspace, long long workspace_bytes);

/* Keep the parameters of the best epoch.  One thread compares value[0] with best_value[0] (mode 0:
 * larger is better, 1: smaller): a strict improvement, or any non-NaN value while best_epoch[0] < 0
 * (nothing kept yet), sets improved[0] = 1, best_value[0] = value[0], best_epoch[0] = epoch[0]; otherwise
 * improved[0] = 0 (a NaN never improves, an equal value keeps the earlier epoch).  A second kernel then
 * copies params -> best (n floats) if improved[0] is set; it only reads improved[0]. */
int iddgcn_keep_best_f32(void* stream, long long n, const float* params, float* best,
                         const double* value, int mode, double* best_value, int* best_epoch,
                         const int* epoch, int* improved);

/* hist_counts[counter[0]] = counts (n_counts long long), hist_values[counter[0]] = values (n_values
 * double), then counter[0] += 1; nothing is written once counter[0] >= capacity.  One workgroup. */
int iddgcn_clf_history_append(void* stream, int n_counts, int n_values, const long long* counts,
                              const double* values, long long* hist_counts, double* hist_values,
                              int capacity, int* counter);

#ifdef __cplusplus
}
#endif

#endif /* IDDGCN_METRICS_H_ */
