/*
 * iddgcn_screen.h — all-candidate link ranking of libiddgcn_hip.so (ABI 13).
 *
 * A query is a triple (h, r, t) and a side: the tail side scores (h, r, c) for every entity c in [0, N), the head
 * side scores (c, r, t).  The score is the model's pre-sigmoid DistMult logit (IDDGCN.py:108).  The head chain and
 * the dynamic weights are node tables (X^l, W^l), and a scored edge's tail chain depends only on the tail node's
 * tables and the head's weights, so with w_l = W^l[head], P^l_r = AE_r K^l_r and ES1 = E S^1
 *
 *     x1 = sigmoid(ES1[tail] + sum_r w_1r P^1_r[tail])
 *     x2 = sigmoid(x1 S^2    + sum_r w_2r P^2_r[tail])
 *     x3 = sigmoid(x2 S^3    + sum_r w_3r P^3_r[tail])
 *     s  = sum_d X^3[head][d] rel[r][d] x3[d]
 *
 * where (head, tail) = (query node, c) on the tail side and (c, query node) on the head side.
 *
 * Conventions as in iddgcn.h (device pointers, caller-owned buffers, no synchronisation; 0 on success, a
 * hipError_t (> 0), or IDDGCN_E_* (< 0) with nothing launched).
 */
#ifndef IDDGCN_SCREEN_H_
#define IDDGCN_SCREEN_H_

#ifdef __cplusplus
extern "C" {
#endif

#define IDDGCN_SCREEN_TAIL 0   /* candidates are tails: head = q_node[q], tail = c */
#define IDDGCN_SCREEN_HEAD 1   /* candidates are heads: head = c, tail = q_node[q] */
#define IDDGCN_TOPK_MAX 64

/* s[q * N + c] = logit of query q against candidate c, q < Q, c < N: the three-layer tail chain and DistMult in
 * one kernel (S^2, S^3 resident in registers, the activations in LDS; 4 bytes written per candidate).
 *   d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL); Q >= 0, N >= 1, side one of IDDGCN_SCREEN_*.
 *   q_node[Q] in [0, N), q_rel[Q] in [0, R): int32, validated by the caller.
 *   ES1 (N, d); P: P^l_r at P + (l-1) * p_layer_stride + r * p_rel_stride, (N, d) rows of d floats;
 *   W: W^l at W + (l-1) * w_layer_stride, (N, R); X3 (N, d); S2, S3 (d, d); rel (R, d).  All fp32.
 *   ES1 and P are read as 16-byte vectors: both 16-byte aligned, p_layer_stride and p_rel_stride multiples of 4
 *   floats (IDDGCN_E_BAD_ARG otherwise).
 * The sum order within a row is fixed: it depends neither on Q, nor on the row's tile, nor on the other queries of
 * the launch. */
int iddgcn_screen_chain_f32(void* stream, int Q, int N, int d, int R, int side, const int* q_node, const int* q_rel,
                            const float* ES1, const float* P, long long p_layer_stride, long long p_rel_stride,
                            const float* W, long long w_layer_stride, const float* X3, const float* S2,
                            const float* S3, const float* rel, float* s);

/* Per-query selection over s (Q, N), which is not modified.
 *   target[Q]: int32 in [-1, N); -1 = no target.
 *   filter (optional: fptr and fidx both null, or both given): CSR over the queries, fptr[Q + 1], fidx the candidate
 *     ids left out of query q, ascending and without duplicates within a query.  The target is exempt from it.
 *   greater[q] / equal[q]: the non-filtered c != target with s_c > s_target / s_c == s_target (0 without a target).
 *   topk_idx (Q, k) int32, topk_val (Q, k) fp32: the k best non-filtered candidates, descending by value, ties by
 *     ascending id (IEEE comparison: -0.0 == +0.0), padded with -1 / -inf.  1 <= k <= IDDGCN_TOPK_MAX.
 * One workgroup per query walks the row in passes; no atomics: the result is deterministic.  Invalid sizes
 * (Q < 0, N < 1, k out of range) or a null required pointer: IDDGCN_E_BAD_ARG. */
int iddgcn_rank_topk_f32(void* stream, int Q, int N, int k, const float* s, const int* target, const int* fptr,
                         const int* fidx, int* greater, int* equal, int* topk_idx, float* topk_val);

#ifdef __cplusplus
}
#endif

#endif /* IDDGCN_SCREEN_H_ */
