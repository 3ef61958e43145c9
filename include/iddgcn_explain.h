/*
 * iddgcn_explain.h — batched explaiNE of libiddgcn_hip.so: the gradient of a triple's predicted probability w.r.t.
 * every stored adjacency value, for Q triples in a fixed number of launches.
 *
 * Every layer is fed all_e, so A_r enters the model only through AE_r = A_r E, and the prediction of (h, r, t) reads
 * only AE_r[h], AE_r[t], E[h] and E[t]:  d p / d A_r[i, j] = <dAE_r[i], E[j]>  is exactly 0 unless i is h or t.
 * Notation of iddgcn_screen.h; per query, with w_l = W^l[h], a_l = Ssm^l[h] (the softmax row), xh^l = X^l[h]:
 *
 *     x1 = sigmoid(ES1[t] + sum_r w_1r P^1_r[t]);  xt^l = sigmoid(xt^{l-1} S^l + sum_r w_lr P^l_r[t]),  l = 2, 3
 *     s = sum_d xh^3 rel[r] xt^3,  p = sigmoid(s),  g = scale p (1 - p)
 *     dxh^3 = g rel[r] * xt^3,  dxt^3 = g rel[r] * xh^3
 *     for l = 3, 2, 1:
 *         dzh = dxh^l * xh^l (1 - xh^l);  dzt = dxt^l * xt^l (1 - xt^l)
 *         GH_r += w_lr (dzh K^l_r^T);  GT_r += w_lr (dzt K^l_r^T)                 for every r
 *         if l > 1:
 *             dw_r = <dzh, P^l_r[h]> + <dzt, P^l_r[t]>
 *             da_r = dw_r w_lr (1 - w_lr);  du = a_l * (da - sum_i a_li da_i)
 *             dxh^{l-1} = dzh S^l^T + du Walpha^l^T;  dxt^{l-1} = dzt S^l^T
 *
 * GH, GT (R x d each) are the query's own dAE_r[h] and dAE_r[t]; the gradient w.r.t. entry (i, j) of A_r is
 * <GH_r, E[j]> for i == h, <GT_r, E[j]> for i == t, <GH_r + GT_r, E[j]> for h == t == i.
 *
 * Conventions as in iddgcn.h (device pointers, caller-owned buffers, no synchronisation; 0 on success, a
 * hipError_t (> 0), or IDDGCN_E_* (< 0) with nothing launched).  No float atomics: every result of a query has a
 * fixed summation order that depends neither on Q, nor on the query's place in the batch, nor on the other queries.
 * The library's ABI version is unchanged by these entries: they only add symbols.
 */
#ifndef IDDGCN_EXPLAIN_H_
#define IDDGCN_EXPLAIN_H_

#ifdef __cplusplus
extern "C" {
#endif

/* The tail chain and the backward above for Q queries (h[q], r[q], t[q]): int32, h and t in [0, N), r in [0, R),
 * validated by the caller.  d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL), Q >= 0, N >= 1.
 *   ES1 (N, d); P: P^l_r at P + (l-1) * p_layer_stride + r * p_rel_stride, (N, d); W, Ssm: layer l at
 *   + (l-1) * w_layer_stride, (N, R); X: X^l at X + (l-1) * x_layer_stride, (N, d); K1, K2, K3 (R, d, d);
 *   S2, S3 (d, d); Wa2, Wa3 (d, R); rel (R, d).  All fp32, exact fp32 arithmetic (fmaf chains).
 *   ES1, P and G are 16-byte aligned, the P strides multiples of 4 floats (IDDGCN_E_BAD_ARG otherwise).
 * Outputs: G (Q, 2, R, d): G[q][0] = GH, G[q][1] = GT;  p (Q). */
int iddgcn_explain_seeds_f32(void* stream, int Q, int N, int d, int R, const int* h, const int* r, const int* t,
                             float scale, const float* ES1, const float* P, long long p_layer_stride,
                             long long p_rel_stride, const float* W, const float* Ssm, long long w_layer_stride,
                             const float* X, long long x_layer_stride, const float* K1, const float* K2,
                             const float* K3, const float* S2, const float* S3, const float* Wa2, const float* Wa3,
                             const float* rel, float* G, float* p);

/* Ragged SDDMM over the rows that matter.  row_ptr (R * (N + 1)), col: the batched forward CSR of iddgcn_spmm_csr_f32.
 * Query q's candidates are the stored entries of row h[q] of relation 0, 1, .., R-1, then (if t[q] != h[q]) those of
 * row t[q] of relation 0, .., R-1, each row in CSR order; candidate j is written at qptr[q] + j:
 *   entry[..] = entry_of_csr[pos] (int64 array over the CSR positions; null: pos itself), int32;
 *   grad[..]  = <G[q][side][rel], E[col[pos]]>  (side 0 for row h, 1 for row t; G[q][0] + G[q][1] when h == t).
 * qptr (Q + 1) int64, ascending: qptr[q + 1] - qptr[q] is the query's candidate count (the sum of its row degrees);
 * a shorter segment is filled as far as it goes, never beyond.  E (N, d) and G are read as 16-byte vectors
 * (IDDGCN_E_BAD_ARG when misaligned).  d in {32, 64}, 1 <= R <= 8. */
int iddgcn_explain_row_grads_f32(void* stream, int Q, int N, int d, int R, const int* h, const int* t,
                                 const int* row_ptr, const int* col, const long long* entry_of_csr, const float* G,
                                 const float* E, const long long* qptr, int* entry, float* grad);

/* Per query, the k best of its candidate segment [qptr[q], qptr[q + 1]) of (entry, grad), 1 <= k <= IDDGCN_TOPK_MAX
 * (iddgcn_screen.h): descending by value (IEEE comparison, -0.0 == +0.0), ties by ascending entry id; the entry ids
 * of a segment are distinct.  topk_entry (Q, k) int32, topk_val (Q, k), padded with -1 / -inf;  n_pos[q] = the
 * number of candidates with value > 0.  One workgroup per query, no atomics. */
int iddgcn_explain_topk_f32(void* stream, int Q, int k, const long long* qptr, const int* entry, const float* grad,
                            int* topk_entry, float* topk_val, int* n_pos);

#ifdef __cplusplus
}
#endif

#endif /* IDDGCN_EXPLAIN_H_ */
