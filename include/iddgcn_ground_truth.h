/*
 * iddgcn_ground_truth.h — explanation ground truth of libiddgcn_hip.so (explanation/ground_truth.py:6-76).
 *
 * For a response triple (mu0, rel0, drug0) the reference collects, from the response table dc and the two
 * similarity tables, the triples that "explain" it.  With
 *   SM = [mu2 of the mu_sim rows with mu1 == mu0, table order] ++ [mu1 of the rows with mu2 == mu0, table order]
 *   SD = the same from drug_sim for drug0            (duplicates and self-pairs stay)
 *   c(m, r, d) = number of rows of dc equal to (m, r, d)
 * the output is, in this order,
 *   1. for m in SM:                      (m, rel0, drug0)  c(m, rel0, drug0) times
 *   2. for d in SD:                      (mu0, rel0, d)    c(mu0, rel0, d) times
 *   3. for d in SD, for m in SM (inner): (m, rel0, d)      c(m, rel0, d) times
 *   4. for d in SD: (drug0, drug_rel, d) once per distinct d, if c(m, rel0, d) > 0 for some m in {mu0} u SM
 *   5. for m in SM: (mu0, mu_rel, m)     once per distinct m, if c(m, rel0, d) > 0 for some d in {drug0} u SD
 * Steps 4 and 5 are the reference's `added_combinations` set when no id is both a mutation and a drug (the caller
 * checks that; iddgcn_amd/ground_truth.py).
 *
 * Device layout.  The similarity lists are a CSR over nodes (iddgcn_gt_sim_lists): a stable radix sort of
 * [forward rows ; reversed rows] by node keeps the table order inside each list, and a second stable sort by
 * (node, value) marks each value's first occurrence in its list.  dc is a CSR over (rel, drug) of the sorted
 * mutations, multiplicities kept (iddgcn_gt_dc_table), so c(m, r, d) is upper_bound - lower_bound in one short
 * segment.  iddgcn_ground_truth_count / _fill run one workgroup per query over the probe grid of steps 1-3 in
 * chunks of the block size and place the hits in order (wave ballot + popcount, a cross-wave prefix in LDS, a
 * running base); the same walk sets per-d / per-m hit flags in LDS, which steps 4 and 5 compact with the
 * first-occurrence flags.  Integer work only, no atomics: the output is a pure function of the input.
 *
 * Conventions as in iddgcn_graph.h: device pointers, caller-owned outputs and workspace, `stream` = hipStream_t
 * as void*, return 0 / a positive hipError_t / a negative IDDGCN_E_*.  Nothing here synchronises: error flags are
 * written to device memory for the caller to read BEFORE it passes the tables on (the query kernels index with
 * the tables' values and rely on them being in range).
 */
#ifndef IDDGCN_GROUND_TRUTH_H_
#define IDDGCN_GROUND_TRUTH_H_

#ifdef __cplusplus
extern "C" {
#endif

/* Longest similarity list (|SM| or |SD|) of a query the query kernels handle: the per-entry hit flags live in
 * LDS.  A query beyond it sets the error flag and emits nothing. */
#define IDDGCN_GT_LIST_CAPACITY 8192

/* *bytes = workspace of iddgcn_gt_sim_lists for a table of n rows; IDDGCN_E_BAD_ARG if 2n >= 2^31. */
int iddgcn_gt_sim_lists_workspace(long long n, long long* bytes);

/* Similarity lists of every node.  sim: (n, 3) int64 rows (a, _, b).  ptr [N+1]; val [2n]: node v's list
 * val[ptr[v] .. ptr[v+1]) = the b of its rows (a == v) in table order, then the a of its rows (b == v) in table
 * order; first [2n]: 1 where val[k] does not occur earlier in the same list.  err [1]: 1 if an id of the table is
 * outside [0, N) (such an id is clamped: the arrays stay in range, their content is then meaningless). */
int iddgcn_gt_sim_lists(void* stream, long long n, int N, const long long* sim, int* ptr, int* val,
                        unsigned char* first, int* err, void* workspace, long long workspace_bytes);

/* *bytes = workspace of iddgcn_gt_dc_table; IDDGCN_E_BAD_ARG if M >= 2^31, R*N >= 2^31 or R*N*N >= 2^63. */
int iddgcn_gt_dc_table_workspace(long long M, int N, int R, long long* bytes);

/* Response lookup table.  dc: (M, 3) int64 rows (mu, rel, drug).  seg_ptr [R*N+1], seg_mu [M]: the mutations of
 * the rows with (rel, drug) = (r, d), ascending and with repeats, are seg_mu[seg_ptr[r*N+d] .. seg_ptr[r*N+d+1]).
 * Keys are 64-bit ((r*N + d)*N + mu).  err [1]: 1 if a mu / drug is outside [0, N) or a rel outside [0, R). */
int iddgcn_gt_dc_table(void* stream, long long M, int N, int R, const long long* dc, int* seg_ptr, int* seg_mu,
                       int* err, void* workspace, long long workspace_bytes);

/* COUNT: len[q] = number of ground-truth triples of query q.  queries: (Q, 3) int64 (mu0, rel0, drug0) with
 * 0 <= mu0, drug0 < N and 0 <= rel0 < R (the caller checks).  err [1] is set to 1 (and len[q] to 0) if a list of
 * query q is longer than IDDGCN_GT_LIST_CAPACITY; the caller zeroes err before. */
int iddgcn_ground_truth_count(void* stream, int Q, int N, int R, const long long* queries,
                              const int* mu_ptr, const int* mu_val, const unsigned char* mu_first,
                              const int* drug_ptr, const int* drug_val, const unsigned char* drug_first,
                              const int* seg_ptr, const int* seg_mu, long long* len, int* err);

/* ptr[0] = 0, ptr[q+1] = len[0] + ... + len[q] (one workgroup). */
int iddgcn_gt_exclusive_scan(void* stream, int Q, const long long* len, long long* ptr);

/* FILL: the triples of query q, in the order above, at triples[3*ptr[q] ..) (int64 (total, 3)). */
int iddgcn_ground_truth_fill(void* stream, int Q, int N, int R, const long long* queries,
                             const int* mu_ptr, const int* mu_val, const unsigned char* mu_first,
                             const int* drug_ptr, const int* drug_val, const unsigned char* drug_first,
                             const int* seg_ptr, const int* seg_mu, const long long* ptr, int drug_rel, int mu_rel,
                             long long* triples);

#ifdef __cplusplus
}
#endif

#endif /* IDDGCN_GROUND_TRUTH_H_ */
