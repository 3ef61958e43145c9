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

/*
 * Batched mask explainers (GNNExplainer / the IDDGCN explainer): every epoch of one triple's mask training in one
 * workgroup.  The computation graph of (h, r, t) is every stored entry whose row or column is h or t; its rows h and
 * t are the full graph's rows h and t, and the prediction reads A_r only through AE_r[h] and AE_r[t].  A query's
 * candidates j = 0 .. n-1 (ascending entry id of the full adjacency, all of base value 1) carry rel_j, col_j and
 * role_j (bit 0: the entry's row is h, bit 1: it is t, 0: only its column is h or t).  Per query, with
 * step0 = epochs_base + q * num_epochs (q = the query's place in the INPUT order: the shared optimizer's count):
 *
 *     load:   e = entry_j;  gap = step0 - steps[e];  m[e] *= b1^gap;  v[e] *= b2^gap;  mask_j = init_e[e]
 *     before = forward(mv = 1)
 *     for ep = 0 .. num_epochs-1:
 *         mv_j = sigmoid(mask_j);   AE_r[h] = sum_{role_j & 1, rel_j = r} mv_j E[col_j]  (j ascending), AE_r[t] alike
 *         forward:  xh^0 = E[h], xt^0 = E[t];  for l = 1, 2, 3:
 *             a_l = softmax(xh^{l-1} Walpha^l + balpha^l),  w_l = sigmoid(a_l),  P^l_r[.] = AE_r[.] K^l_r
 *             xh^l = sigmoid(xh^{l-1} S^l + sum_r w_lr P^l_r[h]),  xt^l = sigmoid(xt^{l-1} S^l + sum_r w_lr P^l_r[t])
 *             p = sigmoid(sum_d xh^3 rel[r] xt^3)
 *         backward: the one above with scale = 1, P^l_r[h], P^l_r[t] the local ones and the layer-1 S = S^1 unused
 *         g_j = (<GH_rel_j, E[col_j]> [role_j & 1] + <GT_rel_j, E[col_j]> [role_j & 2]) * (-before / (p + 1e-5))
 *         with target_ratios (R values):  c_r = sum_{rel_j = r} mv_j,  C = sum_r c_r,  ratio_r = c_r / C,
 *             dr_r = 2 (ratio_r - target_r) / R,  gs_r = (dr_r - sum_i dr_i ratio_i) / C,  g_j = (g_j + gs_rel_j) / 2
 *         g_j = g_j mv_j (1 - mv_j)
 *         Adam, dense form, on e = entry_j:  m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2)
 *             mask_j -= m alpha[step0 + ep] / (sqrt(v) + eps)
 *     finish: out[qptr[q] + j] = sigmoid(mask_j);  steps[e] = step0 + num_epochs
 *
 * m, v, steps hold one value per stored entry of the full adjacency: the moments of the reference's one shared
 * optimizer, decayed lazily over the steps an entry sat out.  One launch runs the queries qids[0 .. n_queries); two
 * queries of one launch must share no entry (explain.mask_schedule), queries that share one run in input order in
 * successive launches of one stream.  No atomics, no flags; every sum has a fixed order that depends on the query's
 * own candidates only.
 */
typedef struct {
    int N, d, R;
    int num_epochs, epochs_base;
    int n_queries;
    const int* qids;                 /* (n_queries) query ids of this launch */
    const int* h; const int* r; const int* t;                 /* per query, int32, validated by the caller */
    const long long* qptr;           /* (Q + 1) candidate segments */
    const int* entry; const int* crel; const int* ccol; const int* crole;   /* per candidate */
    const float* E;                  /* (N, d), 16-byte aligned */
    const float* K[3];               /* (R, d, d) */
    const float* KT[3];              /* (R, d, d): every K^l_r transposed (the backward reads it along rows) */
    const float* S[3];               /* (d, d) */
    const float* ST[3];              /* (d, d): S^l transposed (ST[0] is never read) */
    const float* Wa[3];              /* (d, R) */
    const float* ba[3];              /* (R) */
    const float* rel;                /* (R, d) */
    const float* init_e;             /* (total_nnz) init_value[row, col] of every stored entry */
    float* m; float* v; int* steps;  /* (total_nnz) each */
    const float* alpha;              /* one per global step */
    float b1, b2, eps;
    const float* target_ratios;      /* (R) or null */
    float* out;                      /* (qptr[Q]) final masked values; the masks live here while a query trains */
} iddgcn_mask_explain_t;

/* d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL), n_queries >= 0 (0: nothing launched),
 * num_epochs >= 0; a null pointer (target_ratios excepted) or a misaligned E: IDDGCN_E_BAD_ARG. */
int iddgcn_mask_explain_f32(void* stream, const iddgcn_mask_explain_t* args);

/*
 * Deletion and insertion curves of Q explanations (explain.fidelity_curves): 2 (k + 1) edited forwards per query
 * against one pass over the weights per tile of variants.  A query's candidates j = 0 .. n-1 are the stored,
 * non-placeholder entries of the full adjacency whose ROW is h or t (role_j != 0, bits as above), ascending entry id
 * (so relation-major), each with its stored value val_j and a step_j: the position of the first explanation edge that
 * names it, -1 when none does.  With F_i = {j : 0 <= step_j < i}, for i = 0 .. k:
 *
 *     del[q][i] = forward(keep_j = [j not in F_i]),   ins[q][i] = forward(keep_j = [j in F_i])
 *     forward:  AE_r[h] = sum_{role_j & 1, rel_j = r} keep_j val_j E[col_j]  (one fmaf chain per column, j ascending;
 *               a dropped candidate enters with the multiplier 0), AE_r[t] alike with role_j & 2;
 *               then the mask explainer's forward above: softmax from the head row, w = sigmoid(softmax), DistMult.
 *
 * del[q][0] is the unedited prediction, ins[q][0] the prediction with both rows empty.  One workgroup per (query,
 * tile of 8 variants); no atomics, no flags.  Every point has a fixed summation order that depends on the query's own
 * candidates and on the SET F_i only: not on Q, k, the query's place in the batch, the other variants or the order of
 * the steps inside F_i.
 */
typedef struct {
    int N, d, R;
    int k;                           /* explanation length: k + 1 points per curve, 1 <= k <= IDDGCN_TOPK_MAX */
    int Q;
    const int* h; const int* r; const int* t;                 /* per query, int32, validated by the caller */
    const long long* qptr;           /* (Q + 1) candidate segments */
    const int* crel; const int* ccol; const int* crole; const int* cstep;   /* per candidate; crel ascends in a segment */
    const float* cval;               /* per candidate */
    const float* E;                  /* (N, d), 16-byte aligned */
    const float* K[3];               /* (R, d, d) */
    const float* S[3];               /* (d, d) */
    const float* Wa[3];              /* (d, R) */
    const float* ba[3];              /* (R) */
    const float* rel;                /* (R, d) */
    float* del; float* ins;          /* (Q, k + 1) each */
} iddgcn_explain_curves_t;

/* d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL), 1 <= k <= IDDGCN_TOPK_MAX, Q >= 0 (0: nothing
 * launched), N >= 1; a null pointer (the candidate arrays excepted: they are never read when every segment is empty)
 * or a misaligned E: IDDGCN_E_BAD_ARG. */
int iddgcn_explain_curves_f32(void* stream, const iddgcn_explain_curves_t* args);

/*
 * Counterfactual edge sets by greedy deletion, and the occlusion table (explain.counterfactual_batched,
 * explain.occlusion_batched).  Candidates and the forward are those of iddgcn_explain_curves_f32: for a set F of
 * removed candidates, p(F) is its deletion forward with keep_j = [j not in F], same arithmetic and summation order, so
 * p(F) is bitwise the last deletion point of an explanation that names exactly F.  Each candidate also carries
 * partner_j (the segment-relative index of a candidate removed together with it, symmetric; -1: none) and elig_j
 * (0: the candidate stays in the graph and is never evaluated).  Per query, with dir = +1 (lower p) or -1 (raise it):
 *
 *     mode FLIP: dir = +1 when p(0) > threshold, else -1;  LOWER: +1;  RAISE: -1
 *     flipped(p) = !(p > threshold) when dir = +1,  p > threshold when dir = -1          (fp32 comparisons)
 *     F = {};  path[0] = p(F);  loo[j] = p({j, partner_j}) for every eligible j, NaN for the others
 *     for i = 0 .. K-1, while !flipped(path[i]) and an eligible candidate is left outside F:
 *         p_j = p(F + {j, partner_j}) for every eligible j not in F
 *         j* = the j of the smallest dir p_j; equal bit patterns: the lowest j
 *         chosen[i] = j*;  cstep[j*] = cstep[partner_j*] = i;  F += {j*, partner_j*};  path[i + 1] = p_j*
 *     n_steps = the steps taken;  flipped = flipped(path[n_steps]);  path past n_steps repeats path[n_steps],
 *     chosen past it is -1, cstep of a candidate never removed is -1.
 *
 * The best candidate is taken even when it does not improve p.  2 max(K, 1) launches, none read by the host: a step
 * kernel (one workgroup per (query, tile of 8 variants); variant 0 is F itself, variant 1 + j removes candidate j;
 * a query that has stopped and a tile without an eligible remaining candidate exit at once) writes one fp32 per
 * evaluated candidate (step 0: into loo; later steps: into scratch), a select kernel (one workgroup per query) takes
 * the arg-min by an ordered 64-bit key and updates the outputs.  No atomics; every result of a query depends on its
 * own candidates only: not on Q, on its place in the batch, on the other queries, on max_cand or on K (a shorter
 * search is the prefix of a longer one).
 */
#define IDDGCN_CF_FLIP 0
#define IDDGCN_CF_LOWER 1
#define IDDGCN_CF_RAISE 2

typedef struct {
    int N, d, R;
    int k;                           /* K: steps at most, 0 <= k <= IDDGCN_TOPK_MAX (0: only loo and path[0]) */
    int Q;
    int mode;                        /* IDDGCN_CF_* */
    float threshold;
    int max_cand;                    /* sizes the step kernel's grid: ceil((max_cand + 1) / 8) workgroups per query,
                                        which stride over the tiles of a longer segment.  >= 0; a hint, not a bound */
    const int* h; const int* r; const int* t;                 /* per query, int32, validated by the caller */
    const long long* qptr;           /* (Q + 1) candidate segments */
    const int* crel; const int* ccol; const int* crole;       /* per candidate; crel ascends in a segment */
    const int* cpartner; const int* celig;                    /* per candidate */
    const float* cval;               /* per candidate */
    const float* E;                  /* (N, d), 16-byte aligned */
    const float* K[3];               /* (R, d, d) */
    const float* S[3];               /* (d, d) */
    const float* Wa[3];              /* (d, R) */
    const float* ba[3];              /* (R) */
    const float* rel;                /* (R, d) */
    float* path;                     /* (Q, K + 1) */
    int* chosen;                     /* (Q, K); may be null when K == 0 */
    int* cstep;                      /* per candidate; written, never read before it is written */
    int* n_steps; int* flipped;      /* (Q) each */
    float* loo;                      /* per candidate */
    float* scratch;                  /* per candidate: the values of the steps after step 0; may be null when K <= 1 */
} iddgcn_counterfactual_t;

/* d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL), 0 <= k <= IDDGCN_TOPK_MAX, a mode above, Q >= 0
 * (0: nothing launched), N >= 1, max_cand >= 0; a null pointer (the candidate arrays, cstep, loo and scratch excepted:
 * they are never touched when every segment is empty) or a misaligned E: IDDGCN_E_BAD_ARG.  Allocates nothing and
 * never synchronises. */
int iddgcn_explain_counterfactual_f32(void* stream, const iddgcn_counterfactual_t* args);

/*
 * Integrated gradients over the adjacency values (explain.integrated_gradients_batched): signed per-edge attributions
 * that add up to the change of the prediction between a baseline graph and the actual one.  Candidates, roles and the
 * eligibility flag are those of iddgcn_explain_counterfactual_f32.  Along the path an eligible candidate enters with
 * the value a_j(alpha) = val_j alpha, every other one with val_j (it stays in the graph and gets no attribution):
 *
 *     f(alpha)  = the mask explainer's forward with AE_r[h] = sum_{role_j & 1, rel_j = r} a_j(alpha) E[col_j], AE_r[t] alike
 *     g_j(alpha) = d f / d a_j = <GH_rel_j, E[col_j]> [role_j & 1] + <GT_rel_j, E[col_j]> [role_j & 2]   (backward, scale 1)
 *     attr_j = val_j sum_{i < m} omega_i g_j(alpha_i)      for the quadrature rule (alpha_i, omega_i); exactly 0 when
 *                                                          the candidate is not eligible
 *     p_full = f(1),  p_base = f(0),  total = sum_j attr_j,  gap = total - (p_full - p_base)
 *
 * For an exact integral gap is 0 (completeness); |gap| is the quadrature's error plus rounding.  AE(alpha) is linear
 * in alpha and the backward's K^T products are linear in dz, so a node costs four d x d mat-vecs forward and four
 * backward: a path kernel (one workgroup per (query, chunk of 32 nodes)) writes 6 R d partial sums per chunk to
 * `scratch`, a finish kernel (one workgroup per query) adds the chunks in chunk order, applies K^T and writes the
 * outputs.  Two launches; no atomics, no flags, no allocation, no synchronisation.  Every result of a query has a
 * fixed summation order that depends on the query's own candidates and on the rule (m, alpha, omega) only: not on Q,
 * the query's place in the batch or the other queries.
 */
#define IDDGCN_PATH_MAX_STEPS 1024

typedef struct {
    int N, d, R;
    int Q;
    int m;                           /* quadrature nodes, 1 <= m <= IDDGCN_PATH_MAX_STEPS */
    const int* h; const int* r; const int* t;                 /* per query, int32, validated by the caller */
    const long long* qptr;           /* (Q + 1) candidate segments */
    const int* crel; const int* ccol; const int* crole;       /* per candidate; crel ascends in a segment */
    const int* celig;                /* per candidate */
    const float* cval;               /* per candidate */
    const float* E;                  /* (N, d), 16-byte aligned */
    const float* K[3];               /* (R, d, d) */
    const float* KT[3];              /* (R, d, d): every K^l_r transposed */
    const float* S[3];               /* (d, d) */
    const float* ST[3];              /* (d, d): S^l transposed (ST[0] is never read) */
    const float* Wa[3];              /* (d, R) */
    const float* ba[3];              /* (R) */
    const float* rel;                /* (R, d) */
    const float* alpha; const float* omega;                   /* (m) each: the rule's nodes and weights */
    float* attr;                     /* per candidate */
    float* total; float* p_full; float* p_base; float* gap;   /* (Q) each */
    float* scratch;                  /* iddgcn_explain_path_scratch_floats(Q, m, d, R) floats */
} iddgcn_explain_path_t;

/* The floats `scratch` must hold: Q * ceil(m / 32) * 6 * R * d (0 for arguments the entry below refuses). */
long long iddgcn_explain_path_scratch_floats(int Q, int m, int d, int R);

/* d in {32, 64} (IDDGCN_E_BAD_DIM), 1 <= R <= 8 (IDDGCN_E_BAD_REL), 1 <= m <= IDDGCN_PATH_MAX_STEPS, Q >= 0 (0: nothing
 * launched), N >= 1; a null pointer (the candidate arrays and attr excepted: they are never touched when every segment
 * is empty) or a misaligned E: IDDGCN_E_BAD_ARG. */
int iddgcn_explain_path_f32(void* stream, const iddgcn_explain_path_t* args);

#ifdef __cplusplus
}
#endif

#endif /* IDDGCN_EXPLAIN_H_ */
