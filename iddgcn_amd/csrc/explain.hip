// explain.hip — batched explaiNE and the batched mask explainers for gfx950 (include/iddgcn_explain.h).
//
// The prediction of (h, r, t) reads A_r only through AE_r[h] and AE_r[t], so its gradient w.r.t. the adjacency values
// lives in rows h and t alone.  Three kernels, none of them proportional to N or nnz:
//
// seeds_kernel: QT = 8 queries per workgroup.  The tail chain x^1..x^3 is recomputed from the node tables as in
// screen_chain_kernel, then the backward of iddgcn_explain.h runs on 16 row vectors (head and tail of every query)
// at once.  One d x d matrix (S^l or K^l_r) at a time is staged in LDS with rows padded to d + 1 floats, so that
// both x·M (lanes along a row) and x·M^T (lanes down a column) read it without bank conflicts; every matrix element
// read serves VPG vectors.  GH / GT accumulate in registers over the layers and are written once.  Exact fp32:
// fmaf chains, four per dot product, (c0 + c1) + (c2 + c3).
//
// row_grads_kernel: one workgroup per query; GH, GT in LDS, one candidate (a stored entry of row h or t) per thread,
// its dot product against E[col] in one thread (no cross-lane reduction, no atomics).
//
// topk_kernel: one workgroup per query over its candidate segment: rank_topk_kernel's passes (screen.hip), a bitonic
// sort of 64-bit (value, entry id) keys in LDS merged into the running top 64.
//
// mask_explain_kernel (further down): every epoch of one triple's mask training in one workgroup.
//
// curves_kernel: the deletion and insertion curves of an explanation, a tile of edited forwards per workgroup.
//
// cf_step_kernel / cf_select_kernel: the greedy counterfactual search, one pair of launches per step.
//
// ig_path_kernel / ig_finish_kernel (last): integrated gradients over the adjacency values, a chunk of quadrature
// nodes per workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "iddgcn.h"
#include "iddgcn_explain.h"
#include "iddgcn_screen.h"
#include "per_query.hpp"

namespace xpl {

using namespace pq;      // f32x4, sigmoid_fast, make_key, TK_BUF / TK_CH

constexpr int MAX_R = 8;
constexpr int NT = 256;            // 4 waves
constexpr int QT = 8;              // queries per workgroup of seeds_kernel
constexpr int NV = 2 * QT;         // row vectors: 2 qi = head of query qi, 2 qi + 1 = its tail

struct SeedP {
    int Q, N, R;
    const int* h; const int* r; const int* t;
    float scale;
    const float* ES1; const float* P; long long pls, prs;
    const float* W; const float* Ssm; long long wls;
    const float* X; long long xls;
    const float* K[3]; const float* S[2]; const float* Wa[2]; const float* rel;
    float* G; float* p;
};

// M (D rows of LD floats) <- a (D, D) row-major matrix
template <int D>
__device__ __forceinline__ void stage_matrix(float* M, const float* __restrict__ src) {
#pragma unroll
    for (int it = 0; it < D * D / NT; ++it) {
        const int idx = it * NT + threadIdx.x;
        M[(idx / D) * (D + 1) + idx % D] = src[idx];
    }
}

template <int D>
__global__ __launch_bounds__(NT) void seeds_kernel(const SeedP a) {
    constexpr int LD = D + 1;
    constexpr int GR = NT / D;         // thread groups of D lanes
    constexpr int VPG = NV / GR;       // row vectors per group: 4 at D = 64, 2 at D = 32
    __shared__ float M[D * LD];
    __shared__ float act[3][NV][D];    // x^1..x^3 of every row vector
    __shared__ float dx[NV][D];
    __shared__ float dz[NV][D];
    __shared__ float w[3][QT][MAX_R];
    __shared__ float sm[3][QT][MAX_R];
    __shared__ float dwv[NV][MAX_R];
    __shared__ float da[QT][MAX_R];
    __shared__ float du[QT][MAX_R];
    __shared__ int node[NV];
    __shared__ int qrel[QT];
    const int tid = threadIdx.x;
    const int R = a.R;
    const int q0 = blockIdx.x * QT;
    const int k = tid % D, grp = tid / D;

    // queries past Q repeat the last one (computed, never stored)
    if (tid < QT) {
        const int q = q0 + tid < a.Q ? q0 + tid : a.Q - 1;
        node[2 * tid] = a.h[q];
        node[2 * tid + 1] = a.t[q];
        qrel[tid] = a.r[q];
    }
    __syncthreads();
    for (int idx = tid; idx < 3 * QT * R; idx += NT) {
        const int l = idx / (QT * R), qi = (idx / R) % QT, r = idx % R;
        const size_t o = (size_t)l * a.wls + (size_t)node[2 * qi] * R + r;
        w[l][qi][r] = a.W[o];
        sm[l][qi][r] = a.Ssm[o];
    }
    for (int idx = tid; idx < 3 * QT * D; idx += NT) {
        const int l = idx / (QT * D), qi = (idx / D) % QT, c = idx % D;
        act[l][2 * qi][c] = a.X[(size_t)l * a.xls + (size_t)node[2 * qi] * D + c];
    }
    __syncthreads();

    // tail chain, layer 1: x^1 = sigmoid(ES1[t] + sum_r w_1r P^1_r[t]), r ascending
    for (int idx = tid; idx < QT * D; idx += NT) {
        const int qi = idx / D, c = idx % D;
        const size_t row = (size_t)node[2 * qi + 1] * D + c;
        float v = a.ES1[row];
#pragma unroll
        for (int r = 0; r < MAX_R; ++r)
            if (r < R) v = fmaf(w[0][qi][r], a.P[r * a.prs + row], v);
        act[0][2 * qi + 1][c] = sigmoid_fast(v);
    }
    // layers 2, 3: x^l = sigmoid(x^{l-1} S^l + sum_r w_lr P^l_r[t])
    for (int l = 1; l < 3; ++l) {
        stage_matrix<D>(M, a.S[l - 1]);
        __syncthreads();
        for (int idx = tid; idx < QT * D; idx += NT) {
            const int qi = idx / D, c = idx % D;
            const float* x = act[l - 1][2 * qi + 1];
            float c4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < D; ++i) c4[(i >> 3) & 3] = fmaf(x[i], M[i * LD + c], c4[(i >> 3) & 3]);
            float v = (c4[0] + c4[1]) + (c4[2] + c4[3]);
            const size_t row = (size_t)node[2 * qi + 1] * D + c;
            const float* Pl = a.P + l * a.pls;
#pragma unroll
            for (int r = 0; r < MAX_R; ++r)
                if (r < R) v = fmaf(w[l][qi][r], Pl[r * a.prs + row], v);
            act[l][2 * qi + 1][c] = sigmoid_fast(v);
        }
        __syncthreads();
    }

    // DistMult, the prediction and its seed: one thread per query, d ascending
    if (tid < QT) {
        const float* rl = a.rel + (size_t)qrel[tid] * D;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(act[2][2 * tid][d] * rl[d], act[2][2 * tid + 1][d], s);
        const float p = 1.0f / (1.0f + expf(-s));
        da[tid][0] = a.scale * (p * (1.0f - p));
        if (q0 + tid < a.Q) a.p[q0 + tid] = p;
    }
    __syncthreads();
    for (int idx = tid; idx < QT * D; idx += NT) {
        const int qi = idx / D, c = idx % D;
        const float gr = da[qi][0] * a.rel[(size_t)qrel[qi] * D + c];
        dx[2 * qi][c] = gr * act[2][2 * qi + 1][c];
        dx[2 * qi + 1][c] = gr * act[2][2 * qi][c];
    }
    __syncthreads();

    float Gacc[VPG][MAX_R];
#pragma unroll
    for (int j = 0; j < VPG; ++j)
#pragma unroll
        for (int r = 0; r < MAX_R; ++r) Gacc[j][r] = 0.f;

    for (int l = 2; l >= 0; --l) {
        for (int idx = tid; idx < NV * D; idx += NT) {
            const int v = idx / D, c = idx % D;
            const float x = act[l][v][c];
            dz[v][c] = dx[v][c] * (x * (1.0f - x));
        }
        __syncthreads();
        // G_r += w_lr (dz K^l_r^T): lane k owns output column k of its group's VPG vectors
#pragma unroll
        for (int r = 0; r < MAX_R; ++r)
            if (r < R) {
                stage_matrix<D>(M, a.K[l] + (size_t)r * D * D);
                __syncthreads();
                float c4[VPG][4];
#pragma unroll
                for (int j = 0; j < VPG; ++j) c4[j][0] = c4[j][1] = c4[j][2] = c4[j][3] = 0.f;
#pragma unroll 1
                for (int i0 = 0; i0 < D; i0 += 32)
#pragma unroll
                    for (int ii = 0; ii < 32; ++ii) {
                        const int i = i0 + ii;
                        const float m = M[k * LD + i];
#pragma unroll
                        for (int j = 0; j < VPG; ++j)
                            c4[j][(ii >> 3) & 3] = fmaf(dz[grp * VPG + j][i], m, c4[j][(ii >> 3) & 3]);
                    }
#pragma unroll
                for (int j = 0; j < VPG; ++j) {
                    const float acc = (c4[j][0] + c4[j][1]) + (c4[j][2] + c4[j][3]);
                    Gacc[j][r] = fmaf(w[l][(grp * VPG + j) >> 1][r], acc, Gacc[j][r]);
                }
                __syncthreads();
            }
        if (l == 0) break;

        // dw_r = <dzh, P^l_r[h]> + <dzt, P^l_r[t]>: per vector a butterfly over the D lanes of its group
#pragma unroll
        for (int j = 0; j < VPG; ++j) {
            const int v = grp * VPG + j;
            const float* Pl = a.P + l * a.pls + (size_t)node[v] * D + k;
            const float z = dz[v][k];
#pragma unroll
            for (int r = 0; r < MAX_R; ++r)
                if (r < R) {
                    float part = z * Pl[r * a.prs];
#pragma unroll
                    for (int o = D / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
                    if (k == 0) dwv[v][r] = part;
                }
        }
        __syncthreads();
        if (tid < QT * R) {
            const int qi = tid / R, r = tid % R;
            const float wv = w[l][qi][r];
            da[qi][r] = (dwv[2 * qi][r] + dwv[2 * qi + 1][r]) * (wv * (1.0f - wv));
        }
        __syncthreads();
        if (tid < QT * R) {
            const int qi = tid / R, r = tid % R;
            float sum = 0.f;
            for (int i = 0; i < R; ++i) sum = fmaf(sm[l][qi][i], da[qi][i], sum);
            du[qi][r] = sm[l][qi][r] * (da[qi][r] - sum);
        }
        // dx^{l-1} = dz S^l^T (+ du Walpha^l^T on the head side)
        stage_matrix<D>(M, a.S[l - 1]);
        __syncthreads();
        {
            float c4[VPG][4];
#pragma unroll
            for (int j = 0; j < VPG; ++j) c4[j][0] = c4[j][1] = c4[j][2] = c4[j][3] = 0.f;
#pragma unroll 1
            for (int i0 = 0; i0 < D; i0 += 32)
#pragma unroll
                for (int ii = 0; ii < 32; ++ii) {
                    const int i = i0 + ii;
                    const float m = M[k * LD + i];
#pragma unroll
                    for (int j = 0; j < VPG; ++j)
                        c4[j][(ii >> 3) & 3] = fmaf(dz[grp * VPG + j][i], m, c4[j][(ii >> 3) & 3]);
                }
            const float* wa = a.Wa[l - 1] + (size_t)k * R;
#pragma unroll
            for (int j = 0; j < VPG; ++j) {
                const int v = grp * VPG + j;
                float acc = (c4[j][0] + c4[j][1]) + (c4[j][2] + c4[j][3]);
                if ((v & 1) == 0) {
#pragma unroll
                    for (int r = 0; r < MAX_R; ++r)
                        if (r < R) acc = fmaf(du[v >> 1][r], wa[r], acc);
                }
                dx[v][k] = acc;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < VPG; ++j) {
        const int v = grp * VPG + j;
        const int q = q0 + (v >> 1);
        if (q < a.Q) {
            float* g = a.G + ((size_t)q * 2 + (v & 1)) * R * D + k;
#pragma unroll
            for (int r = 0; r < MAX_R; ++r)
                if (r < R) g[(size_t)r * D] = Gacc[j][r];
        }
    }
}

// ---- ragged SDDMM ----------------------------------------------------------------------------------------------
struct RowP {
    int N, R;
    const int* h; const int* t; const int* row_ptr; const int* col; const long long* eoc;
    const float* G; const float* E; const long long* qptr;
    int* entry; float* grad;
};

template <int D>
__global__ __launch_bounds__(NT) void row_grads_kernel(const RowP a) {
    __shared__ __attribute__((aligned(16))) float Gs[2 * MAX_R * D];
    __shared__ int seg_beg[2 * MAX_R];
    __shared__ int seg_off[2 * MAX_R + 1];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, R = a.R;
    const int hh = a.h[q], tt = a.t[q];
    const bool same = hh == tt;
    const int ns = same ? R : 2 * R;
    const float* g = a.G + (size_t)q * 2 * R * D;
    for (int idx = tid; idx < R * D; idx += NT) {
        const float g0 = g[idx], g1 = g[R * D + idx];
        Gs[idx] = same ? g0 + g1 : g0;
        Gs[R * D + idx] = g1;
    }
    if (tid == 0) {
        int off = 0;
        for (int s = 0; s < ns; ++s) {
            const size_t row = (size_t)(s % R) * (a.N + 1) + (s < R ? hh : tt);
            const int b = a.row_ptr[row], e = a.row_ptr[row + 1];
            seg_beg[s] = b;
            seg_off[s] = off;
            off += e > b ? e - b : 0;
        }
        seg_off[ns] = off;
    }
    __syncthreads();
    const long long base = a.qptr[q];
    const long long room = a.qptr[q + 1] - base;
    const int total = (long long)seg_off[ns] < room ? seg_off[ns] : (int)(room > 0 ? room : 0);
    for (int j = tid; j < total; j += NT) {
        int s = 0;
        while (j >= seg_off[s + 1]) ++s;
        const int pos = seg_beg[s] + (j - seg_off[s]);
        const f32x4* e4 = (const f32x4*)(a.E + (size_t)a.col[pos] * D);
        const f32x4* g4 = (const f32x4*)(Gs + s * D);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < D / 4; ++i) {
            const f32x4 ev = e4[i], gv = g4[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(gv[c], ev[c], acc[c]);
        }
        a.entry[base + j] = a.eoc ? (int)a.eoc[pos] : pos;
        a.grad[base + j] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
}

// ---- selection -------------------------------------------------------------------------------------------------
// the value of a key of make_key (per_query.hpp)
__device__ __forceinline__ float key_value(unsigned long long key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__global__ __launch_bounds__(NT) void topk_kernel(int k, const long long* __restrict__ qptr,
                                                  const int* __restrict__ entry, const float* __restrict__ grad,
                                                  int* __restrict__ topk_entry, float* __restrict__ topk_val,
                                                  int* __restrict__ n_pos) {
    __shared__ unsigned long long buf[TK_BUF];
    __shared__ int sel[IDDGCN_TOPK_MAX];
    __shared__ int cnt[NT / 64];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const long long b0 = qptr[q];
    const long long len = qptr[q + 1] - b0;
    const int* ent = entry + b0;
    const float* val = grad + b0;

    for (int j = tid; j < TK_BUF; j += NT) buf[j] = 0ull;
    __syncthreads();
    unsigned long long thr = 0ull;       // the current k-th key
    int pos = 0;
    for (long long base = 0; base < len; base += TK_CH) {
        unsigned long long keys[TK_BUF / NT];
        int any = 0;
#pragma unroll
        for (int u = 0; u < TK_BUF / NT; ++u) {
            const int j = tid + u * NT;
            unsigned long long key = 0ull;
            if (j < TK_CH && base + j < len) {
                const float v = val[base + j];
                key = make_key(v, ent[base + j]);
                pos += v > 0.0f;
            }
            keys[u] = key;
            any |= key > thr;
        }
        if (__syncthreads_or(any)) {
#pragma unroll
            for (int u = 0; u < TK_BUF / NT; ++u) {
                const int j = tid + u * NT;
                if (j < TK_CH) buf[j] = keys[u];
            }
            __syncthreads();
            // bitonic sort, descending
            for (int k2 = 2; k2 <= TK_BUF; k2 <<= 1)
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < TK_BUF / 2; t += NT) {
                        const int x0 = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                        const int x1 = x0 | j;
                        const unsigned long long x = buf[x0], y = buf[x1];
                        const bool desc = (x0 & k2) == 0;
                        if ((x < y) == desc) {
                            buf[x0] = y;
                            buf[x1] = x;
                        }
                    }
                    __syncthreads();
                }
            const unsigned long long top = tid < IDDGCN_TOPK_MAX ? buf[tid] : 0ull;
            thr = buf[k - 1];
            __syncthreads();
            if (tid < IDDGCN_TOPK_MAX) buf[TK_CH + tid] = top;
        }
    }
    __syncthreads();
    int zero = 0;
    if (tid < k) {
        const unsigned long long key = buf[TK_CH + tid];
        const int c = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
        const float v = key ? key_value(key) : -INFINITY;
        topk_entry[(size_t)q * k + tid] = c;
        topk_val[(size_t)q * k + tid] = v;
        sel[tid] = c;
        zero = c >= 0 && v == 0.0f;
    }
    // the keys carry -0.0 as +0.0: a selected zero gets its stored sign back
    if (__syncthreads_or(zero)) {
        for (long long j = tid; j < len; j += NT) {
            const float v = val[j];
            if (v == 0.0f && (__float_as_uint(v) >> 31)) {
                const int c = ent[j];
                for (int i = 0; i < k; ++i)
                    if (sel[i] == c) topk_val[(size_t)q * k + i] = v;
            }
        }
    }
    // n_pos: an integer sum (any order gives the same result)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos += __shfl_xor(pos, o, 64);
    if ((tid & 63) == 0) cnt[tid >> 6] = pos;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int wv = 0; wv < NT / 64; ++wv) n += cnt[wv];
        n_pos[q] = n;
    }
}

// ---- batched mask explainers -----------------------------------------------------------------------------------
// mask_explain_kernel: one workgroup per query runs the unmasked forward and every epoch of the query's mask training
// (iddgcn_explain.h) on chip.  Per-candidate state (mask in a.out, m, v) stays in global memory, each candidate owned by
// one thread (j = tid mod NT) for the whole kernel; the masked values are staged CH at a time for the AE rows, the E
// rows of the first ES_ROWS candidates once for all epochs (the others are read from global memory every epoch).  Every
// matrix is read from global memory with lanes along a row (coalesced): K and S in the forward, their transposes in the
// backward; the small reductions (softmax logits, DistMult, dw) are butterflies over the D lanes of a group.  Four
// fmaf chains per mat-vec element, (c0 + c1) + (c2 + c3).
constexpr int CH = 512;            // candidates staged per pass (a multiple of NT: a candidate keeps its thread)
constexpr int ES_BYTES = 112 * 1024;   // E rows kept in LDS: 448 candidates at d = 64, 896 at d = 32

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }

// sum over the D lanes of a group (D <= 64 lanes of one wave, all active), a fixed butterfly
template <int D>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = D / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// column k of (vh, vt) · M and of v · M: Mk = M + k, M (D, D) row-major in global memory, vectors in LDS.  The loads go
// out 32 at a time before their fmaf chains (left to itself the scheduler waits for every load in turn).
template <int D>
__device__ __forceinline__ void matvec2(const float* __restrict__ Mk, const float* vh, const float* vt, float& yh,
                                        float& yt) {
    float ch[4] = {0.f, 0.f, 0.f, 0.f}, ct[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i0 = 0; i0 < D; i0 += 32) {
        float kv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) kv[u] = Mk[(size_t)(i0 + u) * D];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            ch[(u >> 3) & 3] = fmaf(vh[i0 + u], kv[u], ch[(u >> 3) & 3]);
            ct[(u >> 3) & 3] = fmaf(vt[i0 + u], kv[u], ct[(u >> 3) & 3]);
        }
    }
    yh = (ch[0] + ch[1]) + (ch[2] + ch[3]);
    yt = (ct[0] + ct[1]) + (ct[2] + ct[3]);
}

template <int D>
__device__ __forceinline__ float matvec1(const float* __restrict__ Mk, const float* v) {
    float c4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i0 = 0; i0 < D; i0 += 32) {
        float kv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) kv[u] = Mk[(size_t)(i0 + u) * D];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 32; ++u) c4[(u >> 3) & 3] = fmaf(v[i0 + u], kv[u], c4[(u >> 3) & 3]);
    }
    return (c4[0] + c4[1]) + (c4[2] + c4[3]);
}

// What the four fused kernels below share, written once.  Each is an inline function of LDS / global pointers the
// caller owns; the rule for these kernels is bitwise results within the same register and LDS budget
// (profiles/r21/), so an output element keeps its expression, its chain split and its candidate order here.

// the relation segments of a query's candidate list (ascending by relation): rstart[r] = the first candidate of a
// relation >= r.  Candidate j's part of the scan; rstart[0 .. MAX_R] starts at n
__device__ __forceinline__ void rstart_mark(int* rstart, const int* crel, int j) {
    const int r1 = crel[j];
    const int r0 = j ? crel[j - 1] : -1;
    for (int r = r0 + 1; r <= r1; ++r) rstart[r] = j;
}

// the whole scan; the caller's next barrier publishes it
__device__ __forceinline__ void rstart_scan(int* rstart, const int* crel, int n) {
    if (threadIdx.x <= MAX_R) rstart[threadIdx.x] = n;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += NT) rstart_mark(rstart, crel, j);
}

// es <- the E rows of the first min(n, ROWS) candidates
template <int D, int ROWS>
__device__ __forceinline__ void stage_es(float* es, const float* __restrict__ E, const int* ccol, int n) {
    const int ns = n < ROWS ? n : ROWS;
    for (int idx = threadIdx.x; idx < ns * D; idx += NT) es[idx] = E[(size_t)ccol[idx / D] * D + idx % D];
}

// element i of the softmax over the logits zs[0 .. R): the max, the sum of expf, expf(z - max) / sum, in that order
__device__ __forceinline__ float rel_softmax(const float* zs, int R, int i) {
    float mx = -INFINITY;
    for (int r = 0; r < R; ++r) mx = fmaxf(mx, zs[r]);
    float sum = 0.f;
    for (int r = 0; r < R; ++r) sum += expf(zs[r] - mx);
    return expf(zs[i] - mx) / sum;
}

// its backward: du_i from the softmax values sm and the gradient da w.r.t. them
__device__ __forceinline__ float rel_softmax_bwd(const float* sm, const float* da, int R, int i) {
    float sum = 0.f;
    for (int r = 0; r < R; ++r) sum = fmaf(sm[r], da[r], sum);
    return sm[i] * (da[i] - sum);
}

// column k of dx^{l-1} = dz S^l^T (+ du Walpha^l^T on the head side): STk = S^l^T + k, wa = row k of Walpha^l
template <int D>
__device__ __forceinline__ float dx_step(const float* STk, const float* dz, bool head, const float* du,
                                         const float* wa, int R) {
    float acc = matvec1<D>(STk, dz);
    if (head)
        for (int r = 0; r < R; ++r) acc = fmaf(du[r], wa[r], acc);
    return acc;
}

template <int D>
__global__ __launch_bounds__(NT) void mask_explain_kernel(const iddgcn_mask_explain_t a) {
    constexpr int GR = NT / D;                 // groups of D lanes: 4 / 8
    constexpr int RPG = MAX_R / GR;            // relations per group in the AE and mat-vec passes: 2 / 1
    constexpr int ES_ROWS = ES_BYTES / (4 * D);
    __shared__ float es[ES_ROWS * D];
    __shared__ float AE[2][MAX_R][D];
    __shared__ float P[3][2][MAX_R][D];
    __shared__ __attribute__((aligned(16))) float G[2][MAX_R][D];
    __shared__ float x[4][2][D];
    __shared__ float dx[2][D];
    __shared__ float dz[2][D];
    __shared__ float w[3][MAX_R];
    __shared__ float sm[3][MAX_R];
    __shared__ float zs[MAX_R];
    __shared__ float da[MAX_R];
    __shared__ float du[MAX_R];
    __shared__ float cnt[MAX_R];
    __shared__ float gsr[MAX_R];
    __shared__ float smv[CH];                  // the masked values of a pass, and as multipliers of the two AE rows
    __shared__ float smvh[CH];
    __shared__ float smvt[CH];
    __shared__ int scol[CH];
    __shared__ int rstart[MAX_R + 1];
    __shared__ float sc[3];                    // before, -before / (p + 1e-5), p (1 - p)

    const int tid = threadIdx.x;
    const int R = a.R;
    const int q = a.qids[blockIdx.x];
    const int hh = a.h[q], rr = a.r[q], tt = a.t[q];
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    const int step0 = a.epochs_base + q * a.num_epochs;
    const int* ent = a.entry + c0;
    const int* crel = a.crel + c0;
    const int* ccol = a.ccol + c0;
    const int* crole = a.crole + c0;
    float* mk = a.out + c0;
    const int k = tid % D, grp = tid / D;
    const int side2 = (tid / D) & 1;           // the (side, column) a thread owns in the 2 D wide passes

    // load: lazily decayed moments, the mask at its init value, the relation segments of the candidate list
    if (tid <= MAX_R) rstart[tid] = n;
    __syncthreads();
    for (int j = tid; j < n; j += NT) {
        const int e = ent[j];
        const int gap = step0 - a.steps[e];
        if (gap > 0) {
            a.m[e] *= powf(a.b1, (float)gap);
            a.v[e] *= powf(a.b2, (float)gap);
        }
        mk[j] = a.init_e[e];
        rstart_mark(rstart, crel, j);
    }
    if (tid < 2 * D) x[0][side2][k] = a.E[(size_t)(side2 ? tt : hh) * D + k];
    stage_es<D, ES_ROWS>(es, a.E, ccol, n);
    __syncthreads();

    for (int ep = -1; ep < a.num_epochs; ++ep) {
        // AE rows of h and t (and the relation sums of the masked values), candidates ascending
        {
            // group grp owns relations grp, grp + GR; a candidate that feeds neither row (or one only) enters with a
            // zero multiplier: fmaf(0, e, acc) is acc
            float ah[RPG], at[RPG], cacc[RPG];
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) ah[ri] = at[ri] = cacc[ri] = 0.f;
            for (int cb = 0; cb == 0 || cb < n; cb += CH) {
                const int ce = cb + CH < n ? cb + CH : n;
                for (int j = cb + tid; j < ce; j += NT) {
                    const float mv = ep < 0 ? 1.0f : sigmoid_ref(mk[j]);
                    const int role = crole[j];
                    smv[j - cb] = mv;
                    smvh[j - cb] = (role & 1) ? mv : 0.f;
                    smvt[j - cb] = (role & 2) ? mv : 0.f;
                    scol[j - cb] = ccol[j];
                }
                __syncthreads();
#pragma unroll
                for (int ri = 0; ri < RPG; ++ri) {
                    const int r = grp + ri * GR;
                    if (r < R) {
                        const int j0 = rstart[r] > cb ? rstart[r] : cb;
                        const int j1 = rstart[r + 1] < ce ? rstart[r + 1] : ce;
                        const int jl = j0 > ES_ROWS ? j0 : ES_ROWS;
                        const int jm = jl < j1 ? jl : j1;             // [j0, jm): E rows in LDS, [jm, j1): global
#pragma unroll 4
                        for (int j = j0; j < jm; ++j) {
                            const float ev = es[j * D + k];
                            ah[ri] = fmaf(smvh[j - cb], ev, ah[ri]);
                            at[ri] = fmaf(smvt[j - cb], ev, at[ri]);
                            cacc[ri] += smv[j - cb];
                        }
                        for (int j = jm; j < j1; ++j) {
                            const float mh = smvh[j - cb], mt = smvt[j - cb];
                            if (mh != 0.f || mt != 0.f) {
                                const float ev = a.E[(size_t)scol[j - cb] * D + k];
                                ah[ri] = fmaf(mh, ev, ah[ri]);
                                at[ri] = fmaf(mt, ev, at[ri]);
                            }
                            cacc[ri] += smv[j - cb];
                        }
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) {
                const int r = grp + ri * GR;
                if (r < R) {
                    AE[0][r][k] = ah[ri];
                    AE[1][r][k] = at[ri];
                    if (k == 0) cnt[r] = cacc[ri];
                }
            }
        }
        __syncthreads();

        // forward: the reference layer on the two rows
        for (int l = 0; l < 3; ++l) {
            for (int r = grp; r < R; r += GR) {
                const float z = group_sum<D>(x[l][0][k] * a.Wa[l][(size_t)k * R + r]);
                if (k == 0) zs[r] = z + a.ba[l][r];
                float ph, pt;
                matvec2<D>(a.K[l] + (size_t)r * D * D + k, AE[0][r], AE[1][r], ph, pt);
                P[l][0][r][k] = ph;
                P[l][1][r][k] = pt;
            }
            __syncthreads();
            if (tid < R) {
                const float s = rel_softmax(zs, R, tid);
                sm[l][tid] = s;
                w[l][tid] = sigmoid_ref(s);
            }
            __syncthreads();
            if (tid < 2 * D) {
                float v = matvec1<D>(a.S[l] + k, x[l][side2]);
                for (int r = 0; r < R; ++r) v = fmaf(w[l][r], P[l][side2][r][k], v);
                x[l + 1][side2][k] = sigmoid_ref(v);
            }
            __syncthreads();
        }
        float s_dm = 0.f;
        if (tid < D) s_dm = group_sum<D>(x[3][0][k] * a.rel[(size_t)rr * D + k] * x[3][1][k]);
        if (tid == 0) {
            const float p = sigmoid_ref(s_dm);
            if (ep < 0) sc[0] = p;
            sc[1] = -sc[0] / (p + 1e-5f);
            sc[2] = p * (1.0f - p);
            // the relation-ratio loss: its gradient w.r.t. the masked values of relation r
            if (a.target_ratios && ep >= 0) {
                float C = 0.f, dot = 0.f, dr[MAX_R];
#pragma unroll
                for (int r = 0; r < MAX_R; ++r)
                    if (r < R) C += cnt[r];
#pragma unroll
                for (int r = 0; r < MAX_R; ++r)
                    if (r < R) {
                        const float ratio = cnt[r] / C;
                        dr[r] = 2.0f * (ratio - a.target_ratios[r]) / (float)R;
                        dot = fmaf(dr[r], ratio, dot);
                    }
#pragma unroll
                for (int r = 0; r < MAX_R; ++r)
                    if (r < R) gsr[r] = (dr[r] - dot) / C;
            }
        }
        __syncthreads();
        if (ep < 0) continue;

        // backward of p: GH, GT
        if (tid < 2 * D) dx[side2][k] = sc[2] * a.rel[(size_t)rr * D + k] * x[3][1 - side2][k];
        float Gh[RPG], Gt[RPG];
#pragma unroll
        for (int ri = 0; ri < RPG; ++ri) Gh[ri] = Gt[ri] = 0.f;
        __syncthreads();
        for (int l = 2; l >= 0; --l) {
            if (tid < 2 * D) {
                const float xv = x[l + 1][side2][k];
                dz[side2][k] = dx[side2][k] * (xv * (1.0f - xv));
            }
            __syncthreads();
            // G_r += w_lr (dz K^l_r^T), from the transposed K: group grp owns relations grp, grp + GR; and the dynamic
            // weights' dw_r = <dzh, P^l_r[h]> + <dzt, P^l_r[t]>, through the sigmoid
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) {
                const int r = grp + ri * GR;
                if (r < R) {
                    float gh, gt;
                    matvec2<D>(a.KT[l] + (size_t)r * D * D + k, dz[0], dz[1], gh, gt);
                    const float wv = w[l][r];
                    Gh[ri] = fmaf(wv, gh, Gh[ri]);
                    Gt[ri] = fmaf(wv, gt, Gt[ri]);
                    if (l > 0) {
                        const float dw = group_sum<D>(fmaf(dz[0][k], P[l][0][r][k], dz[1][k] * P[l][1][r][k]));
                        if (k == 0) da[r] = dw * (wv * (1.0f - wv));
                    }
                }
            }
            if (l == 0) break;
            __syncthreads();
            // through the softmax
            if (tid < R) du[tid] = rel_softmax_bwd(sm[l], da, R, tid);
            __syncthreads();
            // dx^{l-1} = dz S^l^T (+ du Walpha^l^T on the head side), from the transposed S in global memory
            if (tid < 2 * D)
                dx[side2][k] = dx_step<D>(a.ST[l] + k, dz[side2], side2 == 0, du, a.Wa[l] + (size_t)k * R, R);
            __syncthreads();
        }
#pragma unroll
        for (int ri = 0; ri < RPG; ++ri)
            if (grp + ri * GR < R) {
                G[0][grp + ri * GR][k] = Gh[ri];
                G[1][grp + ri * GR][k] = Gt[ri];
            }
        __syncthreads();

        // per candidate: the gradient w.r.t. its mask, one dense-form Adam step
        const float factor = sc[1];
        const float alpha = a.alpha[step0 + ep];
        for (int j = tid; j < n; j += NT) {
            const int role = crole[j], rl = crel[j], e = ent[j];
            const f32x4* e4 = (const f32x4*)(a.E + (size_t)ccol[j] * D);
            float dot = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (role & (1 << s)) {
                    const f32x4* g4 = (const f32x4*)G[s][rl];
                    f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < D / 4; ++i) {
                        const f32x4 ev = e4[i], gv = g4[i];
#pragma unroll
                        for (int c = 0; c < 4; ++c) c4[c] = fmaf(gv[c], ev[c], c4[c]);
                    }
                    dot += (c4[0] + c4[1]) + (c4[2] + c4[3]);
                }
            float g = dot * factor;
            if (a.target_ratios) g = (g + gsr[rl]) * 0.5f;
            const float mkj = mk[j];
            const float mv = sigmoid_ref(mkj);
            g = g * mv * (1.0f - mv);
            float mi = a.m[e], vi = a.v[e];
            mi = mi + (g - mi) * (1.0f - a.b1);
            vi = vi + (g * g - vi) * (1.0f - a.b2);
            a.m[e] = mi;
            a.v[e] = vi;
            mk[j] = mkj - (mi * alpha) / (sqrtf(vi) + a.eps);
        }
    }

    for (int j = tid; j < n; j += NT) {
        mk[j] = sigmoid_ref(mk[j]);
        a.steps[ent[j]] = step0 + a.num_epochs;
    }
}

// ---- deletion / insertion curves -------------------------------------------------------------------------------
// curves_kernel: one workgroup per (query, tile of CV_VT variants); a variant is one edited copy of the query's two
// adjacency rows, so a tile is CV_ROWS = 2 CV_VT row vectors (2 u: the head row of variant u, 2 u + 1: its tail row).
// The candidates' E rows are staged once (the first ES_ROWS; the others come from global memory) and every variant's
// AE rows are built from them; then the mask explainer's forward runs on all rows of the tile at once: a thread loads
// its column of K^l_r (or S^l) 32 elements at a time and applies it to every row before the next load, so a weight
// element read serves CV_ROWS fmaf.  AE, P and the activations live in LDS; group grp of D lanes owns relations grp,
// grp + GR in the AE and P passes and rows grp RW .. in the combine.  The sums are matvec2's: four fmaf chains per
// element, (c0 + c1) + (c2 + c3); a row's arithmetic does not depend on its place in the tile.
//   LDS at D = 64: es 80 KB + AE 32 KB + P 32 KB + x 8 KB + 0.5 KB = 152.5 KB of the CU's 160 KB (one workgroup per CU).
constexpr int CV_VT = 8;
constexpr int CV_ROWS = 2 * CV_VT;
constexpr int CV_ES_BYTES = 80 * 1024;     // E rows kept in LDS: 320 candidates at d = 64, 640 at d = 32

// column k of rows · M for NR row vectors (LDS, stride `rs` floats, 16-byte aligned): Mk = M + k, M (D, D) row-major
template <int D, int NR>
__device__ __forceinline__ void matvec_rows(const float* __restrict__ Mk, const float* rows, int rs, float* y) {
    float c4[NR][4];
#pragma unroll
    for (int j = 0; j < NR; ++j) c4[j][0] = c4[j][1] = c4[j][2] = c4[j][3] = 0.f;
#pragma unroll
    for (int i0 = 0; i0 < D; i0 += 32) {
        float kv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) kv[u] = Mk[(size_t)(i0 + u) * D];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 32; u += 4)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const f32x4 av = *(const f32x4*)(rows + j * rs + i0 + u);
#pragma unroll
                for (int c = 0; c < 4; ++c) c4[j][(u >> 3) & 3] = fmaf(av[c], kv[u + c], c4[j][(u >> 3) & 3]);
            }
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) y[j] = (c4[j][0] + c4[j][1]) + (c4[j][2] + c4[j][3]);
}

// The variant tile of curves_kernel and cf_step_kernel: its LDS block and every step from the staging to a variant's
// score, written once, so that the two kernels run one forward (tests/test_gpu_counterfactual.py holds their outputs
// equal bit for bit).  A kernel adds its variant table, its keep rule and its store rule.  `a` is the kernel's
// argument struct (E, rel, the candidate arrays, the layers' K, S, Wa, ba), c0 the start of the query's candidates.
template <int D>
struct Tile {
    static constexpr int GR = NT / D;                 // groups of D lanes: 4 / 8
    static constexpr int RPG = MAX_R / GR;            // relations per group: 2 / 1
    static constexpr int RW = CV_ROWS / GR;           // rows per group in the combine: 4 / 2
    static constexpr int ES_ROWS = CV_ES_BYTES / (4 * D);
    float es[ES_ROWS * D];
    float AE[MAX_R][CV_ROWS][D];               // AE and x are read 16 bytes at a time: a kernel declares the block
    float P[MAX_R][CV_ROWS][D];                // aligned(16), and their offsets are multiples of 16 (tile_forward)
    float x[2][CV_ROWS][D];
    float zs[CV_VT][MAX_R];
    float w[CV_VT][MAX_R];
    int rstart[MAX_R + 1];
};

// with `stage` (once per workgroup): the relation segments of the candidate list and the staged E rows; then
// x^0 = E[h] / E[t] in every variant, and the barrier that publishes all of it
template <int D, class A>
__device__ __forceinline__ void tile_begin(Tile<D>& T, const A& a, long long c0, int n, int hh, int tt, bool stage) {
    if (stage) {
        rstart_scan(T.rstart, a.crel + c0, n);
        stage_es<D, Tile<D>::ES_ROWS>(T.es, a.E, a.ccol + c0, n);
    }
    for (int idx = threadIdx.x; idx < CV_ROWS * D; idx += NT) {
        const int row = idx / D;
        T.x[0][row][idx % D] = a.E[(size_t)((row & 1) ? tt : hh) * D + idx % D];
    }
    __syncthreads();
}

// AE rows of every variant: candidates ascending, one chain per (row, relation, column).  keep(j, kp), called once per
// candidate, says which of the tile's variants keep it; a candidate a variant drops (or that does not feed the side)
// enters with a zero multiplier: fmaf(0, e, acc) is acc
template <int D, class A, class Keep>
__device__ __forceinline__ void tile_ae(Tile<D>& T, const A& a, long long c0, const Keep& keep) {
    constexpr int GR = Tile<D>::GR, ES_ROWS = Tile<D>::ES_ROWS;
    const int k = threadIdx.x % D, grp = threadIdx.x / D;
    const int* ccol = a.ccol + c0;
    const int* crole = a.crole + c0;
    const float* cval = a.cval + c0;
#pragma unroll
    for (int ri = 0; ri < Tile<D>::RPG; ++ri) {
        const int r = grp + ri * GR;
        if (r < a.R) {
            float acc[CV_ROWS];
#pragma unroll
            for (int j = 0; j < CV_ROWS; ++j) acc[j] = 0.f;
            const int j1 = T.rstart[r + 1];
            for (int j = T.rstart[r]; j < j1; ++j) {
                const float val = cval[j];
                const int role = crole[j];
                bool kp[CV_VT];
                keep(j, kp);
                const float ev = j < ES_ROWS ? T.es[j * D + k] : a.E[(size_t)ccol[j] * D + k];
                const float vh = (role & 1) ? val : 0.f, vt = (role & 2) ? val : 0.f;
#pragma unroll
                for (int u = 0; u < CV_VT; ++u) {
                    acc[2 * u] = fmaf(kp[u] ? vh : 0.f, ev, acc[2 * u]);
                    acc[2 * u + 1] = fmaf(kp[u] ? vt : 0.f, ev, acc[2 * u + 1]);
                }
            }
#pragma unroll
            for (int j = 0; j < CV_ROWS; ++j) T.AE[r][j][k] = acc[j];
        }
    }
    __syncthreads();
}

// forward: the reference layer on the CV_ROWS rows, three times; x^3 is left in x[1], behind a barrier
template <int D, class A>
__device__ __forceinline__ void tile_forward(Tile<D>& T, const A& a) {
    static_assert(offsetof(Tile<D>, AE) % 16 == 0 && offsetof(Tile<D>, x) % 16 == 0, "matvec_rows reads f32x4");
    constexpr int GR = Tile<D>::GR, RW = Tile<D>::RW;
    const int tid = threadIdx.x, k = tid % D, grp = tid / D;
    const int R = a.R;
    for (int l = 0; l < 3; ++l) {
        const int cur = l & 1;
        for (int item = grp; item < CV_VT * R; item += GR) {
            const int u = item / R, r = item % R;
            const float z = group_sum<D>(T.x[cur][2 * u][k] * a.Wa[l][(size_t)k * R + r]);
            if (k == 0) T.zs[u][r] = z + a.ba[l][r];
        }
#pragma unroll
        for (int ri = 0; ri < Tile<D>::RPG; ++ri) {
            const int r = grp + ri * GR;
            if (r < R) {
                float y[CV_ROWS];
                matvec_rows<D, CV_ROWS>(a.K[l] + (size_t)r * D * D + k, &T.AE[r][0][0], D, y);
#pragma unroll
                for (int j = 0; j < CV_ROWS; ++j) T.P[r][j][k] = y[j];
            }
        }
        __syncthreads();
        if (tid < CV_VT * R) T.w[tid / R][tid % R] = sigmoid_ref(rel_softmax(T.zs[tid / R], R, tid % R));
        __syncthreads();
        {
            float y[RW];
            matvec_rows<D, RW>(a.S[l] + k, &T.x[cur][grp * RW][0], D, y);
#pragma unroll
            for (int j = 0; j < RW; ++j) {
                const int row = grp * RW + j;
                float v = y[j];
                for (int r = 0; r < R; ++r) v = fmaf(T.w[row >> 1][r], T.P[r][row][k], v);
                T.x[1 - cur][row][k] = sigmoid_ref(v);
            }
        }
        __syncthreads();
    }
}

// the DistMult score of variant u against the relation row rl, the same value in every lane of the calling group
template <int D>
__device__ __forceinline__ float tile_score(const Tile<D>& T, const float* rl, int u) {
    const int k = threadIdx.x % D;
    return sigmoid_ref(group_sum<D>(T.x[1][2 * u][k] * rl[k] * T.x[1][2 * u + 1][k]));
}

// curves_kernel's variants: 0 .. k are the deletion points, k + 1 .. 2 k + 1 the insertion points.  Variant u keeps a
// candidate when "flipped within the first pt[u] steps" equals isins[u]
struct CurvesKeep {
    const int* cstep;
    int pt[CV_VT];
    bool isins[CV_VT];
    __device__ __forceinline__ void operator()(int j, bool* kp) const {
        const int st = cstep[j];
#pragma unroll
        for (int u = 0; u < CV_VT; ++u) kp[u] = (st >= 0 && st < pt[u]) == isins[u];
    }
};

template <int D>
__global__ __launch_bounds__(NT) void curves_kernel(const iddgcn_explain_curves_t a, int n_tiles) {
    __shared__ __attribute__((aligned(16))) Tile<D> T;
    const int q = blockIdx.x / n_tiles;
    const int v0 = (blockIdx.x % n_tiles) * CV_VT;
    const int nv = 2 * (a.k + 1);
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    const float* rl = a.rel + (size_t)a.r[q] * D;

    // variants past the last repeat it (computed, never stored)
    CurvesKeep keep;
    keep.cstep = a.cstep + c0;
#pragma unroll
    for (int u = 0; u < CV_VT; ++u) {
        const int vi = v0 + u < nv ? v0 + u : nv - 1;
        keep.isins[u] = vi > a.k;
        keep.pt[u] = keep.isins[u] ? vi - (a.k + 1) : vi;
    }

    tile_begin<D>(T, a, c0, n, a.h[q], a.t[q], true);
    tile_ae<D>(T, a, c0, keep);
    tile_forward<D>(T, a);
    for (int u = threadIdx.x / D; u < CV_VT; u += Tile<D>::GR) {
        const float p = tile_score<D>(T, rl, u);
        const int vi = v0 + u;
        if (threadIdx.x % D == 0 && vi < nv) {
            float* out = vi > a.k ? a.ins + (size_t)q * (a.k + 1) + (vi - (a.k + 1)) : a.del + (size_t)q * (a.k + 1) + vi;
            *out = p;
        }
    }
}

// ---- counterfactual search -------------------------------------------------------------------------------------
// cf_step_kernel: step `step` of the greedy search on curves_kernel's tile (Tile and the tile_ functions above: one
// LDS block, one staging, one set of AE chains, one forward for both kernels), with its own variants.  With F the
// candidates removed so far (cstep >= 0; nothing at step 0, where cstep is not initialised and not read), variant 0 is
// F itself and variant 1 + j drops candidate j and its partner too.  A variant is stored when it is the base at step 0
// (path[q][0]) or an eligible candidate outside F (vals[j]); the others are computed and dropped.  Workgroup b of a
// query's `tiles` takes the tiles b, b + tiles, .. of 8 variants, so the E rows are staged once and the grid need not
// know the segment's length.  The variant table lives in registers.
struct CfKeep {
    const int* cstep;
    bool later;                                // step > 0
    int jv[CV_VT], pv[CV_VT];                  // the candidate a variant drops and its partner, -1: none
    __device__ __forceinline__ void operator()(int j, bool* kp) const {
        const bool gone = later && cstep[j] >= 0;
#pragma unroll
        for (int u = 0; u < CV_VT; ++u) kp[u] = !gone && j != jv[u] && j != pv[u];
    }
};

template <int D>
__global__ __launch_bounds__(NT) void cf_step_kernel(const iddgcn_counterfactual_t a, int step, int tiles,
                                                     float* __restrict__ vals) {
    __shared__ __attribute__((aligned(16))) Tile<D> T;
    const int q = blockIdx.x / tiles;
    // a query that has stopped: flipped, or the step before this one was not taken
    if (step > 0 && (a.flipped[q] || a.n_steps[q] != step)) return;
    const int hh = a.h[q], tt = a.t[q];
    const float* rl = a.rel + (size_t)a.r[q] * D;
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    const int nv = n + 1;
    const int* cpartner = a.cpartner + c0;
    const int* celig = a.celig + c0;
    CfKeep keep;
    keep.cstep = a.cstep + c0;
    keep.later = step > 0;
    bool staged = false;

    for (int v0 = (blockIdx.x % tiles) * CV_VT; v0 < nv; v0 += tiles * CV_VT) {
        // variants past the last repeat it (computed, never stored)
        bool store[CV_VT];
        bool any = false;
#pragma unroll
        for (int u = 0; u < CV_VT; ++u) {
            const int vi = v0 + u < nv ? v0 + u : nv - 1;
            keep.jv[u] = vi - 1;
            keep.pv[u] = -1;
            store[u] = false;
            if (v0 + u < nv) {
                if (vi == 0) {
                    store[u] = step == 0;
                } else {
                    keep.pv[u] = cpartner[vi - 1];
                    store[u] = celig[vi - 1] != 0 && (step == 0 || keep.cstep[vi - 1] < 0);
                }
            }
            any = any || store[u];
        }
        if (!any) continue;                    // uniform over the workgroup

        tile_begin<D>(T, a, c0, n, hh, tt, !staged);       // the last tile's readers of x are past a barrier
        staged = true;
        tile_ae<D>(T, a, c0, keep);
        tile_forward<D>(T, a);
        for (int u = threadIdx.x / D; u < CV_VT; u += Tile<D>::GR) {
            const float p = tile_score<D>(T, rl, u);
            // a stored variant is v0 + u itself: the base, or the one that drops candidate v0 + u - 1.  (The keep table
            // is indexed by constants only, so it stays in registers.)
            if (threadIdx.x % D == 0 && store[u]) {
                if (v0 + u == 0)
                    a.path[(size_t)q * (a.k + 1)] = p;
                else
                    vals[c0 + v0 + u - 1] = p;
            }
        }
        __syncthreads();                       // x[1] is read above, x[0] rewritten by the next tile
    }
}

// the candidate of the smallest dir * p first, equal bit patterns: the lowest index (p is a sigmoid: never negative)
__device__ __forceinline__ unsigned long long cf_key(float p, int lower, int j) {
    const unsigned u = __float_as_uint(p);
    return ((unsigned long long)(lower ? u : ~u) << 32) | (unsigned)j;
}

// cf_select_kernel: one workgroup per query, step `step` (choose = 0: K = 0, only the bookkeeping of step 0).
__global__ __launch_bounds__(NT) void cf_select_kernel(const iddgcn_counterfactual_t a, int step, int choose,
                                                       const float* __restrict__ vals) {
    __shared__ unsigned long long best[NT];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int K = a.k;
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    float* path = a.path + (size_t)q * (K + 1);
    const float p0 = path[0];
    const float thr = a.threshold;
    const int lower = a.mode == IDDGCN_CF_LOWER || (a.mode == IDDGCN_CF_FLIP && p0 > thr);
    int active;
    if (step == 0) {
        active = lower ? p0 > thr : !(p0 > thr);           // not yet on the target side
        for (int j = tid; j < n; j += NT) {
            a.cstep[c0 + j] = -1;
            if (!a.celig[c0 + j]) a.loo[c0 + j] = __int_as_float(0x7fc00000);
        }
    } else {
        active = !a.flipped[q] && a.n_steps[q] == step;
    }
    unsigned long long key = ~0ull;
    if (active && choose)
        for (int j = tid; j < n; j += NT)
            if (a.celig[c0 + j] && (step == 0 || a.cstep[c0 + j] < 0)) {
                const unsigned long long kj = cf_key(vals[c0 + j], lower, j);
                key = kj < key ? kj : key;
            }
    best[tid] = key;
    __syncthreads();                                       // also orders step 0's cstep = -1 before the choice's writes
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s && best[tid + s] < best[tid]) best[tid] = best[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    key = best[0];
    const bool take = key != ~0ull;                        // an eligible candidate was left
    if (take) {
        const int j = (int)(unsigned)key;
        const float p = vals[c0 + j];
        const int pj = a.cpartner[c0 + j];
        a.cstep[c0 + j] = step;
        if (pj >= 0 && pj < n) a.cstep[c0 + pj] = step;
        a.chosen[(size_t)q * K + step] = j;
        path[step + 1] = p;
        a.n_steps[q] = step + 1;
        a.flipped[q] = lower ? !(p > thr) : p > thr;
    } else {
        if (choose) {
            a.chosen[(size_t)q * K + step] = -1;
            path[step + 1] = path[step];
        }
        if (step == 0) {
            a.n_steps[q] = 0;
            a.flipped[q] = !active;
        }
    }
}

// ---- integrated gradients over the adjacency values --------------------------------------------------------------
// ig_path_kernel: one workgroup per (query, chunk of IG_CHUNK quadrature nodes).  The path scales the eligible
// candidates' values by alpha, so AE(alpha) = F + alpha U and every projection is PF + alpha PU: F, U (one fmaf chain
// per column, candidates ascending) and the 2 x 3 R projections per side are built once per workgroup, as are the
// layer-1 terms E[h] S^1, E[t] S^1 and the layer-1 dynamic weights.  S^2, S^3 and their transposes sit in LDS, so a
// node reads no global memory but its (alpha, omega).  Per node: the mask explainer's forward and backward (scale 1)
// up to dz; the backward's K^T products are linear in dz, so the node loop only accumulates
// acc[l][side][r] += omega w_lr dz^l[side] (nodes ascending) and ig_finish_kernel applies K^T once.  Chunk 0 also
// evaluates the two end points (forward only): p_base = f(0), p_full = f(1).
//   LDS at D = 64: S 32 KB + S^T 32 KB + PF, PU 24 KB + P 8 KB + acc 12 KB + AE 8 KB + Wa 4 KB + 3 KB = 123 KB.
// ig_finish_kernel: one workgroup per query sums the chunks' accumulators in chunk order, applies K^T (layers
// ascending), and gives every candidate its attribution, one candidate per thread from global memory (a row of any
// length); total is a fixed tree over the threads' strided partial sums.
constexpr int IG_CHUNK = 32;               // quadrature nodes per workgroup

struct PathP {
    iddgcn_explain_path_t a;
    int nch;                               // chunks per query: ceil(m / IG_CHUNK)
};

template <int D>
__global__ __launch_bounds__(NT) void ig_path_kernel(const PathP pp) {
    constexpr int GR = NT / D;
    constexpr int RPG = MAX_R / GR;
    __shared__ float Sm[2][D * D];             // S^2, S^3
    __shared__ float STm[2][D * D];            // their transposes
    __shared__ float PF[3][2][MAX_R][D];
    __shared__ float PU[3][2][MAX_R][D];
    __shared__ float P[2][2][MAX_R][D];        // P^2, P^3 at the node's alpha (the backward's dw reads them)
    __shared__ float acc[3][2][MAX_R][D];
    __shared__ float AEF[2][MAX_R][D];
    __shared__ float AEU[2][MAX_R][D];
    __shared__ float Was[2][D * MAX_R];        // Walpha^2, Walpha^3
    __shared__ float bas[2][MAX_R];
    __shared__ float x[4][2][D];
    __shared__ float c1[2][D];                 // E[h] S^1, E[t] S^1
    __shared__ float dx[2][D];
    __shared__ float dz[2][D];
    __shared__ float rels[D];
    __shared__ float w[3][MAX_R];
    __shared__ float sm[3][MAX_R];
    __shared__ float zs[MAX_R];
    __shared__ float da[MAX_R];
    __shared__ float du[MAX_R];
    __shared__ int rstart[MAX_R + 1];
    __shared__ float sc[1];                    // p (1 - p)

    const iddgcn_explain_path_t& a = pp.a;
    const int tid = threadIdx.x;
    const int R = a.R;
    const int q = blockIdx.x / pp.nch;
    const int chunk = blockIdx.x % pp.nch;
    const int hh = a.h[q], rr = a.r[q], tt = a.t[q];
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    const int* crel = a.crel + c0;
    const int* ccol = a.ccol + c0;
    const int* crole = a.crole + c0;
    const int* celig = a.celig + c0;
    const float* cval = a.cval + c0;
    const int k = tid % D, grp = tid / D;
    const int side2 = (tid / D) & 1;

    // the relation segments of the candidate list, x^0, the staged matrices
    rstart_scan(rstart, crel, n);
    if (tid < 2 * D) x[0][side2][k] = a.E[(size_t)(side2 ? tt : hh) * D + k];
    if (tid < D) rels[k] = a.rel[(size_t)rr * D + k];
    for (int idx = tid; idx < D * D; idx += NT) {
        Sm[0][idx] = a.S[1][idx];
        Sm[1][idx] = a.S[2][idx];
        STm[0][idx] = a.ST[1][idx];
        STm[1][idx] = a.ST[2][idx];
    }
    for (int idx = tid; idx < D * R; idx += NT) {
        Was[0][idx] = a.Wa[1][idx];
        Was[1][idx] = a.Wa[2][idx];
    }
    if (tid < R) {
        bas[0][tid] = a.ba[1][tid];
        bas[1][tid] = a.ba[2][tid];
    }
    for (int idx = tid; idx < 3 * 2 * MAX_R * D; idx += NT) (&acc[0][0][0][0])[idx] = 0.f;
    __syncthreads();

    // F and U: the fixed and the eligible part of the AE rows, candidates ascending; a candidate that does not feed a
    // part enters it with a zero multiplier: fmaf(0, e, acc) is acc
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        const int r = grp + ri * GR;
        if (r < R) {
            float fh = 0.f, ft = 0.f, uh = 0.f, ut = 0.f;
            const int j1 = rstart[r + 1];
            for (int j = rstart[r]; j < j1; ++j) {
                const float val = cval[j];
                const int role = crole[j];
                const bool el = celig[j] != 0;
                const float ev = a.E[(size_t)ccol[j] * D + k];
                const float vh = (role & 1) ? val : 0.f, vt = (role & 2) ? val : 0.f;
                fh = fmaf(el ? 0.f : vh, ev, fh);
                ft = fmaf(el ? 0.f : vt, ev, ft);
                uh = fmaf(el ? vh : 0.f, ev, uh);
                ut = fmaf(el ? vt : 0.f, ev, ut);
            }
            AEF[0][r][k] = fh;
            AEF[1][r][k] = ft;
            AEU[0][r][k] = uh;
            AEU[1][r][k] = ut;
        }
    }
    __syncthreads();

    // the projections of both parts, the layer-1 logits
    for (int l = 0; l < 3; ++l)
        for (int r = grp; r < R; r += GR) {
            float ph, pt;
            matvec2<D>(a.K[l] + (size_t)r * D * D + k, AEF[0][r], AEF[1][r], ph, pt);
            PF[l][0][r][k] = ph;
            PF[l][1][r][k] = pt;
            matvec2<D>(a.K[l] + (size_t)r * D * D + k, AEU[0][r], AEU[1][r], ph, pt);
            PU[l][0][r][k] = ph;
            PU[l][1][r][k] = pt;
        }
    for (int r = grp; r < R; r += GR) {
        const float z = group_sum<D>(x[0][0][k] * a.Wa[0][(size_t)k * R + r]);
        if (k == 0) zs[r] = z + a.ba[0][r];
    }
    if (tid < 2 * D) c1[side2][k] = matvec1<D>(a.S[0] + k, x[0][side2]);
    __syncthreads();
    if (tid < R) {
        const float s = rel_softmax(zs, R, tid);
        sm[0][tid] = s;
        w[0][tid] = sigmoid_ref(s);
    }
    __syncthreads();

    const int i0 = chunk * IG_CHUNK;
    const int cnt = a.m - i0 < IG_CHUNK ? a.m - i0 : IG_CHUNK;
    for (int it = chunk == 0 ? -2 : 0; it < cnt; ++it) {
        // it = -2, -1: the end points alpha = 0, 1, forward only
        const float al = it < 0 ? (float)(it + 2) : a.alpha[i0 + it];
        const float om = it < 0 ? 0.f : a.omega[i0 + it];

        // forward; layer 1 from its constant terms
        if (tid < 2 * D) {
            float v = c1[side2][k];
            for (int r = 0; r < R; ++r) v = fmaf(w[0][r], fmaf(al, PU[0][side2][r][k], PF[0][side2][r][k]), v);
            x[1][side2][k] = sigmoid_ref(v);
        }
        __syncthreads();
        for (int l = 1; l < 3; ++l) {
            for (int r = grp; r < R; r += GR) {
                const float z = group_sum<D>(x[l][0][k] * Was[l - 1][k * R + r]);
                if (k == 0) zs[r] = z + bas[l - 1][r];
            }
            for (int idx = tid; idx < 2 * R * D; idx += NT) {
                const int s = idx / (R * D), r = (idx / D) % R, c = idx % D;
                P[l - 1][s][r][c] = fmaf(al, PU[l][s][r][c], PF[l][s][r][c]);
            }
            __syncthreads();
            if (tid < R) {
                const float s = rel_softmax(zs, R, tid);
                sm[l][tid] = s;
                w[l][tid] = sigmoid_ref(s);
            }
            __syncthreads();
            if (tid < 2 * D) {
                float v = matvec1<D>(&Sm[l - 1][k], x[l][side2]);
                for (int r = 0; r < R; ++r) v = fmaf(w[l][r], P[l - 1][side2][r][k], v);
                x[l + 1][side2][k] = sigmoid_ref(v);
            }
            __syncthreads();
        }
        float s_dm = 0.f;
        if (tid < D) s_dm = group_sum<D>(x[3][0][k] * rels[k] * x[3][1][k]);
        if (tid == 0) {
            const float p = sigmoid_ref(s_dm);
            sc[0] = p * (1.0f - p);
            if (it == -2) a.p_base[q] = p;
            if (it == -1) a.p_full[q] = p;
        }
        __syncthreads();
        if (it < 0) continue;                  // uniform over the workgroup

        // backward up to dz of every layer
        if (tid < 2 * D) dx[side2][k] = sc[0] * rels[k] * x[3][1 - side2][k];
        __syncthreads();
        for (int l = 2; l >= 0; --l) {
            if (tid < 2 * D) {
                const float xv = x[l + 1][side2][k];
                dz[side2][k] = dx[side2][k] * (xv * (1.0f - xv));
            }
            __syncthreads();
            for (int idx = tid; idx < 2 * R * D; idx += NT) {
                const int s = idx / (R * D), r = (idx / D) % R, c = idx % D;
                acc[l][s][r][c] = fmaf(om * w[l][r], dz[s][c], acc[l][s][r][c]);
            }
            if (l == 0) break;
            // through the dynamic weights: dw_r = <dzh, P^l_r[h]> + <dzt, P^l_r[t]>, the sigmoid, the softmax
            for (int r = grp; r < R; r += GR) {
                const float dw = group_sum<D>(fmaf(dz[0][k], P[l - 1][0][r][k], dz[1][k] * P[l - 1][1][r][k]));
                const float wv = w[l][r];
                if (k == 0) da[r] = dw * (wv * (1.0f - wv));
            }
            __syncthreads();
            if (tid < R) du[tid] = rel_softmax_bwd(sm[l], da, R, tid);
            __syncthreads();
            // dx^{l-1} = dz S^l^T (+ du Walpha^l^T on the head side), from the LDS copies
            if (tid < 2 * D)
                dx[side2][k] = dx_step<D>(&STm[l - 1][k], dz[side2], side2 == 0, du, &Was[l - 1][k * R], R);
            __syncthreads();
        }
    }
    __syncthreads();

    // the chunk's accumulators, [l][side][r][column] with R relations
    float* out = a.scratch + ((size_t)q * pp.nch + chunk) * (size_t)(6 * R * D);
    for (int idx = tid; idx < 6 * R * D; idx += NT) {
        const int ls = idx / (R * D), r = (idx / D) % R, c = idx % D;
        out[idx] = acc[ls >> 1][ls & 1][r][c];
    }
}

template <int D>
__global__ __launch_bounds__(NT) void ig_finish_kernel(const PathP pp) {
    constexpr int GR = NT / D;
    __shared__ float A[3][2][MAX_R][D];
    __shared__ __attribute__((aligned(16))) float G[2][MAX_R][D];
    __shared__ float red[NT];
    const iddgcn_explain_path_t& a = pp.a;
    const int tid = threadIdx.x;
    const int R = a.R;
    const int q = blockIdx.x;
    const long long c0 = a.qptr[q];
    const int n = (int)(a.qptr[q + 1] - c0);
    const int k = tid % D, grp = tid / D;

    // the chunks in chunk order
    const size_t sz = (size_t)(6 * R * D);
    const float* part = a.scratch + (size_t)q * pp.nch * sz;
    for (int idx = tid; idx < 6 * R * D; idx += NT) {
        const int ls = idx / (R * D), r = (idx / D) % R, c = idx % D;
        float s = part[idx];
        for (int ch = 1; ch < pp.nch; ++ch) s += part[ch * sz + idx];
        A[ls >> 1][ls & 1][r][c] = s;
    }
    __syncthreads();
    // G_r = sum_l A^l_r K^l_r^T, layers ascending, from the transposed K
    for (int r = grp; r < R; r += GR) {
        float Gh = 0.f, Gt = 0.f;
        for (int l = 0; l < 3; ++l) {
            float gh, gt;
            matvec2<D>(a.KT[l] + (size_t)r * D * D + k, A[l][0][r], A[l][1][r], gh, gt);
            Gh += gh;
            Gt += gt;
        }
        G[0][r][k] = Gh;
        G[1][r][k] = Gt;
    }
    __syncthreads();

    // per candidate: attr = val (<GH_rel, E[col]> [role & 1] + <GT_rel, E[col]> [role & 2]), exactly 0 when not eligible
    float tot = 0.f;
    for (int j = tid; j < n; j += NT) {
        float at = 0.f;
        if (a.celig[c0 + j]) {
            const int role = a.crole[c0 + j], rl = a.crel[c0 + j];
            const f32x4* e4 = (const f32x4*)(a.E + (size_t)a.ccol[c0 + j] * D);
            float dot = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (role & (1 << s)) {
                    const f32x4* g4 = (const f32x4*)G[s][rl];
                    f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < D / 4; ++i) {
                        const f32x4 ev = e4[i], gv = g4[i];
#pragma unroll
                        for (int c = 0; c < 4; ++c) c4[c] = fmaf(gv[c], ev[c], c4[c]);
                    }
                    dot += (c4[0] + c4[1]) + (c4[2] + c4[3]);
                }
            at = a.cval[c0 + j] * dot;
        }
        a.attr[c0 + j] = at;
        tot += at;
    }
    red[tid] = tot;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = red[0];
        a.total[q] = total;
        a.gap[q] = total - (a.p_full[q] - a.p_base[q]);
    }
}

}  // namespace xpl

extern "C" {

int iddgcn_explain_seeds_f32(void* stream, int Q, int N, int d, int R, const int* h, const int* r, const int* t,
                             float scale, const float* ES1, const float* P, long long p_layer_stride,
                             long long p_rel_stride, const float* W, const float* Ssm, long long w_layer_stride,
                             const float* X, long long x_layer_stride, const float* K1, const float* K2,
                             const float* K3, const float* S2, const float* S3, const float* Wa2, const float* Wa3,
                             const float* rel, float* G, float* p) {
    using namespace xpl;
    if (d != 32 && d != 64) return IDDGCN_E_BAD_DIM;
    if (R < 1 || R > MAX_R) return IDDGCN_E_BAD_REL;
    if (Q < 0 || N < 1) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    if (!h || !r || !t || !ES1 || !P || !W || !Ssm || !X || !K1 || !K2 || !K3 || !S2 || !S3 || !Wa2 || !Wa3 || !rel ||
        !G || !p)
        return IDDGCN_E_BAD_ARG;
    if (p_layer_stride < 0 || p_rel_stride < 0 || w_layer_stride < 0 || x_layer_stride < 0) return IDDGCN_E_BAD_ARG;
    if (((uintptr_t)ES1 & 15) || ((uintptr_t)P & 15) || ((uintptr_t)G & 15) || (p_layer_stride & 3) ||
        (p_rel_stride & 3))
        return IDDGCN_E_BAD_ARG;
    SeedP a;
    a.Q = Q; a.N = N; a.R = R;
    a.h = h; a.r = r; a.t = t;
    a.scale = scale;
    a.ES1 = ES1; a.P = P; a.pls = p_layer_stride; a.prs = p_rel_stride;
    a.W = W; a.Ssm = Ssm; a.wls = w_layer_stride;
    a.X = X; a.xls = x_layer_stride;
    a.K[0] = K1; a.K[1] = K2; a.K[2] = K3;
    a.S[0] = S2; a.S[1] = S3;
    a.Wa[0] = Wa2; a.Wa[1] = Wa3;
    a.rel = rel; a.G = G; a.p = p;
    const unsigned blocks = (unsigned)((Q + QT - 1) / QT);
    for_small_width(d, [&](auto D) {
        hipLaunchKernelGGL(seeds_kernel<decltype(D)::value>, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, a);
    });
    return (int)hipGetLastError();
}

int iddgcn_explain_row_grads_f32(void* stream, int Q, int N, int d, int R, const int* h, const int* t,
                                 const int* row_ptr, const int* col, const long long* entry_of_csr, const float* G,
                                 const float* E, const long long* qptr, int* entry, float* grad) {
    using namespace xpl;
    if (d != 32 && d != 64) return IDDGCN_E_BAD_DIM;
    if (R < 1 || R > MAX_R) return IDDGCN_E_BAD_REL;
    if (Q < 0 || N < 1) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    if (!h || !t || !row_ptr || !col || !G || !E || !qptr || !entry || !grad) return IDDGCN_E_BAD_ARG;
    if (((uintptr_t)E & 15) || ((uintptr_t)G & 15)) return IDDGCN_E_BAD_ARG;
    RowP a;
    a.N = N; a.R = R;
    a.h = h; a.t = t; a.row_ptr = row_ptr; a.col = col; a.eoc = entry_of_csr;
    a.G = G; a.E = E; a.qptr = qptr; a.entry = entry; a.grad = grad;
    for_small_width(d, [&](auto D) {
        hipLaunchKernelGGL(row_grads_kernel<decltype(D)::value>, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, a);
    });
    return (int)hipGetLastError();
}

int iddgcn_explain_topk_f32(void* stream, int Q, int k, const long long* qptr, const int* entry, const float* grad,
                            int* topk_entry, float* topk_val, int* n_pos) {
    using namespace xpl;
    if (Q < 0 || k < 1 || k > IDDGCN_TOPK_MAX) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    // entry / grad may be null when every segment is empty: they are then never read
    if (!qptr || !topk_entry || !topk_val || !n_pos) return IDDGCN_E_BAD_ARG;
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, k, qptr, entry, grad,
                       topk_entry, topk_val, n_pos);
    return (int)hipGetLastError();
}

int iddgcn_mask_explain_f32(void* stream, const iddgcn_mask_explain_t* args) {
    using namespace xpl;
    if (!args) return IDDGCN_E_BAD_ARG;
    const iddgcn_mask_explain_t& a = *args;
    if (a.d != 32 && a.d != 64) return IDDGCN_E_BAD_DIM;
    if (a.R < 1 || a.R > MAX_R) return IDDGCN_E_BAD_REL;
    if (a.n_queries < 0 || a.N < 1 || a.num_epochs < 0 || a.epochs_base < 0) return IDDGCN_E_BAD_ARG;
    if (a.n_queries == 0) return 0;
    if (!a.qids || !a.h || !a.r || !a.t || !a.qptr || !a.E || !a.rel || !a.init_e || !a.m || !a.v || !a.steps ||
        !a.alpha || !a.out)
        return IDDGCN_E_BAD_ARG;
    // the candidate arrays may be null when every segment is empty: they are then never read
    if (!layers_ok(a.K, a.KT, a.S, a.ST, a.Wa, a.ba)) return IDDGCN_E_BAD_ARG;
    if ((uintptr_t)a.E & 15) return IDDGCN_E_BAD_ARG;
    for_small_width(a.d, [&](auto D) {
        hipLaunchKernelGGL(mask_explain_kernel<decltype(D)::value>, dim3((unsigned)a.n_queries), dim3(NT), 0,
                           (hipStream_t)stream, a);
    });
    return (int)hipGetLastError();
}

int iddgcn_explain_curves_f32(void* stream, const iddgcn_explain_curves_t* args) {
    using namespace xpl;
    if (!args) return IDDGCN_E_BAD_ARG;
    const iddgcn_explain_curves_t& a = *args;
    if (a.d != 32 && a.d != 64) return IDDGCN_E_BAD_DIM;
    if (a.R < 1 || a.R > MAX_R) return IDDGCN_E_BAD_REL;
    if (a.k < 1 || a.k > IDDGCN_TOPK_MAX || a.Q < 0 || a.N < 1) return IDDGCN_E_BAD_ARG;
    if (a.Q == 0) return 0;
    if (!a.h || !a.r || !a.t || !a.qptr || !a.E || !a.rel || !a.del || !a.ins) return IDDGCN_E_BAD_ARG;
    // the candidate arrays may be null when every segment is empty: they are then never read
    if (!layers_ok(a.K, a.S, a.Wa, a.ba)) return IDDGCN_E_BAD_ARG;
    if ((uintptr_t)a.E & 15) return IDDGCN_E_BAD_ARG;
    const int n_tiles = (2 * (a.k + 1) + CV_VT - 1) / CV_VT;
    if ((long long)a.Q * n_tiles > 0x7fffffffLL) return IDDGCN_E_BAD_ARG;
    const dim3 grid((unsigned)(a.Q * n_tiles));
    for_small_width(a.d, [&](auto D) {
        hipLaunchKernelGGL(curves_kernel<decltype(D)::value>, grid, dim3(NT), 0, (hipStream_t)stream, a, n_tiles);
    });
    return (int)hipGetLastError();
}

int iddgcn_explain_counterfactual_f32(void* stream, const iddgcn_counterfactual_t* args) {
    using namespace xpl;
    if (!args) return IDDGCN_E_BAD_ARG;
    const iddgcn_counterfactual_t& a = *args;
    if (a.d != 32 && a.d != 64) return IDDGCN_E_BAD_DIM;
    if (a.R < 1 || a.R > MAX_R) return IDDGCN_E_BAD_REL;
    if (a.k < 0 || a.k > IDDGCN_TOPK_MAX || a.Q < 0 || a.N < 1 || a.max_cand < 0) return IDDGCN_E_BAD_ARG;
    if (a.mode != IDDGCN_CF_FLIP && a.mode != IDDGCN_CF_LOWER && a.mode != IDDGCN_CF_RAISE) return IDDGCN_E_BAD_ARG;
    if (a.Q == 0) return 0;
    if (!a.h || !a.r || !a.t || !a.qptr || !a.E || !a.rel || !a.path || !a.n_steps || !a.flipped ||
        (a.k > 0 && !a.chosen) || (a.k > 1 && a.loo && !a.scratch))
        return IDDGCN_E_BAD_ARG;
    // the per-candidate arrays may be null when every segment is empty: they are then never touched
    if (!layers_ok(a.K, a.S, a.Wa, a.ba)) return IDDGCN_E_BAD_ARG;
    if ((uintptr_t)a.E & 15) return IDDGCN_E_BAD_ARG;
    long long tiles = ((long long)a.max_cand + 1 + CV_VT - 1) / CV_VT;
    tiles = tiles > 1024 ? 1024 : tiles;
    if ((long long)a.Q * tiles > 0x7fffffffLL) return IDDGCN_E_BAD_ARG;
    const dim3 grid((unsigned)(a.Q * tiles));
    const hipStream_t st = (hipStream_t)stream;
    const int steps = a.k > 0 ? a.k : 1;
    for (int i = 0; i < steps; ++i) {
        float* vals = i == 0 ? a.loo : a.scratch;
        for_small_width(a.d, [&](auto D) {
            hipLaunchKernelGGL(cf_step_kernel<decltype(D)::value>, grid, dim3(NT), 0, st, a, i, (int)tiles, vals);
        });
        hipLaunchKernelGGL(cf_select_kernel, dim3((unsigned)a.Q), dim3(NT), 0, st, a, i, a.k > 0 ? 1 : 0, vals);
    }
    return (int)hipGetLastError();
}

long long iddgcn_explain_path_scratch_floats(int Q, int m, int d, int R) {
    using namespace xpl;
    if ((d != 32 && d != 64) || R < 1 || R > MAX_R || Q < 0 || m < 1 || m > IDDGCN_PATH_MAX_STEPS) return 0;
    return (long long)Q * ((m + IG_CHUNK - 1) / IG_CHUNK) * 6 * R * d;
}

int iddgcn_explain_path_f32(void* stream, const iddgcn_explain_path_t* args) {
    using namespace xpl;
    if (!args) return IDDGCN_E_BAD_ARG;
    const iddgcn_explain_path_t& a = *args;
    if (a.d != 32 && a.d != 64) return IDDGCN_E_BAD_DIM;
    if (a.R < 1 || a.R > MAX_R) return IDDGCN_E_BAD_REL;
    if (a.m < 1 || a.m > IDDGCN_PATH_MAX_STEPS || a.Q < 0 || a.N < 1) return IDDGCN_E_BAD_ARG;
    if (a.Q == 0) return 0;
    if (!a.h || !a.r || !a.t || !a.qptr || !a.E || !a.rel || !a.alpha || !a.omega || !a.total || !a.p_full ||
        !a.p_base || !a.gap || !a.scratch)
        return IDDGCN_E_BAD_ARG;
    // the per-candidate arrays may be null when every segment is empty: they are then never touched
    if (!layers_ok(a.K, a.KT, a.S, a.ST, a.Wa, a.ba)) return IDDGCN_E_BAD_ARG;
    if ((uintptr_t)a.E & 15) return IDDGCN_E_BAD_ARG;
    PathP pp;
    pp.a = a;
    pp.nch = (a.m + IG_CHUNK - 1) / IG_CHUNK;
    if ((long long)a.Q * pp.nch > 0x7fffffffLL) return IDDGCN_E_BAD_ARG;
    const hipStream_t st = (hipStream_t)stream;
    for_small_width(a.d, [&](auto D) {
        hipLaunchKernelGGL(ig_path_kernel<decltype(D)::value>, dim3((unsigned)(a.Q * pp.nch)), dim3(NT), 0, st, pp);
        hipLaunchKernelGGL(ig_finish_kernel<decltype(D)::value>, dim3((unsigned)a.Q), dim3(NT), 0, st, pp);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
