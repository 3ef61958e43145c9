// screen.hip — all-candidate link ranking for gfx950 (include/iddgcn_screen.h).
//
// screen_chain_kernel: the tail chain of Q x N dense (query, candidate) pairs and their DistMult logit in one
// kernel.  The candidates of a block are consecutive entity ids, so no index array is read; one side of every pair
// is the query's node, so either the gathered rows (head side) or the coefficients (tail side) are the same for
// the whole block.  S^2 and S^3 stay in VGPRs in rowgemm_kernel's fragment layout (iddgcn_hip.hip), the
// activations x^1, x^2 live in two LDS tiles, x^3 never leaves the accumulator registers: one float per
// candidate goes to global memory.
//
// rank_topk_kernel: rank counts against a target and the k best candidates of every row of s, one workgroup per
// query, the row walked in passes of 960 candidates that are merged into the running top 64 by a bitonic sort of
// 64-bit (value, id) keys in LDS.  A pass with no candidate above the current k-th key skips its sort.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "iddgcn.h"
#include "iddgcn_screen.h"
#include "per_query.hpp"

namespace scr {

using namespace pq;      // f32x4, sigmoid_fast, ld4 / st4, make_key, TK_BUF / TK_CH

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAX_R = 8;
constexpr int NT = 256;            // 4 waves

// wave w: column slab cs = w % CS (32 output columns), row group rg = w / CS (32 rows), as rowgemm_kernel
template <int D>
struct SC {
    static constexpr int CS = D / 32;
    static constexpr int NW = NT / 64;
    static constexpr int RGS = NW / CS;
    static constexpr int TR = RGS * 32;        // rows (candidates) per tile: 64 at D = 64, 128 at D = 32
    static constexpr int LDA = D + 4;          // padded LDS rows: conflict-free ds_read_b128 fragment reads
};

struct ScreenP {
    int N, R, side;
    const int* q_node; const int* q_rel;
    const float* ES1; const float* P; long long pls, prs;
    const float* W; long long wls;
    const float* X3; const float* S2; const float* S3; const float* rel;
    float* s;
    int ntiles, tpb, groups;       // row tiles per query, tiles per block, blocks per query
};

// x (32 rows of the LDS tile) · B slab, k-step q (8 k-values) into chain q % 4, (c0 + c1) + (c2 + c3): the
// engine's four-chain form of v_mfma_f32_32x32x2_f32 (IDDGCN_GEMM_F32_4CHAIN)
template <int D>
__device__ __forceinline__ f32x16 tile_mm(const float* arow, const float (&b)[D / 2]) {
    f32x16 a0, a1, a2, a3;
#pragma unroll
    for (int j = 0; j < 16; ++j) a0[j] = a1[j] = a2[j] = a3[j] = 0.f;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
        const f32x4 a4 = ld4(arow + 8 * q);
        f32x16& ac = (q & 3) == 0 ? a0 : (q & 3) == 1 ? a1 : (q & 3) == 2 ? a2 : a3;
        ac = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[0], b[4 * q + 0], ac, 0, 0, 0);
        ac = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[1], b[4 * q + 1], ac, 0, 0, 0);
        ac = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[2], b[4 * q + 2], ac, 0, 0, 0);
        ac = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[3], b[4 * q + 3], ac, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) a0[j] = (a0[j] + a1[j]) + (a2[j] + a3[j]);
    return a0;
}

// acc + sum_r W^l[head][r] P^l_r[tail][c], r ascending (every operand loaded before the first fma)
__device__ __forceinline__ float add_relations(float v, const float* __restrict__ w, const float* __restrict__ pc,
                                               long long prs, int R) {
    float cf[MAX_R], pv[MAX_R];
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) {
        cf[r] = r < R ? w[r] : 0.f;
        pv[r] = r < R ? pc[r * prs] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < MAX_R; ++r)
        if (r < R) v = fmaf(cf[r], pv[r], v);
    return v;
}

template <int D>
__global__ __launch_bounds__(NT, 2) void screen_chain_kernel(const ScreenP p) {
    using C = SC<D>;
    __shared__ __attribute__((aligned(16))) float A0[C::TR * C::LDA];     // x^1
    __shared__ __attribute__((aligned(16))) float A1[C::TR * C::LDA];     // x^2
    __shared__ float red[C::CS * C::TR];                                  // DistMult partials per column slab
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cs = wave % C::CS, rg = wave / C::CS;
    const int i = lane & 31, h = lane >> 5;
    const int c = cs * 32 + i;

    // B slabs of S^2, S^3: b[s] = S[kk(s, h)][c], kk(s, h) = 8(s / 4) + 4h + s % 4
    float b2[D / 2], b3[D / 2];
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        const int kk = 8 * (s >> 2) + 4 * h + (s & 3);
        b2[s] = p.S2[kk * D + c];
        b3[s] = p.S3[kk * D + c];
    }

    const int q = blockIdx.x / p.groups, g = blockIdx.x % p.groups;
    const int qn = p.q_node[q], qr = p.q_rel[q];
    const int R = p.R, N = p.N;
    const bool head_side = p.side == IDDGCN_SCREEN_HEAD;
    const float relc = p.rel[(size_t)qr * D + c];
    const float* W1 = p.W;
    const float* W2 = p.W + p.wls;
    const float* W3 = p.W + 2 * p.wls;
    const float* P1 = p.P;
    const float* P2 = p.P + p.pls;
    const float* P3 = p.P + 2 * p.pls;
    float* srow = p.s + (size_t)q * N;

    const int t_beg = g * p.tpb;
    const int t_end = t_beg + p.tpb < p.ntiles ? t_beg + p.tpb : p.ntiles;
    for (int tile = t_beg; tile < t_end; ++tile) {
        const int row0 = tile * C::TR;
        // x^1 = sigmoid(ES1[tail] + sum_r W^1[head][r] P^1_r[tail]) into A0 (rows past N: zeros)
        constexpr int F4R = D / 4;
#pragma unroll
        for (int it = 0; it < C::TR * F4R / NT; ++it) {
            const int idx = it * NT + threadIdx.x;
            const int r = idx / F4R, c4 = (idx % F4R) * 4;
            const int e = row0 + r;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < N) {
                const size_t hd = head_side ? e : qn, tl = head_side ? qn : e;
                v = ld4(p.ES1 + tl * D + c4);
                const float* w = W1 + hd * R;
                const float* pc = P1 + tl * D + c4;
                float cf[MAX_R];
                f32x4 pv[MAX_R];
#pragma unroll
                for (int k = 0; k < MAX_R; ++k) {
                    cf[k] = k < R ? w[k] : 0.f;
                    pv[k] = k < R ? ld4(pc + k * p.prs) : v;
                }
#pragma unroll
                for (int k = 0; k < MAX_R; ++k)
                    if (k < R) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = fmaf(cf[k], pv[k][j], v[j]);
                    }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = sigmoid_fast(v[j]);
            }
            st4(A0 + r * C::LDA + c4, v);
        }
        __syncthreads();

        // layer 2: x^2 = sigmoid(x^1 S^2 + sum_r W^2[head][r] P^2_r[tail]) into A1
        f32x16 acc = tile_mm<D>(A0 + (rg * 32 + i) * C::LDA + 4 * h, b2);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = rg * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int e = row0 + row;
            float v = 0.f;
            if (e < N) {
                const size_t hd = head_side ? e : qn, tl = head_side ? qn : e;
                v = sigmoid_fast(add_relations(acc[reg], W2 + hd * R, P2 + tl * D + c, p.prs, R));
            }
            A1[row * C::LDA + c] = v;
        }
        __syncthreads();

        // layer 3 and DistMult: x^3 stays in registers; the row's dot over this wave's 32 columns is a butterfly
        // over the 32 lanes of a half-wave, the column slabs are added in slab order below
        acc = tile_mm<D>(A1 + (rg * 32 + i) * C::LDA + 4 * h, b3);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = rg * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int e = row0 + row;
            float part = 0.f;
            if (e < N) {
                const size_t hd = head_side ? e : qn, tl = head_side ? qn : e;
                const float x3 = sigmoid_fast(add_relations(acc[reg], W3 + hd * R, P3 + tl * D + c, p.prs, R));
                part = (p.X3[hd * D + c] * relc) * x3;
            }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (i == 0) red[cs * C::TR + row] = part;
        }
        __syncthreads();
        if (threadIdx.x < C::TR && row0 + (int)threadIdx.x < N) {
            float v = red[threadIdx.x];
#pragma unroll
            for (int k = 1; k < C::CS; ++k) v += red[k * C::TR + threadIdx.x];
            srow[row0 + threadIdx.x] = v;
        }
        // the next tile's writes of A0 / A1 / red come after barriers every reader above has passed
    }
}

// ---- selection -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_sorted(const int* __restrict__ f, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (f[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < n && f[lo] == c;
}

__global__ __launch_bounds__(NT) void rank_topk_kernel(int N, int k, const float* __restrict__ s,
                                                       const int* __restrict__ target, const int* __restrict__ fptr,
                                                       const int* __restrict__ fidx, int* __restrict__ greater,
                                                       int* __restrict__ equal, int* __restrict__ topk_idx,
                                                       float* __restrict__ topk_val) {
    __shared__ unsigned long long buf[TK_BUF];
    __shared__ int cnt[2][NT / 64];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const float* row = s + (size_t)q * N;
    const int tg = target[q];
    const bool has_t = tg >= 0 && tg < N;
    const float st = has_t ? row[tg] : 0.f;
    const int f0 = fptr ? fptr[q] : 0;
    const int nf = fptr ? fptr[q + 1] - f0 : 0;
    const int* fl = fidx + f0;

    for (int j = tid; j < TK_BUF; j += NT) buf[j] = 0ull;
    __syncthreads();
    unsigned long long thr = 0ull;       // the current k-th key
    int g = 0, eq = 0;
    for (long long base = 0; base < N; base += TK_CH) {
        unsigned long long keys[TK_BUF / NT];
        int any = 0;
#pragma unroll
        for (int u = 0; u < TK_BUF / NT; ++u) {
            const int j = tid + u * NT;
            unsigned long long key = 0ull;
            if (j < TK_CH && base + j < N) {
                const int c = (int)(base + j);
                const float v = row[c];
                const bool is_t = c == tg;
                if (is_t || nf == 0 || !in_sorted(fl, nf, c)) {
                    key = make_key(v, c);
                    if (has_t && !is_t) {
                        g += v > st;
                        eq += v == st;
                    }
                }
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
                        const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                        const int b = a | j;
                        const unsigned long long x = buf[a], y = buf[b];
                        const bool desc = (a & k2) == 0;
                        if ((x < y) == desc) {
                            buf[a] = y;
                            buf[b] = x;
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
    if (tid < k) {
        const unsigned long long key = buf[TK_CH + tid];
        const int c = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
        topk_idx[(size_t)q * k + tid] = c;
        topk_val[(size_t)q * k + tid] = c >= 0 ? row[c] : -INFINITY;
    }
    // rank counts: integer sums (any order gives the same result)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        g += __shfl_xor(g, o, 64);
        eq += __shfl_xor(eq, o, 64);
    }
    if ((tid & 63) == 0) {
        cnt[0][tid >> 6] = g;
        cnt[1][tid >> 6] = eq;
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < NT / 64; ++w) {
            a += cnt[0][w];
            b += cnt[1][w];
        }
        greater[q] = a;
        equal[q] = b;
    }
}

}  // namespace scr

extern "C" {

int iddgcn_screen_chain_f32(void* stream, int Q, int N, int d, int R, int side, const int* q_node, const int* q_rel,
                            const float* ES1, const float* P, long long p_layer_stride, long long p_rel_stride,
                            const float* W, long long w_layer_stride, const float* X3, const float* S2,
                            const float* S3, const float* rel, float* s) {
    using namespace scr;
    if (d != 32 && d != 64) return IDDGCN_E_BAD_DIM;
    if (R < 1 || R > MAX_R) return IDDGCN_E_BAD_REL;
    if (Q < 0 || N < 1 || (side != IDDGCN_SCREEN_TAIL && side != IDDGCN_SCREEN_HEAD)) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    if (!q_node || !q_rel || !ES1 || !P || !W || !X3 || !S2 || !S3 || !rel || !s) return IDDGCN_E_BAD_ARG;
    if (p_layer_stride < 0 || p_rel_stride < 0 || w_layer_stride < 0) return IDDGCN_E_BAD_ARG;
    // rows of ES1 and P are read as 16-byte vectors
    if (((uintptr_t)ES1 & 15) || ((uintptr_t)P & 15) || (p_layer_stride & 3) || (p_rel_stride & 3))
        return IDDGCN_E_BAD_ARG;
    int TR = 0;
    for_small_width(d, [&](auto D) { TR = SC<decltype(D)::value>::TR; });
    ScreenP p;
    p.N = N; p.R = R; p.side = side;
    p.q_node = q_node; p.q_rel = q_rel;
    p.ES1 = ES1; p.P = P; p.pls = p_layer_stride; p.prs = p_rel_stride;
    p.W = W; p.wls = w_layer_stride;
    p.X3 = X3; p.S2 = S2; p.S3 = S3; p.rel = rel; p.s = s;
    p.ntiles = (int)(((long long)N + TR - 1) / TR);
    // consecutive tiles of one query per block, so that the register-resident S^2 / S^3 are loaded once for
    // several tiles while the grid keeps about 2048 blocks (8 per CU)
    const long long total = (long long)Q * p.ntiles;
    long long tpb = total / 2048;
    if (tpb < 1) tpb = 1;
    if (tpb > p.ntiles) tpb = p.ntiles;
    p.tpb = (int)tpb;
    p.groups = (p.ntiles + p.tpb - 1) / p.tpb;
    const long long blocks = (long long)Q * p.groups;
    if (blocks >= (1ll << 31)) return IDDGCN_E_BAD_ARG;
    for_small_width(d, [&](auto D) {
        hipLaunchKernelGGL(screen_chain_kernel<decltype(D)::value>, dim3((unsigned)blocks), dim3(NT), 0,
                           (hipStream_t)stream, p);
    });
    return (int)hipGetLastError();
}

int iddgcn_rank_topk_f32(void* stream, int Q, int N, int k, const float* s, const int* target, const int* fptr,
                         const int* fidx, int* greater, int* equal, int* topk_idx, float* topk_val) {
    using namespace scr;
    if (Q < 0 || N < 1 || k < 1 || k > IDDGCN_TOPK_MAX) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    if (!s || !target || !greater || !equal || !topk_idx || !topk_val) return IDDGCN_E_BAD_ARG;
    if ((fptr == nullptr) != (fidx == nullptr)) return IDDGCN_E_BAD_ARG;
    hipLaunchKernelGGL(rank_topk_kernel, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, N, k, s, target, fptr,
                       fidx, greater, equal, topk_idx, topk_val);
    return (int)hipGetLastError();
}

}  // extern "C"
