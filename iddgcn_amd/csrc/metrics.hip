// metrics.hip — binary-classification metrics on the device for gfx950 (include/iddgcn_metrics.h; semantics there).
//
// One 64-bit key per element: bits [2, 34) the inverted float32 bit pattern of the probability (-0.0 as +0.0), so an
// ascending sort walks the scores downwards; bit 1 a label outside {0, 1}; bit 0 set for a negative; bits [34, ..)
// the slot (general path only).  Two elements tie iff key >> 2 is equal.  After the sort a scan gives every element
//   cum[i] : positives among the sorted elements up to and including i (from the scan's origin);
//   gst[i] : index of the first element of i's tie group (a max-scan of the group starts' own indices),
// and the LAST element of every tie group, which sees the inclusive counts of its group in cum[i] and the counts
// strictly above the group in cum[gst[i]], adds the group's ROC-AUC term (integer) and AUPR term (fp64).  Nothing is
// compacted, so a tie group or a slot that crosses a workgroup boundary needs no special case: both ends are indices.
//
//   small path  (n <= IDDGCN_CLF_SMALL_MAX): one launch, workgroup s keeps the elements of slot s (the others become a
//                sentinel key that sorts last), bitonic-sorts the keys in LDS, scans them (wave shuffles + an LDS carry
//                across waves) and reduces the terms.
//   general path: keys kernel, iddgcn_radix_sort_pairs once on the score bits (slot 0) and once on (slot, score)
//                (slots 1..G; outside [0, G) -> slot G + 1, never read), both into one array of m = n or 2n keys; tile
//                aggregates / scan of the aggregates by one workgroup / apply; the terms of (tile c of slot s) by
//                workgroup (c, s); workgroup s adds the tiles' partials in index order.
// fp64 sums: each thread adds its consecutive elements in order, a wave adds by a fixed shuffle tree, wave totals are
// added in wave order by one thread; tile partials in index order.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iddgcn.h"
#include "iddgcn_graph.h"
#include "iddgcn_metrics.h"

namespace mt {

constexpr int SMALL_NT = 1024;                              // threads of a small-path workgroup
constexpr int SMALL_IPT = IDDGCN_CLF_SMALL_MAX / SMALL_NT;  // consecutive sorted elements per thread
constexpr int NT = 256;                                     // general path: threads per tile
constexpr int IPT = 4;
constexpr int TILE = NT * IPT;
constexpr int SCORE_SHIFT = 2, SLOT_SHIFT = 34;
constexpr uint64_t SENTINEL = ~0ull;
constexpr double EPS = 1e-7;                                // Keras backend epsilon

static_assert(IDDGCN_CLF_SMALL_MAX == 4096 && SMALL_IPT == 4, "small path: 4096 keys, 4 per thread");

#define MT_CHECK(x)                              \
    do {                                         \
        const hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return (int)e_;    \
    } while (0)

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline int bit_length(uint64_t x) {
    int b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

// ---- keys ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t make_key(float p, float y) {
    unsigned b = __float_as_uint(p);
    if (b == 0x80000000u) b = 0u;
    const unsigned bad_label = !(y == 0.0f || y == 1.0f);
    return ((uint64_t)(~b) << SCORE_SHIFT) | (uint64_t)(bad_label << 1) | (uint64_t)(y == 1.0f ? 0u : 1u);
}
__device__ __forceinline__ float key_prob(uint64_t k) { return __uint_as_float(~(unsigned)(k >> SCORE_SHIFT)); }
__device__ __forceinline__ unsigned key_pos(uint64_t k) { return (unsigned)(~k & 1ull); }
__device__ __forceinline__ uint64_t key_tie(uint64_t k) { return k >> SCORE_SHIFT; }

// ---- per-slot accumulators ----------------------------------------------------------------------
struct Acc {
    uint64_t tp, fp, P, auc, nthr, bad;
    double aupr, bce;
};
constexpr int ACC_U64 = 6, ACC_F64 = 2;

__device__ __forceinline__ Acc acc_zero() { return Acc{0, 0, 0, 0, 0, 0, 0.0, 0.0}; }

// Element i of the slot whose sorted keys are K[b0, e0); base = positives before b0 in cum's count.
template <typename CumT, typename IdxT>
__device__ __forceinline__ void elem_terms(Acc& a, const uint64_t* K, const CumT* cum, const IdxT* gst, long long i,
                                           long long b0, long long e0, uint64_t base, double thr) {
    const uint64_t k = K[i];
    const unsigned pos = key_pos(k);
    const float p = key_prob(k);
    const bool pred = (double)p > thr;
    a.P += pos;
    a.tp += (pred && pos) ? 1u : 0u;
    a.fp += (pred && !pos) ? 1u : 0u;
    a.bad |= ((k >> 1) & 1ull) | (uint64_t)(!(p >= 0.0f && p <= 1.0f));
    double q = (double)p;
    q = q < EPS ? EPS : (q > 1.0 - EPS ? 1.0 - EPS : q);
    a.bce -= log(pos ? q + EPS : (1.0 - q) + EPS);
    if (i + 1 == e0 || key_tie(K[i + 1]) != key_tie(k)) {       // last element of its tie group
        const long long js = (long long)gst[i];
        const uint64_t TPi = (uint64_t)cum[i] - base, FPi = (uint64_t)(i - b0 + 1) - TPi;
        const uint64_t TPb = (uint64_t)cum[js] - key_pos(K[js]) - base, FPb = (uint64_t)(js - b0) - TPb;
        const uint64_t tpg = TPi - TPb, fpg = FPi - FPb;
        a.auc += fpg * (2 * TPb + tpg);
        a.nthr += 1;
        const double prec = (double)TPi / (double)(TPi + FPi);
        const double prev = js == b0 ? 1.0 : (double)TPb / (double)(TPb + FPb);
        a.aupr += (double)tpg * (prec + prev) * 0.5;
    }
}

// Sum over the workgroup in a fixed order; the result is valid in thread 0.  scratch: one T per wave.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                       // scratch may still be read from the previous call
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    T r = scratch[0];
    if (threadIdx.x == 0)
        for (unsigned w = 1; w < nw; ++w) r += scratch[w];
    return r;
}

__device__ __forceinline__ Acc block_sum_acc(const Acc& a, uint64_t* su, double* sd) {
    Acc r;
    r.tp = block_sum(a.tp, su);
    r.fp = block_sum(a.fp, su);
    r.P = block_sum(a.P, su);
    r.auc = block_sum(a.auc, su);
    r.nthr = block_sum(a.nthr, su);
    r.bad = block_sum(a.bad, su);
    r.aupr = block_sum(a.aupr, sd);
    r.bce = block_sum(a.bce, sd);
    return r;
}

// Exclusive scan over the workgroup's threads of (sum, max) pairs, identity (0, 0); tot_*: the workgroup's totals.
// scratch: 2 unsigned per wave.
__device__ __forceinline__ void block_excl_scan_pair(unsigned& s, unsigned& m, unsigned& tot_s, unsigned& tot_m,
                                                     unsigned* scratch) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    unsigned is = s, im = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned ys = __shfl_up(is, o, 64), ym = __shfl_up(im, o, 64);
        if (lane >= (unsigned)o) {
            is += ys;
            im = im > ym ? im : ym;
        }
    }
    unsigned es = __shfl_up(is, 1, 64), em = __shfl_up(im, 1, 64);
    if (lane == 0) es = 0u, em = 0u;
    __syncthreads();                       // scratch may still be read from the previous call
    if (lane == 63) scratch[2 * wave] = is, scratch[2 * wave + 1] = im;
    __syncthreads();
    unsigned ps = 0u, pm = 0u, ts = 0u, tm = 0u;
    for (unsigned w = 0; w < nw; ++w) {
        const unsigned ws = scratch[2 * w], wm = scratch[2 * w + 1];
        if (w < wave) {
            ps += ws;
            pm = pm > wm ? pm : wm;
        }
        ts += ws;
        tm = tm > wm ? tm : wm;
    }
    s = ps + es;
    m = pm > em ? pm : em;
    tot_s = ts;
    tot_m = tm;
}

__device__ __forceinline__ void finalize(const Acc& a, uint64_t cnt, long long* __restrict__ counts,
                                         double* __restrict__ values) {
    const uint64_t P = a.P, N = cnt - P, tp = a.tp, fp = a.fp, fn = P - tp, tn = N - fp;
    counts[IDDGCN_CLF_TP] = (long long)tp;
    counts[IDDGCN_CLF_TN] = (long long)tn;
    counts[IDDGCN_CLF_FP] = (long long)fp;
    counts[IDDGCN_CLF_FN] = (long long)fn;
    counts[IDDGCN_CLF_P] = (long long)P;
    counts[IDDGCN_CLF_N_NEG] = (long long)N;
    counts[IDDGCN_CLF_AUC_NUM2] = (long long)a.auc;
    counts[IDDGCN_CLF_N_THRESHOLDS] = (long long)a.nthr;
    counts[IDDGCN_CLF_STATUS] = (P == 0 ? IDDGCN_CLF_ST_NO_POS : 0) | (N == 0 ? IDDGCN_CLF_ST_NO_NEG : 0) |
                                (a.bad ? IDDGCN_CLF_ST_BAD_INPUT : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double rec = P ? (double)tp / (double)P : nan;
    const double prec = (tp + fp) ? (double)tp / (double)(tp + fp) : nan;
    values[IDDGCN_CLF_V_ACCURACY] = cnt ? (double)(tp + tn) / (double)cnt : nan;
    values[IDDGCN_CLF_V_RECALL] = rec;
    values[IDDGCN_CLF_V_PRECISION] = prec;
    values[IDDGCN_CLF_V_SPECIFICITY] = N ? (double)tn / (double)N : nan;
    values[IDDGCN_CLF_V_F1] = (prec + rec) != 0.0 ? 2.0 * prec * rec / (prec + rec) : nan;
    values[IDDGCN_CLF_V_ROC_AUC] = (P && N) ? (double)a.auc / (double)(2 * P * N) : nan;
    values[IDDGCN_CLF_V_AUPR] = P ? a.aupr / (double)P : nan;
    values[IDDGCN_CLF_V_BCE] = cnt ? a.bce / (double)cnt : nan;
}

// ---- small path ---------------------------------------------------------------------------------
__global__ __launch_bounds__(SMALL_NT) void clf_small_kernel(int n, const float* __restrict__ prob,
                                                             const float* __restrict__ label,
                                                             const int* __restrict__ group, double thr,
                                                             long long* __restrict__ counts,
                                                             double* __restrict__ values) {
    __shared__ uint64_t K[IDDGCN_CLF_SMALL_MAX];
    __shared__ unsigned cum[IDDGCN_CLF_SMALL_MAX];
    __shared__ unsigned short gst[IDDGCN_CLF_SMALL_MAX];
    __shared__ uint64_t su[SMALL_NT / 64];
    __shared__ double sd[SMALL_NT / 64];
    __shared__ unsigned sp[2 * SMALL_NT / 64];
    __shared__ unsigned s_cnt;
    const int tid = threadIdx.x, slot = blockIdx.x;
    int npad = 2;
    while (npad < n) npad <<= 1;                                   // n <= 4096: npad <= 4096

    uint64_t mine = 0;
    for (int i = tid; i < npad; i += SMALL_NT) {
        uint64_t k = SENTINEL;
        if (i < n && (slot == 0 || group[i] == slot - 1)) {
            k = make_key(prob[i], label[i]);
            ++mine;
        }
        K[i] = k;
    }
    mine = block_sum(mine, su);
    if (tid == 0) s_cnt = (unsigned)mine;
    __syncthreads();
    const int cnt = (int)s_cnt;

    // bitonic sort, ascending: the slot's keys (< 2^34) first, the sentinels after them
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npad >> 1); t += SMALL_NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = K[i], b = K[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    K[i] = b;
                    K[l] = a;
                }
            }
            __syncthreads();
        }
    }

    // scan: thread tid owns the sorted positions [SMALL_IPT * tid, SMALL_IPT * tid + SMALL_IPT)
    const int i0 = SMALL_IPT * tid;
    unsigned lsum = 0u, lmax = 0u;
    for (int e = 0; e < SMALL_IPT; ++e) {
        const int i = i0 + e;
        if (i < cnt) {
            lsum += key_pos(K[i]);
            if (i > 0 && key_tie(K[i - 1]) != key_tie(K[i])) lmax = (unsigned)i;
        }
    }
    unsigned es = lsum, em = lmax, ts, tm;
    block_excl_scan_pair(es, em, ts, tm, sp);
    for (int e = 0; e < SMALL_IPT; ++e) {
        const int i = i0 + e;
        if (i < cnt) {
            es += key_pos(K[i]);
            if (i > 0 && key_tie(K[i - 1]) != key_tie(K[i])) em = (unsigned)i;
            cum[i] = es;
            gst[i] = (unsigned short)em;
        }
    }
    __syncthreads();

    Acc a = acc_zero();
    for (int e = 0; e < SMALL_IPT; ++e) {
        const int i = i0 + e;
        if (i < cnt) elem_terms(a, K, cum, gst, i, 0, cnt, 0ull, thr);
    }
    const Acc r = block_sum_acc(a, su, sd);
    if (tid == 0)
        finalize(r, (uint64_t)cnt, counts + (size_t)slot * IDDGCN_CLF_N_COUNTS,
                 values + (size_t)slot * IDDGCN_CLF_N_VALUES);
}

// ---- general path -------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void clf_keys_kernel(long long n, int G, const float* __restrict__ prob,
                                                      const float* __restrict__ label,
                                                      const int* __restrict__ group, uint64_t* __restrict__ k0,
                                                      uint64_t* __restrict__ k1) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = make_key(prob[i], label[i]);
    k0[i] = k;
    if (G > 0) {
        const int g = group[i];
        const uint64_t slot = (g >= 0 && g < G) ? (uint64_t)g + 1 : (uint64_t)G + 1;
        k1[i] = k | (slot << SLOT_SHIFT);
    }
}

// Tile aggregates (positives, last tie-group start) of the m sorted keys, and the slots' [first, end) bounds.
__global__ __launch_bounds__(NT) void clf_tile_kernel(const uint64_t* __restrict__ K, long long m,
                                                      unsigned* __restrict__ tsum, unsigned* __restrict__ tmax,
                                                      unsigned* __restrict__ bounds) {
    __shared__ unsigned sp[2 * NT / 64];
    const long long i0 = (long long)blockIdx.x * TILE + (long long)threadIdx.x * IPT;
    unsigned lsum = 0u, lmax = 0u;
    for (int e = 0; e < IPT; ++e) {
        const long long i = i0 + e;
        if (i < m) {
            const uint64_t k = K[i];
            lsum += key_pos(k);
            if (i > 0) {
                const uint64_t kp = K[i - 1];
                if (key_tie(kp) != key_tie(k)) lmax = (unsigned)i;
                if ((kp >> SLOT_SHIFT) != (k >> SLOT_SHIFT)) {
                    bounds[2 * (k >> SLOT_SHIFT)] = (unsigned)i;
                    bounds[2 * (kp >> SLOT_SHIFT) + 1] = (unsigned)i;
                }
            } else {
                bounds[2 * (k >> SLOT_SHIFT)] = 0u;
            }
            if (i == m - 1) bounds[2 * (k >> SLOT_SHIFT) + 1] = (unsigned)m;
        }
    }
    unsigned es = lsum, em = lmax, ts, tm;
    block_excl_scan_pair(es, em, ts, tm, sp);
    if (threadIdx.x == 0) {
        tsum[blockIdx.x] = ts;
        tmax[blockIdx.x] = tm;
    }
}

// Exclusive (sum, max) scan of the nt tile aggregates in place, by one workgroup.
__global__ __launch_bounds__(1024) void clf_scan_tiles_kernel(unsigned* __restrict__ tsum,
                                                              unsigned* __restrict__ tmax, long long nt) {
    __shared__ unsigned sp[2 * 1024 / 64];
    unsigned cs = 0u, cm = 0u;
    for (long long base = 0; base < nt; base += 1024) {
        const long long i = base + threadIdx.x;
        unsigned s = i < nt ? tsum[i] : 0u, mx = i < nt ? tmax[i] : 0u, ts, tm;
        block_excl_scan_pair(s, mx, ts, tm, sp);
        if (i < nt) {
            tsum[i] = cs + s;
            tmax[i] = cm > mx ? cm : mx;
        }
        cs += ts;
        cm = cm > tm ? cm : tm;
    }
}

__global__ __launch_bounds__(NT) void clf_apply_kernel(const uint64_t* __restrict__ K, long long m,
                                                       const unsigned* __restrict__ tsum,
                                                       const unsigned* __restrict__ tmax,
                                                       unsigned* __restrict__ cum, unsigned* __restrict__ gst) {
    __shared__ unsigned sp[2 * NT / 64];
    const long long i0 = (long long)blockIdx.x * TILE + (long long)threadIdx.x * IPT;
    unsigned lsum = 0u, lmax = 0u;
    unsigned pos[IPT], st[IPT];
    for (int e = 0; e < IPT; ++e) {
        const long long i = i0 + e;
        pos[e] = 0u;
        st[e] = 0u;
        if (i < m) {
            const uint64_t k = K[i];
            pos[e] = key_pos(k);
            if (i > 0 && key_tie(K[i - 1]) != key_tie(k)) st[e] = (unsigned)i;
            lsum += pos[e];
            lmax = st[e] ? st[e] : lmax;
        }
    }
    unsigned es = lsum, em = lmax, ts, tm;
    block_excl_scan_pair(es, em, ts, tm, sp);
    es += tsum[blockIdx.x];
    const unsigned bm = tmax[blockIdx.x];
    em = em > bm ? em : bm;
    for (int e = 0; e < IPT; ++e) {
        const long long i = i0 + e;
        if (i < m) {
            es += pos[e];
            em = st[e] ? st[e] : em;
            cum[i] = es;
            gst[i] = em;
        }
    }
}

// Workgroup (c, s): the terms of the c-th tile of slot s, its partial sums to part_*[s * chunks + c].
__global__ __launch_bounds__(NT) void clf_terms_kernel(const uint64_t* __restrict__ K,
                                                       const unsigned* __restrict__ cum,
                                                       const unsigned* __restrict__ gst,
                                                       const unsigned* __restrict__ bounds, double thr,
                                                       uint64_t* __restrict__ part_u, double* __restrict__ part_d) {
    __shared__ uint64_t su[NT / 64];
    __shared__ double sd[NT / 64];
    const unsigned s = blockIdx.y, c = blockIdx.x, chunks = gridDim.x;
    const long long b0 = bounds[2 * s], e0 = bounds[2 * s + 1];
    const long long i0 = b0 + (long long)c * TILE + (long long)threadIdx.x * IPT;
    Acc a = acc_zero();
    if (b0 + (long long)c * TILE < e0) {                          // uniform over the workgroup
        const uint64_t base = (uint64_t)cum[b0] - key_pos(K[b0]);
        for (int e = 0; e < IPT; ++e) {
            const long long i = i0 + e;
            if (i < e0) elem_terms(a, K, cum, gst, i, b0, e0, base, thr);
        }
    }
    const Acc r = block_sum_acc(a, su, sd);
    if (threadIdx.x == 0) {
        uint64_t* pu = part_u + ((size_t)s * chunks + c) * ACC_U64;
        double* pd = part_d + ((size_t)s * chunks + c) * ACC_F64;
        pu[0] = r.tp, pu[1] = r.fp, pu[2] = r.P, pu[3] = r.auc, pu[4] = r.nthr, pu[5] = r.bad;
        pd[0] = r.aupr, pd[1] = r.bce;
    }
}

// Workgroup s adds slot s's tile partials in index order (thread t a contiguous run of them) and writes the slot.
__global__ __launch_bounds__(NT) void clf_final_kernel(const uint64_t* __restrict__ part_u,
                                                       const double* __restrict__ part_d,
                                                       const unsigned* __restrict__ bounds, long long chunks,
                                                       long long* __restrict__ counts, double* __restrict__ values) {
    __shared__ uint64_t su[NT / 64];
    __shared__ double sd[NT / 64];
    const unsigned s = blockIdx.x;
    const long long per = (chunks + NT - 1) / NT;
    const long long c0 = (long long)threadIdx.x * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    Acc a = acc_zero();
    for (long long c = c0; c < c1; ++c) {
        const uint64_t* pu = part_u + ((size_t)s * chunks + c) * ACC_U64;
        const double* pd = part_d + ((size_t)s * chunks + c) * ACC_F64;
        a.tp += pu[0], a.fp += pu[1], a.P += pu[2], a.auc += pu[3], a.nthr += pu[4], a.bad |= pu[5];
        a.aupr += pd[0], a.bce += pd[1];
    }
    const Acc r = block_sum_acc(a, su, sd);
    if (threadIdx.x == 0)
        finalize(r, (uint64_t)bounds[2 * s + 1] - (uint64_t)bounds[2 * s], counts + (size_t)s * IDDGCN_CLF_N_COUNTS,
                 values + (size_t)s * IDDGCN_CLF_N_VALUES);
}

struct ClfWs {
    size_t k0, k1, sorted, cum, gst, tsum, tmax, bounds, part_u, part_d, sort, total;
    long long m, nt, chunks;
    int end0, end1;
};

inline ClfWs clf_ws(long long n, int G) {
    ClfWs w;
    w.m = G > 0 ? 2 * n : n;
    w.nt = (w.m + TILE - 1) / TILE;
    w.chunks = (n + TILE - 1) / TILE;
    w.end0 = SLOT_SHIFT;
    w.end1 = SLOT_SHIFT + bit_length((uint64_t)G + 1);
    size_t o = 0;
    w.k0 = o;      o += al((size_t)n * 8);
    w.k1 = o;      o += al(G > 0 ? (size_t)n * 8 : 0);
    w.sorted = o;  o += al((size_t)w.m * 8);
    w.cum = o;     o += al((size_t)w.m * 4);
    w.gst = o;     o += al((size_t)w.m * 4);
    w.tsum = o;    o += al((size_t)w.nt * 4);
    w.tmax = o;    o += al((size_t)w.nt * 4);
    w.bounds = o;  o += al((size_t)(G + 2) * 2 * 4);
    w.part_u = o;  o += al((size_t)(G + 1) * w.chunks * ACC_U64 * 8);
    w.part_d = o;  o += al((size_t)(G + 1) * w.chunks * ACC_F64 * 8);
    w.sort = o;    o += (size_t)iddgcn_radix_sort_workspace(n, 8);
    w.total = o;
    return w;
}

// ---- keep-best / history --------------------------------------------------------------------------
__global__ void keep_best_decide_kernel(const double* __restrict__ value, int mode, double* __restrict__ best_value,
                                        int* __restrict__ best_epoch, const int* __restrict__ epoch,
                                        int* __restrict__ improved) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double v = value[0], b = best_value[0];
    int imp = 0;
    if (v == v) imp = best_epoch[0] < 0 ? 1 : (mode == 0 ? v > b : v < b);
    if (imp) {
        best_value[0] = v;
        best_epoch[0] = epoch[0];
    }
    improved[0] = imp;
}

__global__ __launch_bounds__(256) void keep_best_copy_kernel(long long n, const float* __restrict__ params,
                                                             float* __restrict__ best,
                                                             const int* __restrict__ improved) {
    if (!improved[0]) return;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) best[i] = params[i];
}

__global__ __launch_bounds__(256) void history_append_kernel(int n_counts, int n_values,
                                                             const long long* __restrict__ counts,
                                                             const double* __restrict__ values,
                                                             long long* __restrict__ hist_counts,
                                                             double* __restrict__ hist_values, int capacity,
                                                             int* __restrict__ counter) {
    const int k = counter[0];
    if (k >= 0 && k < capacity) {
        for (int i = threadIdx.x; i < n_counts; i += 256) hist_counts[(size_t)k * n_counts + i] = counts[i];
        for (int i = threadIdx.x; i < n_values; i += 256) hist_values[(size_t)k * n_values + i] = values[i];
    }
    __syncthreads();                       // every thread has read counter[0]
    if (threadIdx.x == 0 && k >= 0 && k < capacity) counter[0] = k + 1;
}

}  // namespace mt

extern "C" {

long long iddgcn_clf_metrics_workspace(long long n, int G) {
    if (n < 0 || n >= (1ll << 31) || G < 0 || G > IDDGCN_CLF_MAX_GROUPS) return IDDGCN_E_BAD_ARG;
    if (n <= IDDGCN_CLF_SMALL_MAX) return 0;
    return (long long)mt::clf_ws(n, G).total;
}

int iddgcn_clf_metrics(void* stream, long long n, int G, const float* prob, const float* label, const int* group,
                       double threshold, long long* counts, double* values, void* workspace,
                       long long workspace_bytes) {
    const long long need = iddgcn_clf_metrics_workspace(n, G);
    if (need < 0 || n < 1 || !prob || !label || !counts || !values || (G > 0 && !group)) return IDDGCN_E_BAD_ARG;
    if (need > 0 && (!workspace || workspace_bytes < need)) return IDDGCN_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n <= IDDGCN_CLF_SMALL_MAX) {
        hipLaunchKernelGGL(mt::clf_small_kernel, dim3(1 + G), dim3(mt::SMALL_NT), 0, st, (int)n, prob, label, group,
                           threshold, counts, values);
        return (int)hipGetLastError();
    }
    const mt::ClfWs w = mt::clf_ws(n, G);
    char* ws = (char*)workspace;
    uint64_t* k0 = (uint64_t*)(ws + w.k0);
    uint64_t* k1 = (uint64_t*)(ws + w.k1);
    uint64_t* sorted = (uint64_t*)(ws + w.sorted);
    unsigned* cum = (unsigned*)(ws + w.cum);
    unsigned* gst = (unsigned*)(ws + w.gst);
    unsigned* tsum = (unsigned*)(ws + w.tsum);
    unsigned* tmax = (unsigned*)(ws + w.tmax);
    unsigned* bounds = (unsigned*)(ws + w.bounds);
    uint64_t* part_u = (uint64_t*)(ws + w.part_u);
    double* part_d = (double*)(ws + w.part_d);
    const long long sort_bytes = iddgcn_radix_sort_workspace(n, 8);
    MT_CHECK(hipMemsetAsync(bounds, 0, (size_t)(G + 2) * 2 * 4, st));
    hipLaunchKernelGGL(mt::clf_keys_kernel, dim3((unsigned)((n + mt::NT - 1) / mt::NT)), dim3(mt::NT), 0, st, n, G,
                       prob, label, group, k0, k1);
    int rc = iddgcn_radix_sort_pairs(stream, n, 8, w.end0, k0, nullptr, sorted, nullptr, ws + w.sort, sort_bytes);
    if (rc) return rc;
    if (G > 0) {
        rc = iddgcn_radix_sort_pairs(stream, n, 8, w.end1, k1, nullptr, sorted + n, nullptr, ws + w.sort, sort_bytes);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mt::clf_tile_kernel, dim3((unsigned)w.nt), dim3(mt::NT), 0, st, sorted, w.m, tsum, tmax,
                       bounds);
    hipLaunchKernelGGL(mt::clf_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, tsum, tmax, w.nt);
    hipLaunchKernelGGL(mt::clf_apply_kernel, dim3((unsigned)w.nt), dim3(mt::NT), 0, st, sorted, w.m, tsum, tmax, cum,
                       gst);
    hipLaunchKernelGGL(mt::clf_terms_kernel, dim3((unsigned)w.chunks, (unsigned)(1 + G)), dim3(mt::NT), 0, st, sorted,
                       cum, gst, bounds, threshold, part_u, part_d);
    hipLaunchKernelGGL(mt::clf_final_kernel, dim3((unsigned)(1 + G)), dim3(mt::NT), 0, st, part_u, part_d, bounds,
                       w.chunks, counts, values);
    return (int)hipGetLastError();
}

int iddgcn_keep_best_f32(void* stream, long long n, const float* params, float* best, const double* value, int mode,
                         double* best_value, int* best_epoch, const int* epoch, int* improved) {
    if (n < 0 || (mode != 0 && mode != 1) || !value || !best_value || !best_epoch || !epoch || !improved)
        return IDDGCN_E_BAD_ARG;
    if (n > 0 && (!params || !best)) return IDDGCN_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mt::keep_best_decide_kernel, dim3(1), dim3(64), 0, st, value, mode, best_value, best_epoch,
                       epoch, improved);
    if (n > 0) {
        long long nb = (n + 256 * 4 - 1) / (256 * 4);
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(mt::keep_best_copy_kernel, dim3((unsigned)nb), dim3(256), 0, st, n, params, best,
                           improved);
    }
    return (int)hipGetLastError();
}

int iddgcn_clf_history_append(void* stream, int n_counts, int n_values, const long long* counts, const double* values,
                              long long* hist_counts, double* hist_values, int capacity, int* counter) {
    if (n_counts < 0 || n_values < 0 || capacity < 0 || !counter) return IDDGCN_E_BAD_ARG;
    if ((n_counts > 0 && (!counts || !hist_counts)) || (n_values > 0 && (!values || !hist_values)))
        return IDDGCN_E_BAD_ARG;
    hipLaunchKernelGGL(mt::history_append_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_counts, n_values,
                       counts, values, hist_counts, hist_values, capacity, counter);
    return (int)hipGetLastError();
}

}  // extern "C"
