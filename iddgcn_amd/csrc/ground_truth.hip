// ground_truth.hip — explanation ground truth for gfx950 (include/iddgcn_ground_truth.h; semantics there).
//
// Integer work only.  Two table builders on top of the stable LSD radix sort of graph_build.hip
// (iddgcn_radix_sort_pairs), then one query kernel instantiated as COUNT and as FILL:
//   sim lists : keys = node of [forward rows ; reversed rows], payload = position; the stable sort keeps the
//               table order inside each node's list.  A second stable sort of (node, value) with the list
//               position as payload puts the earliest position first in every run of equal pairs: that entry
//               is the value's first occurrence in its list.
//   dc table  : sort of the 64-bit keys (rel*N + drug)*N + mu, multiplicities kept; CSR pointers over
//               (rel, drug) by a lower_bound per pointer entry.
//   query     : one 256-thread workgroup per query walks the probe grid |SM| + |SD| + |SD|*|SM| in chunks of
//               256, one probe per thread (two binary searches in one (rel, drug) segment).  Thread order is
//               probe order, so the exclusive prefix of the hit counts (wave ballot + popcount when no cell is
//               repeated, a shuffle scan otherwise; cross-wave prefix in LDS; running base) is the output
//               position: no atomics, the reference's order.  The walk stores 1 into per-d / per-m flags in LDS
//               (idempotent plain stores); steps 4 and 5 are two more ordered compactions of hit && first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iddgcn.h"
#include "iddgcn_graph.h"
#include "iddgcn_ground_truth.h"

namespace gt {

constexpr int NT = 256;                       // threads per query workgroup = probes per chunk
constexpr int NW = NT / 64;
constexpr int CAP = IDDGCN_GT_LIST_CAPACITY;  // hit flags per side in LDS

#define GT_CHECK(x)                              \
    do {                                         \
        const hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return (int)e_;    \
    } while (0)

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned grid1(long long n, int b) { return (unsigned)((n + b - 1) / b); }
inline int bit_length(uint64_t x) {
    int b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

__device__ __forceinline__ unsigned mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x) {
    const unsigned lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= (unsigned)o) x += y;
    }
    return x;
}

// first index in [lo, hi) with a[i] >= v
template <typename T>
__device__ __forceinline__ long long lower_bound(const T* __restrict__ a, long long lo, long long hi, T v) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- similarity lists ----------------------------------------------------------------------------
__device__ __forceinline__ unsigned checked_id(long long v, int N, int* err) {
    if (v < 0 || v >= N) {
        *err = 1;
        return 0u;
    }
    return (unsigned)v;
}

// entry i of [forward rows ; reversed rows]: the node whose list it joins
__global__ void sim_keys_kernel(const long long* __restrict__ sim, long long n, int N, unsigned* __restrict__ key,
                                int* __restrict__ err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    key[i] = checked_id(i < n ? sim[3 * i] : sim[3 * (i - n) + 2], N, err);
}

// sorted entry k (node skey[k], source position pos[k]): its value, and the (node, value) key
__global__ void sim_vals_kernel(const long long* __restrict__ sim, long long n, int N, const unsigned* __restrict__ skey,
                                const unsigned* __restrict__ pos, int* __restrict__ val, uint64_t* __restrict__ key64,
                                int* __restrict__ err) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * n) return;
    const long long p = pos[k];
    const unsigned v = checked_id(p < n ? sim[3 * p + 2] : sim[3 * (p - n)], N, err);
    val[k] = (int)v;
    key64[k] = (uint64_t)skey[k] * (uint64_t)N + v;
}

__global__ void sim_first_kernel(const uint64_t* __restrict__ skey64, const unsigned* __restrict__ perm, long long n2,
                                 unsigned char* __restrict__ first) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n2) return;
    first[perm[j]] = (j == 0 || skey64[j] != skey64[j - 1]) ? 1 : 0;
}

// ptr[v] = first sorted entry whose key is >= v * scale, v in [0, count)
template <typename T>
__global__ void lower_bound_ptr_kernel(const T* __restrict__ skey, long long n, T scale, long long count,
                                       int* __restrict__ ptr) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= count) return;
    ptr[v] = (int)lower_bound<T>(skey, 0, n, (T)v * scale);
}

// ---- dc lookup table -------------------------------------------------------------------------------
__global__ void dc_keys_kernel(const long long* __restrict__ dc, long long M, int N, int R, uint64_t* __restrict__ key,
                               int* __restrict__ err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const unsigned mu = checked_id(dc[3 * i], N, err);
    const unsigned rel = checked_id(dc[3 * i + 1], R, err);
    const unsigned drug = checked_id(dc[3 * i + 2], N, err);
    key[i] = ((uint64_t)rel * (uint64_t)N + drug) * (uint64_t)N + mu;
}

__global__ void dc_mu_kernel(const uint64_t* __restrict__ skey, long long M, int N, int* __restrict__ seg_mu) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    seg_mu[j] = (int)(skey[j] % (uint64_t)N);
}

// ---- exclusive scan of the query lengths (one workgroup) ---------------------------------------------
__global__ __launch_bounds__(1024) void scan_len_kernel(const long long* __restrict__ len, int Q,
                                                        long long* __restrict__ ptr) {
    __shared__ long long wsum[16];
    __shared__ long long carry;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
        carry = 0;
        ptr[0] = 0;
    }
    __syncthreads();
    for (int c0 = 0; c0 < Q; c0 += 1024) {
        const int c = c0 + tid;
        const long long x = c < Q ? len[c] : 0ll;
        const long long incl = wave_incl_scan<long long>(x);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long pre = carry;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        if (c < Q) ptr[c + 1] = pre + incl;
        __syncthreads();
        if (tid == 1023) carry = pre + incl;
        __syncthreads();
    }
}

// ---- the query kernel ----------------------------------------------------------------------------------
struct Tables {
    const int* mu_ptr;
    const int* mu_val;
    const unsigned char* mu_first;
    const int* drug_ptr;
    const int* drug_val;
    const unsigned char* drug_first;
    const int* seg_ptr;
    const int* seg_mu;
};

// Exclusive prefix of `cnt` over the workgroup in thread order, and the workgroup total.  wsum is this call's
// [NW] slot; the caller alternates two slots, so one barrier per call is enough.
__device__ __forceinline__ unsigned block_excl(unsigned cnt, unsigned* wsum, unsigned& total) {
    const int wave = threadIdx.x >> 6;
    const uint64_t hit = __ballot(cnt > 0u);
    unsigned excl, wtot;
    if (__ballot(cnt > 1u) == 0ull) {          // wave-uniform: every hit takes one slot
        excl = mbcnt(hit);
        wtot = (unsigned)__popcll(hit);
    } else {
        const unsigned incl = wave_incl_scan<unsigned>(cnt);
        excl = incl - cnt;
        wtot = __shfl(incl, 63, 64);
    }
    if ((threadIdx.x & 63) == 0) wsum[wave] = wtot;
    __syncthreads();
    unsigned pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const unsigned s = wsum[w];
        if (w < wave) pre += s;
        tot += s;
    }
    total = tot;
    return pre + excl;
}

template <bool FILL>
__global__ __launch_bounds__(NT) void ground_truth_kernel(const long long* __restrict__ queries, int N, Tables t,
                                                          long long* __restrict__ len,
                                                          const long long* __restrict__ ptr, int drug_rel, int mu_rel,
                                                          long long* __restrict__ out, int* __restrict__ err) {
    __shared__ unsigned char hit_m[CAP];
    __shared__ unsigned char hit_d[CAP];
    __shared__ unsigned wsum[2][NW];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const int mu0 = (int)queries[3 * q], rel0 = (int)queries[3 * q + 1], drug0 = (int)queries[3 * q + 2];
    const int ms = t.mu_ptr[mu0], ds = t.drug_ptr[drug0];
    const unsigned nm = (unsigned)(t.mu_ptr[mu0 + 1] - ms), nd = (unsigned)(t.drug_ptr[drug0 + 1] - ds);
    if (nm > (unsigned)CAP || nd > (unsigned)CAP) {      // uniform over the workgroup; never truncate
        if (!FILL && tid == 0) {                         // the caller reads err before it sizes the FILL
            *err = 1;
            len[q] = 0;
        }
        return;
    }
    for (unsigned i = tid; i < nm; i += NT) hit_m[i] = 0;
    for (unsigned i = tid; i < nd; i += NT) hit_d[i] = 0;
    __syncthreads();
    long long* dst = FILL ? out + 3 * ptr[q] : nullptr;
    const long long seg0 = (long long)rel0 * N;
    long long base = 0;                                  // triples emitted so far (uniform)
    int buf = 0;
    // steps 1-3: probe i is (m_i, rel0, drug0) for i < nm, (mu0, rel0, d) for the next nd, then d-major (d, m)
    const unsigned total = nm + nd + nd * nm;            // <= 2 CAP + CAP^2 < 2^32
    for (unsigned c0 = 0; c0 < total; c0 += NT, buf ^= 1) {
        const unsigned i = c0 + tid;
        unsigned cnt = 0;
        int m = 0, d = 0;
        if (i < total) {
            int mi = -1, di = -1;
            if (i < nm) mi = (int)i;
            else if (i < nm + nd) di = (int)(i - nm);
            else {
                const unsigned j = i - nm - nd;
                di = (int)(j / nm);
                mi = (int)(j - (unsigned)di * nm);
            }
            m = mi < 0 ? mu0 : t.mu_val[ms + mi];
            d = di < 0 ? drug0 : t.drug_val[ds + di];
            const long long lo = t.seg_ptr[seg0 + d], hi = t.seg_ptr[seg0 + d + 1];
            if (lo < hi) {
                const long long a = lower_bound<int>(t.seg_mu, lo, hi, m);
                if (a < hi && t.seg_mu[a] == m) cnt = (unsigned)(lower_bound<int>(t.seg_mu, a + 1, hi, m + 1) - a);
            }
            if (cnt) {
                if (mi >= 0) hit_m[mi] = 1;
                if (di >= 0) hit_d[di] = 1;
            }
        }
        unsigned tot;
        const unsigned off = block_excl(cnt, wsum[buf], tot);
        if (FILL)
            for (unsigned c = 0; c < cnt; ++c) {
                long long* o = dst + 3 * (base + off + c);
                o[0] = m;
                o[1] = rel0;
                o[2] = d;
            }
        base += tot;
    }
    __syncthreads();                                     // the hit flags are complete
    // step 4: (drug0, drug_rel, d) at d's first occurrence in SD, if any probe of d hit
    for (unsigned c0 = 0; c0 < nd; c0 += NT, buf ^= 1) {
        const unsigned k = c0 + tid;
        const unsigned cnt = (k < nd && hit_d[k] && t.drug_first[ds + k]) ? 1u : 0u;
        unsigned tot;
        const unsigned off = block_excl(cnt, wsum[buf], tot);
        if (FILL && cnt) {
            long long* o = dst + 3 * (base + off);
            o[0] = drug0;
            o[1] = drug_rel;
            o[2] = t.drug_val[ds + k];
        }
        base += tot;
    }
    // step 5: (mu0, mu_rel, m) at m's first occurrence in SM, if any probe of m hit
    for (unsigned c0 = 0; c0 < nm; c0 += NT, buf ^= 1) {
        const unsigned k = c0 + tid;
        const unsigned cnt = (k < nm && hit_m[k] && t.mu_first[ms + k]) ? 1u : 0u;
        unsigned tot;
        const unsigned off = block_excl(cnt, wsum[buf], tot);
        if (FILL && cnt) {
            long long* o = dst + 3 * (base + off);
            o[0] = mu0;
            o[1] = mu_rel;
            o[2] = t.mu_val[ms + k];
        }
        base += tot;
    }
    if (!FILL && tid == 0) len[q] = base;
}

struct SimWs {
    size_t key, skey, pos, key64, skey64, perm, sort, total;
};

inline SimWs sim_ws(long long n2) {
    SimWs w;
    size_t o = 0;
    w.key = o;    o += al((size_t)n2 * 4);
    w.skey = o;   o += al((size_t)n2 * 4);
    w.pos = o;    o += al((size_t)n2 * 4);
    w.key64 = o;  o += al((size_t)n2 * 8);
    w.skey64 = o; o += al((size_t)n2 * 8);
    w.perm = o;   o += al((size_t)n2 * 4);
    w.sort = o;   o += (size_t)iddgcn_radix_sort_workspace(n2, 8);      // >= the 4-byte sort's need
    w.total = o;
    return w;
}

inline bool dc_sizes_ok(long long M, int N, int R) {
    if (M < 0 || M >= (1ll << 31) || N < 1 || R < 1) return false;
    if ((long long)R * N >= (1ll << 31)) return false;
    return (uint64_t)R * (uint64_t)N <= (1ull << 62) / (uint64_t)N;
}

inline bool tables_ok(const Tables& t) {
    return t.mu_ptr && t.mu_val && t.mu_first && t.drug_ptr && t.drug_val && t.drug_first && t.seg_ptr && t.seg_mu;
}

}  // namespace gt

extern "C" {

int iddgcn_gt_sim_lists_workspace(long long n, long long* bytes) {
    if (!bytes || n < 0 || 2 * n >= (1ll << 31)) return IDDGCN_E_BAD_ARG;
    *bytes = (long long)gt::sim_ws(2 * n).total;
    return 0;
}

int iddgcn_gt_sim_lists(void* stream, long long n, int N, const long long* sim, int* ptr, int* val,
                        unsigned char* first, int* err, void* workspace, long long workspace_bytes) {
    using namespace gt;
    long long need;
    if (iddgcn_gt_sim_lists_workspace(n, &need) != 0 || N < 1) return IDDGCN_E_BAD_ARG;
    if (!ptr || !err || (n > 0 && (!sim || !val || !first || !workspace || workspace_bytes < need)))
        return IDDGCN_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long n2 = 2 * n;
    const SimWs w = sim_ws(n2);
    char* ws = (char*)workspace;
    unsigned* key = (unsigned*)(ws + w.key);
    unsigned* skey = (unsigned*)(ws + w.skey);
    unsigned* pos = (unsigned*)(ws + w.pos);
    uint64_t* key64 = (uint64_t*)(ws + w.key64);
    uint64_t* skey64 = (uint64_t*)(ws + w.skey64);
    unsigned* perm = (unsigned*)(ws + w.perm);
    GT_CHECK(hipMemsetAsync(err, 0, sizeof(int), st));
    if (n2 > 0) {
        const long long sortb = iddgcn_radix_sort_workspace(n2, 8);
        hipLaunchKernelGGL(sim_keys_kernel, dim3(grid1(n2, 256)), dim3(256), 0, st, sim, n, N, key, err);
        int rc = iddgcn_radix_sort_pairs(stream, n2, 4, bit_length((uint64_t)(N - 1)), key, nullptr, skey, pos,
                                         ws + w.sort, sortb);
        if (rc) return rc;
        hipLaunchKernelGGL(sim_vals_kernel, dim3(grid1(n2, 256)), dim3(256), 0, st, sim, n, N, skey, pos, val, key64,
                           err);
        rc = iddgcn_radix_sort_pairs(stream, n2, 8, bit_length((uint64_t)N * (uint64_t)N - 1), key64, nullptr, skey64,
                                     perm, ws + w.sort, sortb);
        if (rc) return rc;
        hipLaunchKernelGGL(sim_first_kernel, dim3(grid1(n2, 256)), dim3(256), 0, st, skey64, perm, n2, first);
    }
    hipLaunchKernelGGL(lower_bound_ptr_kernel<unsigned>, dim3(grid1((long long)N + 1, 256)), dim3(256), 0, st, skey,
                       n2, 1u, (long long)N + 1, ptr);
    return (int)hipGetLastError();
}

int iddgcn_gt_dc_table_workspace(long long M, int N, int R, long long* bytes) {
    if (!bytes || !gt::dc_sizes_ok(M, N, R)) return IDDGCN_E_BAD_ARG;
    *bytes = (long long)(2 * gt::al((size_t)M * 8)) + iddgcn_radix_sort_workspace(M, 8);
    return 0;
}

int iddgcn_gt_dc_table(void* stream, long long M, int N, int R, const long long* dc, int* seg_ptr, int* seg_mu,
                       int* err, void* workspace, long long workspace_bytes) {
    using namespace gt;
    long long need;
    if (iddgcn_gt_dc_table_workspace(M, N, R, &need) != 0) return IDDGCN_E_BAD_ARG;
    if (!seg_ptr || !err || (M > 0 && (!dc || !seg_mu || !workspace || workspace_bytes < need)))
        return IDDGCN_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint64_t* key = (uint64_t*)ws;
    uint64_t* skey = (uint64_t*)(ws + al((size_t)M * 8));
    char* sort = ws + 2 * al((size_t)M * 8);
    GT_CHECK(hipMemsetAsync(err, 0, sizeof(int), st));
    if (M > 0) {
        hipLaunchKernelGGL(dc_keys_kernel, dim3(grid1(M, 256)), dim3(256), 0, st, dc, M, N, R, key, err);
        const int rc = iddgcn_radix_sort_pairs(stream, M, 8, bit_length((uint64_t)R * N * (uint64_t)N - 1), key,
                                               nullptr, skey, nullptr, sort, iddgcn_radix_sort_workspace(M, 8));
        if (rc) return rc;
        hipLaunchKernelGGL(dc_mu_kernel, dim3(grid1(M, 256)), dim3(256), 0, st, skey, M, N, seg_mu);
    }
    const long long segs = (long long)R * N + 1;
    hipLaunchKernelGGL(lower_bound_ptr_kernel<uint64_t>, dim3(grid1(segs, 256)), dim3(256), 0, st, skey, M,
                       (uint64_t)N, segs, seg_ptr);
    return (int)hipGetLastError();
}

int iddgcn_ground_truth_count(void* stream, int Q, int N, int R, const long long* queries, const int* mu_ptr,
                              const int* mu_val, const unsigned char* mu_first, const int* drug_ptr,
                              const int* drug_val, const unsigned char* drug_first, const int* seg_ptr,
                              const int* seg_mu, long long* len, int* err) {
    using namespace gt;
    const Tables t{mu_ptr, mu_val, mu_first, drug_ptr, drug_val, drug_first, seg_ptr, seg_mu};
    if (Q < 0 || N < 1 || R < 1 || !tables_ok(t) || !err || (Q > 0 && (!queries || !len))) return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    hipLaunchKernelGGL(ground_truth_kernel<false>, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, queries, N, t,
                       len, (const long long*)nullptr, 0, 0, (long long*)nullptr, err);
    return (int)hipGetLastError();
}

int iddgcn_gt_exclusive_scan(void* stream, int Q, const long long* len, long long* ptr) {
    if (Q < 0 || !ptr || (Q > 0 && !len)) return IDDGCN_E_BAD_ARG;
    hipLaunchKernelGGL(gt::scan_len_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, len, Q, ptr);
    return (int)hipGetLastError();
}

int iddgcn_ground_truth_fill(void* stream, int Q, int N, int R, const long long* queries, const int* mu_ptr,
                             const int* mu_val, const unsigned char* mu_first, const int* drug_ptr,
                             const int* drug_val, const unsigned char* drug_first, const int* seg_ptr,
                             const int* seg_mu, const long long* ptr, int drug_rel, int mu_rel, long long* triples) {
    using namespace gt;
    const Tables t{mu_ptr, mu_val, mu_first, drug_ptr, drug_val, drug_first, seg_ptr, seg_mu};
    if (Q < 0 || N < 1 || R < 1 || !tables_ok(t) || (Q > 0 && (!queries || !ptr || !triples)))
        return IDDGCN_E_BAD_ARG;
    if (Q == 0) return 0;
    hipLaunchKernelGGL(ground_truth_kernel<true>, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, queries, N, t,
                       (long long*)nullptr, ptr, drug_rel, mu_rel, triples, (int*)nullptr);
    return (int)hipGetLastError();
}

}  // extern "C"
