// per_query.hpp — what the per-query kernels of screen.hip and explain.hip share: the host-side width dispatch and
// layer check of their C entries, and the device pieces that compile to the same machine code from here as they did
// written out in each kernel (tools/kernel_asm_digest.py is the test; DESIGN.md lists what stayed duplicated).
#pragma once
#include <hip/hip_runtime.h>

#include "iddgcn_screen.h"

namespace pq {

// ---- host: the C entries ---------------------------------------------------------------------------------------
template <int V>
struct Int { static constexpr int value = V; };

// f(Int<D>{}) for the widths of the per-query kernels, d in {32, 64}, in the style of for_width (iddgcn_hip.hip).
// The entries refuse every other d first (anything else would run as 32).
template <class F>
void for_small_width(int d, F&& f) {
    if (d == 64)
        f(Int<64>{});
    else
        f(Int<32>{});
}

// every one of the three layers' pointers is set, in each of the arrays given (K, S, Wa, ba, ...)
template <class... A>
bool layers_ok(const A&... arrays) {
    for (int l = 0; l < 3; ++l)
        if (!(... && (arrays[l] != nullptr))) return false;
    return true;
}

// ---- device ----------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// layer activations as the row GEMM's epilogue computes them (v_exp_f32 + v_rcp_f32, saturating to exactly 0 / 1)
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *(f32x4*)p = v; }

// selection (rank_topk_kernel, topk_kernel): passes of TK_CH candidates merged into the running top 64.  The merge pass
// itself (key store, bitonic sort, running-top update) is written out in both kernels: as a function here it compiled
// to other scalar register numbers and another order of constant moves, and the rule for these kernels is an
// identical digest.  The relation-segment scan (rstart) and the E-row staging (es) of the fused explainer kernels
// stayed written out for the same reason until those kernels' rule became bitwise results within the same budget
// (profiles/r21/): they are functions of explain.hip now.
constexpr int TK_BUF = 1024;                           // keys sorted per pass
constexpr int TK_CH = TK_BUF - IDDGCN_TOPK_MAX;        // new candidates per pass; buf[TK_CH..) holds the running top

// larger key = better candidate: value descending (-0.0 taken as +0.0), then id ascending; 0 = no candidate
__device__ __forceinline__ unsigned long long make_key(float v, int c) {
    if (v == 0.0f) v = 0.0f;
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
}

}  // namespace pq
