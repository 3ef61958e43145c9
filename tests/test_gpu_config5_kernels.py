"""Bars that can fail for the kernels behind BASELINE config 5 (bf16 edge tables) and for the split-fp16 operand mode
with its planes tables, all D = 256: iddgcn_rowgemm_bf16 (rowgemm256_v3_kernel's BF variants and
fwd_gather8_bf16_kernel<HL>), iddgcn_gemm_tn_bf16 (gemm_tn256_bf16t_kernel), iddgcn_sigma_tn_bf16
(sigma_tn_bf16_kernel<W1>), iddgcn_tail_seg_reduce_bf16 / _head_bf16 (tail_seg_mfma8_kernel<DSUM, HEAD> and the VALU
form), iddgcn_combine_bf16, iddgcn_distmult_bce_bf16 / _heads_bf16; iddgcn_rowgemm_f32 and iddgcn_rowgemm_batched_f32 at
precision "split", gemm_tn256_x3_kernel through iddgcn_gemm_tn_f32 / _batched_f32, iddgcn_gemm_tn_planes_f32, the
IDDGCN_PLANES_A / C / AUX flags of the row GEMM and the planes-out combine.

Conventions of test_gpu_mfma_gemms.py: every GPU test compares a kernel with an fp64 (or integer) torch evaluation of
the same operation on the same STORED inputs (bf16 tables as they are, planes tables decoded); no bar is taken from
another kernel's output (bitwise equalities between kernels and between two runs are extra assertions); outputs are
prefilled with NaN and carry a guard row.  The one assumed hardware constant is that module's MFMA_ADD (one fp32 ulp
of the running sum per add inside an MFMA); its gam_e, sigmoid_bar / sig_fast_rel and case builders are imported, as
are the bound builders of test_gpu_step_kernels.py for the VALU forms.

The bar of a value stored as bf16 (bounds.bf16_interval): the kernel's fp32 value y before the rounding satisfies
|y - z| <= b, rounding fp64 -> fp32 -> bf16 is monotone, so the stored value lies in [bf16(f32(z - b)), bf16(f32(z + b))].
For most elements that is ONE bf16 number: bitwise, no measured constant.  Every test prints the share of elements
whose interval holds more than one value and asserts it is at most 5% (a condition on the reference alone; the inputs
are scaled for it: family C operands are POSITIVE, so that the sum of moduli T equals |z|; with random signs T / |z| of a
256-term sum is ~16 and a third of the intervals are ambiguous).

Three input families:
  A. EXACT INTEGERS in [-4, 4] (bf16 and fp16 values under any power-of-two scale: every low piece is zero; the sigma'
     operand from {1/4, 1/2, 3/4}; planes of multiples of 1/4): every product and partial sum exact (sum |terms| < 2^24
     asserted from the reference), so the fp32 result is exact in any order and a bf16 output is its round-to-nearest.
     BITWISE.  Gathered-row addressing: A = 0, one-hot coefficients, distinct V rows of bf16 values.  Split-fp16 also
     with rows times 2^k, k = -20..20 (row GEMM: pow2_scale / pow2_inv) and tiles times 2^(2 j) (TN: the running
     block scale lowered, kept, met by zero tiles first and in the middle of a row range).
  B. SINGLE TERMS: full-mantissa values placed so that every output element is one product; sees the low pieces.
  C. DENSE operands at short lengths: bound = (gamma_e(n) + rep) T per element, n the adds on the longest path at
     e = MFMA_ADD, T the sum of moduli of the element's terms.

Error model, each term from the source:
  * bf16 hi + lo weights (iddgcn_hip.hip: rowgemm256_v3_kernel with BF, sigma_tn_bf16_kernel and
    fwd_gather8_bf16_kernel: hi = bf16(w), lo = bf16(w - hi)): w - hi is within half a bf16 ulp of w, 2^-8 2^e with 2^e <= |w|; its own ulp is then at most 2^(e-16), so
    |w - hi - lo| <= 2^-17 |w| = REP_HL.  (2^-18 |w| is not a bound: test_selfcheck_hilo_representation finds random
    weights beyond it.)  A bf16 x bf16 product is exact in fp32; n = 2 D (two MFMAs per k-step), one product a hi + a lo
    is one add: HL_SINGLE = REP_HL + MFMA_ADD (1 + 2^-8).
  * IDDGCN_GEMM_BF16 (include/iddgcn.h:63-70): the reference takes the weights rounded to bf16, in fwd_gather8 also
    the node rows and coefficients: no representation term, n = D, a single product is exact (family B bitwise).
  * fwd_gather8's combine (:4976-5009): ch vh + cl vh + ch vl into the accumulators that hold x S (no separate add):
    n grows by 3 R (R with bf16 operands); |cl| <= 2^-8 (1 + 2^-8) |c| and likewise vl, so the dropped cl vl is at most
    2^-16 (1 + 2^-8)^2 |c v| (not 2^-18), plus 2 REP_HL + REP_HL^2 of the pieces: REP_COMB ~ 2^-15.  The v3 kernel's
    combine (R <= 2, and R = 8 with an unaligned coefficient table) is R fp32 fused multiply-adds.
  * sigma' epilogue: 1 - x, x (1 - x), the product: n + 3; bf16 x is exact in fp32.
  * TN over bf16 tables and sigma_tn's dS: exact products, n = M + partials (+ accumulate); family B is bitwise.
  * tail_seg_mfma8 (:4114-4136): W, P and head_dO enter as EXACT three-piece splits (no representation, no drop):
    three products per non-zero term of dP and dWedge (+ the DPP add of dWedge's two columns), nine of dwh (+ 3), one
    of dsum; HEAD adds one fused multiply-add / add.  Exact zeros add nothing, so a single-term element has n = 3.
  * split-fp16 (:448-477, :1354-1365): a value scaled by a power of two so that its row / column / block maximum lies in
    [2^14, 2^15) is hi + lo with 22 significant bits while lo is a normal fp16 (REP16 = 2^-22 relative), else within
    2^-25 of the scaled value (split16_same: ABS_SAME = 2^-39 of the row or block maximum; split16 of the weights,
    lo carried at 2^11: ABS_W = 2^-50 of the column maximum); the dropped lo lo is REP16.  Per product 3 REP16 |a w| +
    ABS_SAME max |w| + ABS_W max |a|.  Row GEMM: n = 2 D + 1 (wh ah + wh al in one accumulator, + 2^-11 (wl ah)); TN:
    n = 3 M + partials, the block maximum taken over the whole table (the running maximum never exceeds it; the
    power-of-two rescaling of the accumulators is exact).  A planes A table (x 2^15 = hi + lo) is compared on its
    decoded values: no A-side term.

Not covered here as the issue words it: fwd_gather8's tile loop needs more than 256 tiles of 64 rows to give a
workgroup a second tile, so its multi-tile case uses 32 833 rows (three tiles per workgroup; beyond the 10 000-row
limit, 16 MiB, under a second); its node tables stay below 5 000 rows.

What the bars replace.  No existing test is removed or loosened: tests/test_gpu_bf16.py, the split cases of
tests/test_gpu_kernels.py and tests/test_gpu_planes.py stay as workload-sized checks (M = 20 017 .. 300 017, the
2^32-offset case, determinism).  Their limits, for scale: bf16 outputs 6e-3 of max|ref| (a lost lo weight piece is
2^-9 relative, a dropped k term 4e-3 of one element); fp32 outputs 1e-5 of max|ref| with dO ~ 1e-3 N(0, 1) against
X ~ U(0, 1); split-fp16 max(2 x the exact kernel's own error, 1e-6) of max|ref|.  Here a dropped k term trips 15-55%
of the stored bf16 elements of a dense case (96% of a split-fp16 one), a lost lo weight piece 26% of a single-term
bf16 case (100% before the output rounding), every family-A case is bitwise.

Worst observed |err| / bound on an MI355X (1 = at the bound; every family-A case bitwise; the bf16 outputs: share of
ambiguous intervals, every stored value inside, at most one bf16 ulp from bf16(ref) except where noted):
    rowgemm_bf16 v3 / fwd_gather8   dense: ambiguous 2.2-2.7% (hi + lo), 1.0-1.6% (bf16 weights), gathered R = 8
                                    3.9% (MFMA combine) and 4.7% (v3 combine), sigmoid forms 0.4-1.6%; single term
                                    0.3% / 0 (bf16 weights: bitwise); combine single term 1.1% (fwd_gather8 hi + lo)
    sigma_tn_bf16                   dS dense 0.038, single bitwise; dx dense ambiguous 2.8% / 1.2%, single 0.3% / 0.02%
    gemm_tn_bf16                    dense 0.17; single bitwise (with accumulate: the one rounding, 1.0)
    tail_seg_mfma8                  dP 0.31 (HEAD 0.49), dWedge dense 0.0011, single 0.31, dsum 0.0023 (HEAD 0.24),
                                    dwh dense 0.00016, single 0.11; head_dz on its outputs 0.080
    tail_seg_reduce_bf16 (VALU)     dP 0.65, dsum 0.43, dWedge 0.0031
    combine_bf16                    ambiguous <= 0.06%
    distmult_bce(_heads)_bf16       s 0.0099, p 0.023, ds 0.048, drel 0.023, loss 0.012, dXh 0.067; do ambiguous 0.8%;
                                    prediction seed: ds 0.025, dXh 0.029, do ambiguous 3.2% (its saturated edges have
                                    ds = scale p q with q ~ 1e-10 known to a few per cent only: the interval there is
                                    wide and the stored value up to 255 bf16 ulp from bf16(ref), inside it)
    rowgemm split                   dense 0.0022-0.0039 on every variant (gamma_e(2 D) grows like n, the errors do
                                    not align), zero rows with the sigmoid 0.41 (sigmoid_fast alone); single 0.46-0.86
    gemm_tn split (+ batched)       dense 0.37 (short M), single 0.54, batched single 0.51
    planes                          consumers dense 0.0018-0.0037, TN 0.51; producers: combine 0.66, row GEMM 0.0038
CPU self-checks (no `gpu` mark): a torch emulation of each kernel's arithmetic (piece splits by .to(bfloat16) /
.half(), the kept products summed in fp64, the fp32 epilogue, the output rounding) lies inside every bar, and these
mutants are refused (share of elements tripped): a dropped k term (bf16 dense 15-55%, split 63-97%); a gathered row
replaced by its neighbour (90-98% of that row); the last ragged tile left at its sentinel (NaN: all of it); the lo
weight piece dropped (single term 26% stored / 100% before the rounding; dense ~1%); one of the three pieces of a
tail_seg_mfma8 operand (single term: hi 100%, mid 100%, lo 76-78%; dense: hi 100%, mid 57-93%, lo 0-22%: the third
piece is family B's to see); the ch vl product of fwd_gather8's combine (single term 26% stored / 99% before); one
row of the last TN block (99-100% at short M); a split-fp16 block scale off by two for one tile (dense 80-99%,
single term the tile's 2% of the columns); a bf16 output truncated instead of rounded (47-50%).

GPU time of the module on an MI355X: 15 s for its 223 GPU cases (the slowest, the 32 833-row gathered forward, 2.5 s).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_mfma_gemms as G
import test_gpu_step_kernels as K
from bounds import (BF16, NAN, U, ambiguous_share, assert_bf16_interval, assert_within, bf16_interval, gam, guard_intact,
                    guarded, outside_interval, rejects, rejects_interval, to_bf16)
from iddgcn_amd import _lib as L
from iddgcn_amd import ops
from test_gpu_mfma_gemms import LIM, MFMA_ADD, assert_bitwise, gam_e, ints, sigmoid_bar, spread_rows

gpu = pytest.mark.gpu
F64, F32, I32 = torch.float64, torch.float32, torch.int32
D = 256
REP_HL = 2.0 ** -17                         # |w - hi - lo| <= REP_HL |w|, hi = bf16(w), lo = bf16(w - hi)
HL_SINGLE = REP_HL + MFMA_ADD * (1 + 2.0 ** -8)      # one product a w as a hi + a lo: the representation + one add
REP_COMB = 2.0 ** -16 * (1 + 2.0 ** -8) ** 2 + 2 * REP_HL + REP_HL ** 2     # c v as ch vh + ch vl + cl vh
COMB_SINGLE = REP_COMB + 2 * MFMA_ADD * (1 + 2.0 ** -7)                     # + two adds of the three products
AMBIGUOUS_MAX = 0.05


def _gen(*seed):
    return G._gen(5, *seed)


def hilo(w):
    """The kernels' weight pieces (iddgcn_hip.hip, rowgemm256_v3_kernel with BF): hi = bf16(w), lo = bf16(w - hi), as fp64."""
    hi = w.float().to(BF16).float()
    lo = (w.float() - hi).to(BF16).float()
    return hi.double(), lo.double()


def trunc_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (the mutant of the output rounding), as fp64."""
    return (x.float().contiguous().view(I32) & -65536).view(F32).double()


def share(mask):
    return float(mask.double().mean()) if mask.numel() else 0.0


# =============================================================================================================
# iddgcn_rowgemm_bf16: rowgemm256_v3_kernel<.., BF> and fwd_gather8_bf16_kernel<HL>
# =============================================================================================================
def _bf_forms():
    F = {"plain": {}, "b_trans": dict(b_trans=True), "sig": dict(act="sig"),
         "dsig": dict(b_trans=True, act="dsig"), "dsig_inplace": dict(b_trans=True, act="dsig", alias=True),
         "a_idx": dict(a_idx=True), "a_idx_dsig": dict(a_idx=True, b_trans=True, act="dsig")}
    for R in (1, 2, 8):
        F[f"gather_R{R}"] = dict(R=R)
        F[f"gather_R{R}_sig"] = dict(R=R, act="sig")
    # the R = 8 forward with a coefficient table 4 B off 16-B alignment: iddgcn_rowgemm_bf16 sends it to the v3 kernel
    F["gather_R8_v3"] = dict(R=8, unaligned=True)
    F["gather_R8_v3_sig"] = dict(R=8, unaligned=True, act="sig")
    return F


BF_FORMS = _bf_forms()
LINEAR_FORMS = [f for f, o in BF_FORMS.items() if o.get("act") != "sig"]
V3_MS = (1, 31, 32, 33, 785)
V3_M2 = 256 * 32 + 33          # launch_v3: min(tiles, 256) workgroups, so 258 tiles are two per workgroup (ragged last)
FG8_MS = (1, 63, 64, 65, 785)
FG8_M3 = 2 * 256 * 64 + 65     # launch_fwd_gather8: 514 tiles of 64 rows over 172 workgroups: three tiles each
VK8 = ("one", "four", "five", "all", "runs13", "random")


def v_index8(kind, M, g):
    """(v_idx, table rows).  Distinct V rows (runs of equal v_idx: the kernel's slots) per 64-row tile: one; exactly 4
    (the staged block); 5 (one slot past it); 64 (identity); sorted runs of 1-3; unsorted (64 distinct rows)."""
    e = torch.arange(M)
    if kind == "one":
        return torch.full((M,), 1, dtype=torch.int64), 3
    if kind == "four":
        idx = e // 16
    elif kind == "five":
        idx = 5 * (e // 64) + torch.clamp((e % 64) // 13, max=4)
    elif kind == "all":
        idx = e.clone()
    elif kind == "runs13":
        idx = torch.repeat_interleave(torch.arange(M), torch.randint(1, 4, (M,), generator=g))[:M]
    else:
        N = max(M, 70)
        return torch.randperm(N, generator=g)[:M], N
    return idx, int(idx.max()) + 1


def slots_per_tile(v_idx, tile=64):
    """Runs of equal v_idx in every tile (the gather kernels' slots)."""
    out = []
    for t in range(0, len(v_idx), tile):
        w = v_idx[t:t + tile]
        out.append(1 + int((w[1:] != w[:-1]).sum()))
    return out


def bf_case(M, form, kind, vkind="runs13"):
    """CPU operands of one bf16 row GEMM: A and aux bf16 (as stored), weights / coefficients / node rows fp32.
    kind: "int" (family A), "single" (family B: A row e non-zero only in column e mod D; coefficients zero), "dense"
    (family C: every operand POSITIVE, so that T = |z| and the bf16 interval of the output is a single value on all but
    a few per cent of the elements; A, coef ~ U(0, 1), weights in [1/256, 1/64], V in [0, 1/4]: |z| < 4)."""
    opt = BF_FORMS[form]
    g = _gen(M, sorted(BF_FORMS).index(form), VK8.index(vkind), len(kind))
    c = SimpleNamespace(M=M, form=form, kind=kind, b_trans=opt.get("b_trans", False), act=opt.get("act", "none"),
                        alias=opt.get("alias", False), R=opt.get("R", 0), unaligned=opt.get("unaligned", False),
                        a_idx=None, v_idx=None, aux=None, coef=None, V=None)
    c.fg8 = c.R == 8 and not c.unaligned
    NA = M + 5 if opt.get("a_idx") else M
    if kind == "int":
        A, c.B = ints(g, NA, D), ints(g, D, D)
    elif kind == "single":
        A = torch.zeros(NA, D)
        e = torch.arange(NA)
        A[e, e % D] = torch.randn(NA, generator=g)
        c.B = torch.randn(D, D, generator=g)
    else:
        A = torch.rand(NA, D, generator=g)
        c.B = (0.25 + 0.75 * torch.rand(D, D, generator=g)) / 64
    c.A = A.to(BF16)
    if opt.get("a_idx"):
        c.a_idx = torch.randint(0, NA, (M,), generator=g)
        if M > 40:
            c.a_idx[10:30] = 7                              # a run of one repeated row
    if c.act == "dsig":
        aux = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (M, D), generator=g)] if kind == "int" \
            else 0.05 + 0.9 * torch.rand(M, D, generator=g)
        c.aux = aux.to(BF16)
    if c.R:
        c.v_idx, N = v_index8(vkind, M, g)
        if kind == "int":
            c.coef, c.V = ints(g, M, c.R), ints(g, c.R, N, D)
        elif kind == "single":
            c.coef, c.V = torch.zeros(M, c.R), torch.randn(c.R, N, D, generator=g)
        else:
            c.coef, c.V = torch.rand(M, c.R, generator=g), torch.rand(c.R, N, D, generator=g) * 0.25
    return c


def bf_ref(c, w1, drop_k=None):
    """fp64 pre-activation z on the stored operands and the sums of moduli Tg (GEMM products) and Tc (combine terms).
    w1 (IDDGCN_GEMM_BF16): the weights rounded to bf16, and in the R = 8 MFMA forward the coefficients and node rows
    too, as include/iddgcn.h documents; else the fp32 values themselves."""
    A = c.A.double()
    Ar = A[c.a_idx] if c.a_idx is not None else A[:c.M]
    Bw = to_bf16(c.B) if w1 else c.B.double()
    Bm = Bw.t() if c.b_trans else Bw
    if drop_k is not None:
        Ar = Ar.clone()
        Ar[:, drop_k] = 0
    z, Tg = Ar @ Bm, Ar.abs() @ Bm.abs()
    Tc = torch.zeros_like(z)
    if c.R:
        op = to_bf16 if (w1 and c.fg8) else (lambda x: x.double())
        cf, V = op(c.coef), op(c.V)
        for r in range(c.R):
            t = cf[:, r:r + 1] * V[r][c.v_idx]
            z, Tc = z + t, Tc + t.abs()
    return z, Tg, Tc


def bf_bound_z(c, w1, Tg, Tc):
    """Family C bound of the fp32 pre-activation.  Adds on the longest path: one per MFMA product of a k (two with
    hi + lo weights) and, after them, R fused multiply-adds (v3: fp32 VALU, one rounding each) or the combine's MFMA
    products into the SAME accumulators (fwd_gather8: one per term with bf16 operands, three with hi + lo), every add
    at MFMA_ADD; the sigma' epilogue's three roundings.  Representation: REP_HL of the weights' products, REP_COMB of
    the R = 8 combine's; none where the reference takes the operands rounded (w1)."""
    k = 1 if w1 else 2
    n = k * D + ((c.R if w1 else 3 * c.R) if c.fg8 else c.R) + (3 if c.act == "dsig" else 0)
    return gam_e(n, MFMA_ADD) * (Tg + Tc) + (0.0 if w1 else REP_HL) * Tg + (REP_COMB if c.fg8 and not w1 else 0.0) * Tc


def bf_activate(c, z, bz):
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, bz * s
    if c.act == "sig":
        assert float(z.abs().max()) < 8.0, "a saturated pre-activation"
        return sigmoid_bar(z, bz)
    return z, bz


def bf_expect(c, w1, ref=None):
    """(y, b): the fp64 value of the output before its bf16 rounding and the bound on the kernel's fp32 value."""
    z, Tg, Tc = bf_ref(c, w1) if ref is None else ref
    return bf_activate(c, z, bf_bound_z(c, w1, Tg, Tc))


def bf_exact(c):
    """Family A: the exact fp32 value before the rounding (both weight forms: integers are bf16 values, lo = 0)."""
    z, Tg, Tc = bf_ref(c, False)
    assert z.numel() == 0 or float((Tg + Tc).max()) * 3 < LIM, "integer case leaves the exact range of fp32"
    y = bf_activate(c, z, torch.zeros_like(z))[0]
    assert bool((y.float().double() == y).all())
    return y


def bf_single_expect(c, w1):
    """Family B: every element one product a w of a bf16 a and a full-mantissa w.  hi + lo weights: a hi and a lo are
    exact products, one add, and w - hi - lo (HL_SINGLE); bf16 weights against bf16(w): the product is exact.  Then
    the sigma' epilogue's three roundings; the gathered forms carry zero coefficients (fma(0, v, z) = z)."""
    z, Tg, _ = bf_ref(c, w1)
    base = 0.0 if w1 else HL_SINGLE
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, s * Tg * (base * (1 + gam(3)) + gam(3))
    return z, base * Tg


def bf_emul(c, w1, drop_lo=False, drop_hilo=False, pre_rounding=False):
    """The kernel's arithmetic in torch on the CPU: the bf16 piece products summed in fp64, rounded to fp32, the fp32
    epilogue, the bf16 rounding of the output.  drop_lo: the weights' lo piece left out; drop_hilo: the ch vl product
    of the R = 8 combine left out."""
    A = c.A.double()
    Ar = A[c.a_idx] if c.a_idx is not None else A[:c.M]
    hi, lo = hilo(c.B)
    W = hi if (w1 or drop_lo) else hi + lo
    zz = Ar @ (W.t() if c.b_trans else W)
    if c.R and c.fg8:
        ch, cl = hilo(c.coef)
        vh, vl = hilo(c.V)
        for r in range(c.R):
            v_h, v_l = vh[r][c.v_idx], vl[r][c.v_idx]
            zz = zz + ch[:, r:r + 1] * v_h
            if not w1:
                zz = zz + cl[:, r:r + 1] * v_h + (0 if drop_hilo else ch[:, r:r + 1] * v_l)
    z = zz.float()
    if c.R and not c.fg8:
        for r in range(c.R):
            z = (z.double() + c.coef[:, r:r + 1].double() * c.V[r][c.v_idx].double()).float()
    if c.act == "dsig":
        x = c.aux.float()
        z = z * (x * (1.0 - x))
    elif c.act == "sig":
        z = 1.0 / (1.0 + torch.exp(-z))
    return z if pre_rounding else z.to(BF16)


def _bf_row_once(c, dev, precision, what):
    whole, C = guarded(dev, c.M, D, dtype=BF16)
    kw = dict(b_trans=c.b_trans, precision=precision, M=c.M)
    if c.act == "dsig":
        if c.alias:
            C.copy_(c.aux)
        kw.update(act=L.ACT_DSIGMOID, aux=C if c.alias else c.aux.to(dev))
    elif c.act == "sig":
        kw.update(act=L.ACT_SIGMOID)
    if c.R:
        coef = c.coef.to(dev)
        if c.unaligned:
            buf = torch.empty(c.M * c.R + 1, device=dev)[1:].view(c.M, c.R)
            buf.copy_(coef)
            coef = buf
            assert coef.data_ptr() % 16 == 4
        kw.update(coef=coef, V=c.V.to(dev), v_rel_stride=c.V.shape[1] * D, v_idx=c.v_idx.to(I32).to(dev))
    if c.a_idx is not None:
        kw.update(a_idx=c.a_idx.to(I32).to(dev))
    ops.rowgemm(c.A.to(dev), c.B.to(dev), C, **kw)
    out = C.cpu()
    guard_intact(whole, what)
    return out


def run_bf_row(c, dev, precision, what):
    """Two runs into NaN-prefilled bf16 outputs with a guard row: (first, second) as CPU tensors."""
    return _bf_row_once(c, dev, precision, what), _bf_row_once(c, dev, precision, what + " (second run)")


def same_twice(a, b, what):
    assert torch.equal(a, b), f"{what}: the second run differs bitwise"


def _ms(form, big=True):
    if BF_FORMS[form].get("R") == 8 and not BF_FORMS[form].get("unaligned"):
        return FG8_MS + ((FG8_M3,) if big else ())
    return V3_MS + ((V3_M2,) if big else ())


def _vk(form, M):
    if not BF_FORMS[form].get("R"):
        return ("runs13",)
    return VK8 if M <= 785 else ("four",)


PRECS = ("exact", "bf16")              # hi + lo weights; IDDGCN_GEMM_BF16


# ---- family A ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", LINEAR_FORMS)
def test_rowgemm_bf16_exact_integers_bitwise(form, cuda):
    """Family A, every linear form x M x v_idx pattern x weight form: the stored bf16 is BITWISE the round-to-nearest
    of the exact value; the guard row untouched; a second run bitwise the first."""
    for M in _ms(form):
        for vk in _vk(form, M):
            c = bf_case(M, form, "int", vk)
            ref = to_bf16(bf_exact(c))
            for prec in PRECS:
                what = f"rowgemm_bf16[{prec}] {form} int M{M} {vk}"
                a, b = run_bf_row(c, cuda, prec, what)
                assert_bitwise(a.float(), ref, what)
                same_twice(a, b, what)


@gpu
@pytest.mark.parametrize("form", ["gather_R1", "gather_R2", "gather_R8", "gather_R8_v3"])
def test_rowgemm_bf16_gathered_row_addressing(form, cuda):
    """A = 0 and a one-hot coefficient 1.0 in relation r: the output row is bitwise V[r][v_idx[e]] (distinct rows of
    bf16 values: 0 + 1 v survives the output rounding), for every r, every v_idx pattern, ragged and multi-tile M."""
    R = BF_FORMS[form]["R"]
    for M in (65, 785):
        for vk in VK8:
            c = bf_case(M, form, "int", vk)
            c.A = torch.zeros_like(c.A)
            c.V = torch.randn(c.V.shape, generator=_gen(R, M, VK8.index(vk))).to(BF16).float()
            for r in range(R):
                c.coef = torch.zeros(M, R)
                c.coef[:, r] = 1.0
                for prec in PRECS:
                    what = f"rowgemm_bf16[{prec}] {form} one-hot r{r} M{M} {vk}"
                    a, _ = run_bf_row(c, cuda, prec, what)
                    assert_bitwise(a.float(), c.V[r][c.v_idx].double(), what)


# ---- family B ---------------------------------------------------------------------------------------------
SINGLE_FORMS = ("plain", "b_trans", "dsig", "a_idx", "gather_R2", "gather_R8", "gather_R8_v3")


@gpu
@pytest.mark.parametrize("form", SINGLE_FORMS)
def test_rowgemm_bf16_single_term(form, cuda):
    """Family B, M = 2 D + 17: every GEMM element one product of a bf16 a and a full-mantissa weight.  hi + lo: the
    fp32 value within HL_SINGLE |a w| of a w; bf16 weights: exactly a bf16(w); the stored value inside the bf16
    interval of that (a lost lo piece is up to 2^-9 |a w|: 60 bounds)."""
    M = 2 * D + 17
    c = bf_case(M, form, "single", "runs13")
    for prec in PRECS:
        what = f"rowgemm_bf16[{prec}] {form} single M{M}"
        a, b = run_bf_row(c, cuda, prec, what)
        assert_bf16_interval(a, *bf_single_expect(c, prec == "bf16"), what)
        same_twice(a, b, what)


def comb_single_case(form, M, vk):
    """A = 0, one coefficient per row (relation e mod R) and node rows of full-mantissa values: every output element
    is the single product c v of the combine."""
    R = BF_FORMS[form]["R"]
    c = bf_case(M, form, "int", vk)
    g = _gen(R, M, 99)
    c.A = torch.zeros_like(c.A)
    c.V = torch.randn(c.V.shape, generator=g)
    c.coef = torch.zeros(M, R)
    e = torch.arange(M)
    c.coef[e, e % R] = torch.randn(M, generator=g)
    return c


def comb_single_expect(c, w1):
    """fwd_gather8: ch vh + cl vh + ch vl, two adds, the dropped cl vl and the pieces' own error (COMB_SINGLE); bf16
    operands: the exact product of the rounded values; the v3 kernel: one fp32 fused multiply-add, u |c v|."""
    z, _, Tc = bf_ref(c, w1)
    if not c.fg8:
        return z, U * Tc
    return z, (0.0 if w1 else COMB_SINGLE) * Tc


@gpu
@pytest.mark.parametrize("form", ["gather_R8", "gather_R8_v3", "gather_R2"])
def test_rowgemm_bf16_combine_single_term(form, cuda):
    for M, vk in ((785, "runs13"), (65, "random")):
        c = comb_single_case(form, M, vk)
        for prec in PRECS:
            what = f"rowgemm_bf16[{prec}] {form} combine single M{M} {vk}"
            a, _ = run_bf_row(c, cuda, prec, what)
            assert_bf16_interval(a, *comb_single_expect(c, prec == "bf16"), what)


# ---- family C ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", list(BF_FORMS))
def test_rowgemm_bf16_dense_per_element(form, cuda):
    """Family C: positive dense operands; the stored bf16 inside the interval of (gamma_e(n) + rep) T around the fp64
    value, the activation forms with the bound carried through the sigmoid."""
    for M in _ms(form, big=False)[::2] + (_ms(form)[-1],):
        vk = "runs13" if M > 100 else "random"
        if M > 785:
            vk = "four"
        c = bf_case(M, form, "dense", vk)
        for prec in PRECS:
            what = f"rowgemm_bf16[{prec}] {form} dense M{M} {vk}"
            a, b = run_bf_row(c, cuda, prec, what)
            assert_bf16_interval(a, *bf_expect(c, prec == "bf16"), what)
            same_twice(a, b, what)


# ---- CPU self-checks ----------------------------------------------------------------------------------------
def test_selfcheck_hilo_representation():
    """REP_HL: w - hi lies within half a bf16 ulp of w, 2^-8 2^e with 2^e <= |w|, so it is below 2^(e-8), its own bf16
    ulp is at most 2^(e-16) and lo misses it by at most 2^(e-17) <= 2^-17 |w|.  (2^-18 |w| is NOT a bound: random
    weights exceed it.)  REP_COMB likewise, with |cl vl| <= (2^-8 (1 + 2^-8))^2 |c v|."""
    g = _gen(1)
    w = torch.randn(1 << 16, generator=g)
    hi, lo = hilo(w)
    rel = ((w.double() - hi - lo).abs() / w.double().abs()).max()
    assert 2.0 ** -18 < float(rel) <= REP_HL
    c, v = torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g)
    (ch, cl), (vh, vl) = hilo(c), hilo(v)
    cv = c.double() * v.double()
    rel = ((cv - (ch * vh + ch * vl + cl * vh)).abs() / cv.abs()).max()
    assert 2.0 ** -18 < float(rel) <= REP_COMB
    assert 50 * HL_SINGLE < 2.0 ** -11             # an average lost lo piece (~2^-10 |a w|) is 50 bounds out
    print(f"COVER hi + lo: worst |w - hi - lo| / |w| = 2^{float(torch.log2(rel)):.2f} (combine product)")


def test_selfcheck_v_index_patterns():
    g = _gen(2)
    for M in (65, 785):
        for vk, n in (("one", 1), ("four", 4), ("five", 5), ("all", 64), ("random", 64)):
            idx, N = v_index8(vk, M, g)
            assert set(slots_per_tile(idx)[:M // 64]) == {n}, (vk, M)               # every full tile
            assert int(idx.max()) < N and int(idx.min()) >= 0
        idx, _ = v_index8("runs13", M, g)
        assert max(slots_per_tile(idx)) > 16                     # more than four blocks of four slots
        assert not bool((v_index8("random", M, g)[0].sort().values == v_index8("random", M, g)[0]).all())


@pytest.mark.parametrize("form", LINEAR_FORMS)
def test_selfcheck_rowgemm_bf16_integer_reference(form):
    """Family A on the CPU: the emulation (both weight forms) is bitwise the reference; refused: a dropped k term, a
    neighbour's gathered row, the last ragged tile at its sentinel, an output truncated instead of rounded."""
    M = 785
    c = bf_case(M, form, "int", "runs13")
    y = bf_exact(c)
    ref = to_bf16(y)
    for w1 in (False, True):
        assert_bitwise(bf_emul(c, w1).float(), ref, f"cpu emulation {form} int w1={w1}")
    zd = bf_activate(c, bf_ref(c, False, drop_k=D - 1)[0], 0)[0]
    with pytest.raises(AssertionError):
        assert_bitwise(to_bf16(zd).float(), ref, "dropped k")
    cand = ref.clone()
    cand[M - M % 32:] = NAN
    with pytest.raises(AssertionError):
        assert_bitwise(cand.float(), ref, "ragged tile at its sentinel")
    with pytest.raises(AssertionError):
        assert_bitwise(trunc_bf16(y).float(), ref, "truncated output")
    if c.R:
        m = SimpleNamespace(**vars(c))
        m.v_idx = c.v_idx.clone()
        e = M // 2
        m.v_idx[e] += 1 if int(m.v_idx[e]) + 1 < c.V.shape[1] else -1
        with pytest.raises(AssertionError):
            assert_bitwise(to_bf16(bf_exact(m)).float(), ref, "neighbour row")


@pytest.mark.parametrize("w1", [False, True])
@pytest.mark.parametrize("form", list(BF_FORMS))
def test_selfcheck_rowgemm_bf16_dense_bound(form, w1):
    """Family C on the CPU: the emulation inside the bar before and after the output rounding; the bar ambiguous on at
    most 5% of the elements; every mutant refused, with the share of elements it trips printed."""
    M = 145
    c = bf_case(M, form, "dense", "runs13")
    y, b = bf_expect(c, w1)
    lo, hi = bf16_interval(y, b)
    amb = ambiguous_share(lo, hi)
    assert_within(bf_emul(c, w1, pre_rounding=True), y, b, f"cpu emulation {form} dense w1={w1} (fp32)")
    assert assert_bf16_interval(bf_emul(c, w1), y, b, f"cpu emulation {form} dense w1={w1}") <= AMBIGUOUS_MAX
    trip = {}
    mut = to_bf16(bf_activate(c, bf_ref(c, w1, drop_k=7)[0], 0)[0])
    trip["dropped k term"] = share(outside_interval(mut, lo, hi))
    trip["truncated output"] = share(outside_interval(trunc_bf16(bf_emul(c, w1, pre_rounding=True)), lo, hi))
    if not w1:
        trip["lo weight piece dropped"] = share(outside_interval(bf_emul(c, w1, drop_lo=True), lo, hi))
    if c.fg8 and not w1:
        trip["ch vl of the combine dropped"] = share(outside_interval(bf_emul(c, w1, drop_hilo=True), lo, hi))
    if c.R:
        m = SimpleNamespace(**vars(c))
        m.v_idx = c.v_idx.clone()
        e = M // 2
        m.v_idx[e] += 1
        out = outside_interval(to_bf16(bf_expect(m, w1)[0]), lo, hi)
        assert not bool(out[:e].any()) and not bool(out[e + 1:].any())
        trip["neighbour's gathered row (of that row)"] = share(out[e])
    cand = to_bf16(y)
    cand[M - M % 32:] = NAN
    assert rejects_interval(cand, lo, hi)
    print(f"COVER rowgemm_bf16 {form} w1={w1}: ambiguous {100 * amb:.2f}%; " +
          "; ".join(f"{k} trips {100 * v:.0f}%" for k, v in trip.items()))
    for k, v in trip.items():
        assert v > 0, f"{k} passes the bar"


@pytest.mark.parametrize("form", SINGLE_FORMS)
def test_selfcheck_rowgemm_bf16_single_term_bound(form):
    M = 2 * D + 17
    c = bf_case(M, form, "single", "runs13")
    for w1 in (False, True):
        y, b = bf_single_expect(c, w1)
        assert_within(bf_emul(c, w1, pre_rounding=True), y, b, f"cpu emulation {form} single w1={w1} (fp32)")
        assert assert_bf16_interval(bf_emul(c, w1), y, b, f"cpu emulation {form} single w1={w1}") <= AMBIGUOUS_MAX
        lo, hi = bf16_interval(y, b)
        live = y != 0
        if not w1:
            out = outside_interval(bf_emul(c, w1, drop_lo=True), lo, hi)
            pre = ~((bf_emul(c, w1, drop_lo=True, pre_rounding=True).double() - y).abs() <= b)
            print(f"COVER rowgemm_bf16 {form} single: the lo weight piece dropped trips {100 * share(out[live]):.0f}% of "
                  f"the stored elements ({100 * share(pre[live]):.0f}% before the output rounding)")
            assert bool(out.any())
        out = outside_interval(trunc_bf16(bf_emul(c, w1, pre_rounding=True)), lo, hi)
        print(f"COVER rowgemm_bf16 {form} single w1={w1}: a truncated output trips {100 * share(out[live]):.0f}%")
        assert bool(out.any())
        zero_k = SimpleNamespace(**vars(c))
        zero_k.A = c.A.clone()
        zero_k.A[:, 5] = 0
        assert rejects_interval(bf_emul(zero_k, w1), lo, hi)


@pytest.mark.parametrize("form", ["gather_R8", "gather_R8_v3", "gather_R2"])
def test_selfcheck_combine_single_term_bound(form):
    c = comb_single_case(form, 785, "runs13")
    for w1 in (False, True):
        y, b = comb_single_expect(c, w1)
        assert_within(bf_emul(c, w1, pre_rounding=True), y, b, f"cpu emulation {form} combine single w1={w1} (fp32)")
        assert assert_bf16_interval(bf_emul(c, w1), y, b, f"cpu emulation {form} combine single w1={w1}") <= AMBIGUOUS_MAX
        if c.fg8 and not w1:
            lo, hi = bf16_interval(y, b)
            out = outside_interval(bf_emul(c, w1, drop_hilo=True), lo, hi)
            pre = ~((bf_emul(c, w1, drop_hilo=True, pre_rounding=True).double() - y).abs() <= b)
            print(f"COVER fwd_gather8 combine single: ch vl dropped trips {100 * share(out):.0f}% of the stored elements "
                  f"({100 * share(pre):.0f}% before the output rounding)")
            assert share(out) > 0.05


# =============================================================================================================
# gemm_tn256_bf16t_kernel (iddgcn_gemm_tn_bf16) and sigma_tn_bf16_kernel<W1> (iddgcn_sigma_tn_bf16)
# =============================================================================================================
TNB_MS = (1, 15, 16, 17, 31, 32, 33, 785, 4097)
TNB_M2 = 256 * 32 + 33          # 258 tiles over 256 blocks of 64 rows: block 128 holds one full tile and one ragged row
SHORT_MS = (1, 15, 17, 33, 257)


def tnb_case(M, kind, acc, seed=0):
    g = _gen(M, len(kind), int(acc), seed, 41)
    c = SimpleNamespace(M=M, kind=kind, acc=acc)
    if kind == "int":
        A, B, c.C0 = ints(g, M, D), ints(g, M, D), ints(g, D, D)
    elif kind == "single":
        c.pi = spread_rows(M, D)
        A = torch.zeros(M, D)
        A[c.pi, torch.arange(D)] = torch.randn(D, generator=g)
        B, c.C0 = torch.randn(M, D, generator=g), torch.randn(D, D, generator=g)
    else:
        A, B, c.C0 = torch.rand(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(D, D, generator=g)
    c.A, c.B = A.to(BF16), B.to(BF16)
    return c


def tnb_ref(c, drop_row=None):
    A, B = c.A.double(), c.B.double()
    if drop_row is not None:
        A = A.clone()
        A[drop_row] = 0
    z, T = A.t() @ B, A.abs().t() @ B.abs()
    if c.acc:
        z, T = z + c.C0.double(), T + c.C0.double().abs()
    return z, T


def tnb_bound(c, T, n_partials):
    """bf16 x bf16 products are exact in fp32: M adds inside the MFMAs, the slab partials, the accumulated C."""
    return gam_e(c.M + n_partials + int(c.acc), MFMA_ADD) * T


def run_tnb(c, dev, what):
    outs = []
    for _ in range(2):
        slab = torch.full((ops.tn_blocks(c.M, D) * D * D,), NAN, device=dev)
        whole, C = guarded(dev, D, D)
        if c.acc:
            C.copy_(c.C0)
        ops.gemm_tn(c.A.to(dev), c.B.to(dev), C, slab, accumulate=c.acc)
        outs.append(C.cpu())
        guard_intact(whole, what)
    return outs


@gpu
@pytest.mark.parametrize("acc", [False, True])
def test_gemm_tn_bf16_exact_integers_bitwise(acc, cuda):
    """Family A: random integers in every row of A and B (a swapped or misplaced row changes the sum): bitwise, from
    a NaN-filled slab into a NaN-guarded C, M around the 16- and 32-row tiles, several blocks, a second tile per
    block with a ragged row after a full tile and blocks without rows; twice."""
    assert ops.tn_blocks(TNB_M2, D) == 256
    for M in TNB_MS + (TNB_M2,):
        c = tnb_case(M, "int", acc)
        z, T = tnb_ref(c)
        assert float(T.max()) < LIM
        what = f"gemm_tn_bf16 int M{M} acc{int(acc)}"
        a, b = run_tnb(c, cuda, what)
        assert_bitwise(a, z, what)
        same_twice(a, b, what)


@gpu
@pytest.mark.parametrize("acc", [False, True])
def test_gemm_tn_bf16_single_term(acc, cuda):
    """Family B: column i of A non-zero only in row pi(i): C[i][j] = A[pi(i)][i] B[pi(i)][j], an exact product of
    two bf16 values and exact zeros: bitwise without accumulate, one rounding of the accumulated C with it."""
    for M in (785, 4097, TNB_M2):
        c = tnb_case(M, "single", acc)
        z, T = tnb_ref(c)
        what = f"gemm_tn_bf16 single M{M} acc{int(acc)}"
        a, _ = run_tnb(c, cuda, what)
        assert_within(a, z, U * T if acc else torch.zeros_like(T), what)


@gpu
@pytest.mark.parametrize("acc", [False, True])
def test_gemm_tn_bf16_dense_per_element(acc, cuda):
    for M in SHORT_MS:
        c = tnb_case(M, "dense", acc)
        z, T = tnb_ref(c)
        what = f"gemm_tn_bf16 dense M{M} acc{int(acc)}"
        a, b = run_tnb(c, cuda, what)
        assert_within(a, z, tnb_bound(c, T, ops.tn_blocks(M, D)), what)
        same_twice(a, b, what)


def test_selfcheck_tn_bf16_bounds():
    for M in (1, 17, 257):
        ci = tnb_case(M, "int", True)
        assert_bitwise(ci.A.float().t() @ ci.B.float() + ci.C0, tnb_ref(ci)[0], f"cpu-fp32 tn_bf16 int M{M}")
        c = tnb_case(M, "dense", True)
        z, T = tnb_ref(c)
        bound = tnb_bound(c, T, (M + 31) // 32)
        assert_within(c.A.float().t() @ c.B.float() + c.C0, z, bound, f"cpu-fp32 tn_bf16 dense M{M}")
        out = (tnb_ref(c, drop_row=M - 1)[0] - z).abs() > bound
        print(f"COVER tn_bf16 dense M{M}: the last row dropped trips {100 * share(out):.0f}% of the elements")
        assert bool(out.any())
    with pytest.raises(AssertionError):
        assert_bitwise(tnb_ref(ci, drop_row=256)[0].float(), tnb_ref(ci)[0], "dropped row")
    c = tnb_case(785, "single", False)
    z, T = tnb_ref(c)
    assert bool(((c.A != 0).sum(0) == 1).all()) and int(c.pi[-1]) == 784
    assert_bitwise((c.A.float().t() @ c.B.float()), z, "cpu-fp32 tn_bf16 single")
    assert rejects(tnb_ref(c, drop_row=784)[0], z, torch.zeros_like(T))


def stnb_case(M, kind):
    """int: family A; dense: positive operands (family C, the dx interval a single value almost everywhere); single:
    X column i non-zero only in row pi(i) (dS one product); single_dx: dO row e non-zero only in column e mod D (dx
    one product)."""
    g = _gen(M, len(kind), 53)
    c = SimpleNamespace(M=M, kind=kind)
    if kind == "int":
        X = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (M, D), generator=g)]
        dO, c.S = ints(g, M, D), ints(g, D, D)
    else:
        X = 0.05 + 0.9 * torch.rand(M, D, generator=g)
        dO = torch.rand(M, D, generator=g)
        c.S = (0.25 + 0.75 * torch.rand(D, D, generator=g)) / 64
        if kind == "single":
            c.pi = spread_rows(M, D)
            keep = torch.zeros(M, D, dtype=torch.bool)
            keep[c.pi, torch.arange(D)] = True
            X = torch.where(keep, X, torch.zeros(()))
            dO = torch.randn(M, D, generator=g)
        elif kind == "single_dx":
            e = torch.arange(M)
            dO = torch.zeros(M, D)
            dO[e, e % D] = torch.randn(M, generator=g)
            c.S = torch.randn(D, D, generator=g)
    c.X, c.dO = X.to(BF16), dO.to(BF16)
    return c


def stnb_ref(c, w1, drop_row=None):
    """dS = X^T dO and dX = (dO S^T) x (1 - x) in fp64 on the stored tables, with the sums of moduli of their terms;
    the weights rounded to bf16 for w1."""
    X, dO = c.X.double(), c.dO.double()
    if drop_row is not None:
        dO = dO.clone()
        dO[drop_row] = 0
    S = to_bf16(c.S) if w1 else c.S.double()
    s = X * (1 - X)
    return {"dS": (X.t() @ dO, X.abs().t() @ dO.abs()), "dX": ((dO @ S.t()) * s, (dO.abs() @ S.abs().t()) * s)}


def stnb_bounds(c, refs, w1, n_ranges):
    """dS: exact products, M adds and the range partials.  dX: the sigma' row form's bound (k D adds + 3, REP_HL);
    single_dx: the one-product bound with the epilogue's three roundings."""
    bS = gam_e(c.M + n_ranges, MFMA_ADD) * refs["dS"][1]
    if c.kind == "single":
        bS = torch.zeros_like(bS)
    TX = refs["dX"][1]
    if c.kind == "single_dx":
        base = 0.0 if w1 else HL_SINGLE
        bX = TX * (base * (1 + gam(3)) + gam(3))
    else:
        bX = (gam_e((1 if w1 else 2) * D + 3, MFMA_ADD) + (0.0 if w1 else REP_HL)) * TX
    return bS, bX


def stnb_emul(c, w1, drop_lo=False):
    hi, lo = hilo(c.S)
    W = hi if (w1 or drop_lo) else hi + lo
    x = c.X.float()
    dS = (c.X.double().t() @ c.dO.double()).float()
    dX = (c.dO.double() @ W.t()).float() * (x * (1.0 - x))
    return dS, dX


def run_stnb(c, dev, precision, what):
    outs = []
    for _ in range(2):
        nfl = ops.sigma_tn_slab_floats(c.M)
        slab = torch.full((nfl,), NAN, device=dev)
        wS, dS = guarded(dev, D, D)
        wX, X = guarded(dev, c.M, D, dtype=BF16)
        X.copy_(c.X)
        ops.sigma_tn(c.dO.to(dev), X, c.S.to(dev), dS, slab, precision=precision)
        outs.append({"dS": dS.cpu(), "dX": X.cpu()})
        guard_intact(wS, what + " dS")
        guard_intact(wX, what + " dX")
    return outs[0], outs[1], nfl // (D * D)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_sigma_tn_bf16_exact_integers_bitwise(prec, cuda):
    """Family A: dS and the in-place dx both bitwise from NaN-filled slab and dS; M = 0 gives dS = 0; at 4097 rows two
    tiles per range and ranges past the table; dx also bitwise the row GEMM's sigma' output; twice."""
    for M in (0, 1, 31, 32, 33, 785, 4097):
        c = stnb_case(M, "int")
        refs = stnb_ref(c, False)
        assert float(refs["dS"][1].max() if M else 0) < LIM and float(refs["dX"][1].max() if M else 0) * 16 < LIM
        what = f"sigma_tn_bf16[{prec}] int M{M}"
        a, b, _ = run_stnb(c, cuda, prec, what)
        assert_bitwise(a["dS"], refs["dS"][0], what + " dS")
        assert_bitwise(a["dX"].float(), to_bf16(refs["dX"][0]), what + " dX")
        same_twice(a["dS"], b["dS"], what + " dS")
        same_twice(a["dX"], b["dX"], what + " dX")
        if M:
            C = torch.full((M, D), NAN, dtype=BF16, device=cuda)
            ops.rowgemm(c.dO.to(cuda), c.S.to(cuda), C, b_trans=True, act=L.ACT_DSIGMOID, aux=c.X.to(cuda), precision=prec)
            assert torch.equal(C.cpu(), a["dX"]), what + ": dx differs from the row GEMM's sigma' output"


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_sigma_tn_bf16_single_term_and_dense(prec, cuda):
    """Family B (dS: exact single products, bitwise; dx: one product per element) at long M, family C at short M."""
    w1 = prec == "bf16"
    for kind, Ms in (("single", (785, 4097)), ("single_dx", (785, 4097)), ("dense", SHORT_MS)):
        for M in Ms:
            c = stnb_case(M, kind)
            refs = stnb_ref(c, w1)
            what = f"sigma_tn_bf16[{prec}] {kind} M{M}"
            a, b, nr = run_stnb(c, cuda, prec, what)
            bS, bX = stnb_bounds(c, refs, w1, nr)
            assert_within(a["dS"], refs["dS"][0], bS, what + " dS")
            assert_bf16_interval(a["dX"], refs["dX"][0], bX, what + " dX")
            same_twice(a["dS"], b["dS"], what + " dS")
            same_twice(a["dX"], b["dX"], what + " dX")


def test_selfcheck_sigma_tn_bf16_bounds():
    for w1 in (False, True):
        for M in (1, 33, 257):
            ci = stnb_case(M, "int")
            ri = stnb_ref(ci, w1)
            eS, eX = stnb_emul(ci, w1)
            assert_bitwise(eS, ri["dS"][0], "cpu emulation sigma_tn_bf16 int dS")
            assert_bitwise(eX.to(BF16).float(), to_bf16(ri["dX"][0]), "cpu emulation sigma_tn_bf16 int dX")
            c = stnb_case(M, "dense")
            refs = stnb_ref(c, w1)
            bS, bX = stnb_bounds(c, refs, w1, 8)
            eS, eX = stnb_emul(c, w1)
            assert_within(eS, refs["dS"][0], bS, "cpu emulation sigma_tn_bf16 dS")
            assert_within(eX, refs["dX"][0], bX, "cpu emulation sigma_tn_bf16 dX (fp32)")
            assert assert_bf16_interval(eX.to(BF16), refs["dX"][0], bX, f"cpu emulation sigma_tn_bf16 dX w1={w1} M{M}") \
                <= AMBIGUOUS_MAX
            lo, hi = bf16_interval(refs["dX"][0], bX)
            mut = stnb_ref(c, w1, drop_row=M - 1)
            assert rejects(mut["dS"][0], refs["dS"][0], bS) and rejects_interval(to_bf16(mut["dX"][0]), lo, hi)
            assert rejects_interval(trunc_bf16(eX), lo, hi)
            if not w1:
                out = outside_interval(stnb_emul(c, w1, drop_lo=True)[1].to(BF16), lo, hi)
                print(f"COVER sigma_tn_bf16 dense M{M}: the lo weight piece dropped trips {100 * share(out):.0f}% of dx")
                assert bool(out.any())
        c = stnb_case(785, "single_dx")
        refs = stnb_ref(c, w1)
        bS, bX = stnb_bounds(c, refs, w1, 8)
        eS, eX = stnb_emul(c, w1)
        assert_within(eX, refs["dX"][0], bX, "cpu emulation sigma_tn_bf16 single dX (fp32)")
        assert assert_bf16_interval(eX.to(BF16), refs["dX"][0], bX, f"cpu emulation sigma_tn_bf16 single dX w1={w1}") \
            <= AMBIGUOUS_MAX
        c = stnb_case(785, "single")
        refs = stnb_ref(c, w1)
        assert bool(((c.X != 0).sum(0) == 1).all())
        assert_bitwise(stnb_emul(c, w1)[0], refs["dS"][0], "cpu emulation sigma_tn_bf16 single dS")


# =============================================================================================================
# tail_seg_mfma8_kernel<DSUM, HEAD> (iddgcn_tail_seg_reduce_bf16 at R = 8 with per-edge W; _head_bf16)
# =============================================================================================================
TSM_GRAPHS = {"edges": [0, 0, 1, 31, 32, 33, 65, 0, 200, 2, 0, 0],       # empty leading / trailing nodes, a hub
              "n1": [33], "n1_empty": [0], "n3": [1, 0, 40], "n4": [32, 0, 65, 1], "n5": [0, 31, 0, 0, 7]}


def tsm_case(graph, kind):
    """Segment lengths per node (four nodes per workgroup); W per edge (T x 8), dO bf16, P, head_dO, Wn fp32.
    single: dO row e non-zero only in column e mod D, so every dWedge element is one product, and every dP element
    one product at segment lengths up to D."""
    lens = torch.tensor(TSM_GRAPHS[graph])
    N, T, R = len(lens), int(lens.sum()), 8
    g = _gen(sorted(TSM_GRAPHS).index(graph), len(kind), 67)
    c = SimpleNamespace(N=N, T=T, R=R, lens=lens, kind=kind, t=torch.repeat_interleave(torch.arange(N), lens))
    c.ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(I32)
    if kind == "int":
        c.W, dO, c.P, c.hd, c.Wn = ints(g, T, R), ints(g, T, D), ints(g, R, N, D), ints(g, N, D), ints(g, N, R)
    else:
        c.W, c.P = torch.rand(T, R, generator=g), torch.randn(R, N, D, generator=g)
        c.hd, c.Wn = torch.randn(N, D, generator=g), torch.rand(N, R, generator=g)
        dO = torch.randn(T, D, generator=g)
        if kind == "single":
            e = torch.arange(T)
            keep = torch.zeros(T, D, dtype=torch.bool)
            keep[e, e % D] = True
            dO = torch.where(keep, dO, torch.zeros(()))
            n = torch.arange(N)
            keep = torch.zeros(N, D, dtype=torch.bool)
            keep[n, (7 * n + 3) % D] = True                  # head_dO likewise: dwh one term (nine piece products)
            c.hd = torch.where(keep, c.hd, torch.zeros(()))
    c.dO = dO.to(BF16)
    return c


def tsm_ref(c, head, drop_edge=None):
    """fp64 index_add references on the stored rows: name -> (reference, bound).  W, P and head_dO enter as EXACT
    three-piece bf16 splits (no representation term): three products per NON-ZERO term of dP and dWedge (an exact
    zero adds nothing; + the DPP add of dWedge's two columns), nine of dwh (+ 3), one of dsum (the ones row), every
    add at MFMA_ADD; HEAD adds one fused multiply-add (dP) or add (dsum).  A single-term element so has n = 3."""
    N, R = c.N, c.R
    d, W, P = c.dO.double(), c.W.double(), c.P.double()
    if drop_edge is not None:
        d = d.clone()
        d[drop_edge] = 0
    h = int(head)
    out = {}
    wd = W.t()[:, :, None] * d[None]                                           # (R, T, D)
    dP = torch.zeros(R, N, D, dtype=F64).index_add_(1, c.t, wd)
    TP = torch.zeros(R, N, D, dtype=F64).index_add_(1, c.t, wd.abs())
    nP = torch.zeros(R, N, D, dtype=F64).index_add_(1, c.t, (wd != 0).double())     # the element's non-zero terms
    ds = torch.zeros(N, D, dtype=F64).index_add_(0, c.t, d)
    Ts = torch.zeros(N, D, dtype=F64).index_add_(0, c.t, d.abs())
    ns = torch.zeros(N, D, dtype=F64).index_add_(0, c.t, (d != 0).double())
    if head:
        hw = c.Wn.double().t()[:, :, None] * c.hd.double()[None]
        dP, TP = dP + hw, TP + hw.abs()
        ds, Ts = ds + c.hd.double(), Ts + c.hd.double().abs()
        q = c.hd.double()[None] * P
        out["dwh"] = (q.sum(2).t(), gam_e(9 * (q != 0).double().sum(2).t() + 3, MFMA_ADD) * q.abs().sum(2).t())
    out["dP"] = (dP, gam_e(3 * nP + h, MFMA_ADD) * TP)
    out["dsum"] = (ds, gam_e(ns + h, MFMA_ADD) * Ts)
    q = d[None] * P[:, c.t]                                                    # (R, T, D)
    nW = (q != 0).double().sum(2).t()
    out["dWedge"] = (q.sum(2).t(), gam_e(3 * nW + 1, MFMA_ADD) * q.abs().sum(2).t())
    return out


def tsm_emul(c, head, drop_piece=None):
    """split3 of W, P, head_dO by .to(bfloat16), the piece products summed in fp64, rounded to fp32.  drop_piece: one
    of the three pieces of W (dP) and of P (dWedge, dwh) left out."""
    def pieces(x):
        p = G.split3(x)
        return sum(q for k, q in enumerate(p) if k != drop_piece)
    d, W, P, hd = c.dO.double(), pieces(c.W), pieces(c.P), sum(G.split3(c.hd))
    wd = W.t()[:, :, None] * d[None]
    dP = torch.zeros(c.R, c.N, D, dtype=F64).index_add_(1, c.t, wd)
    ds = torch.zeros(c.N, D, dtype=F64).index_add_(0, c.t, d)
    out = {"dWedge": (d[None] * P[:, c.t]).sum(2).t().float()}
    if head:
        dP = (dP.float().double() + c.Wn.double().t()[:, :, None] * c.hd.double()[None])
        ds = ds.float().double() + c.hd.double()
        out["dwh"] = (hd[None] * P).sum(2).t().float()
    out["dP"], out["dsum"] = dP.float(), ds.float()
    return out


def run_tsm(c, dev, head, dsum):
    """One launch on row-range views [2, 2 + N) of larger NaN-filled P / dP tables; every output NaN-prefilled and
    guarded; returns CPU copies."""
    N, T, R = c.N, c.T, c.R
    Pb = torch.full((R, N + 3, D), NAN, device=dev)
    Pb[:, 2:2 + N] = c.P.to(dev)
    dPb = torch.full((R, N + 3, D), NAN, device=dev)
    wW, dWe = guarded(dev, T, R)
    wS, ds = guarded(dev, N, D)
    wH, dwh = guarded(dev, N, R)
    # one unused trailing row of 1e30 on W and dO: a graph without edges still passes non-null tables, and a read past
    # the last segment cannot stay inside any bar
    W1 = torch.cat([c.W, torch.full((1, R), 1e30)]).to(dev)
    dO1 = torch.cat([c.dO, torch.full((1, D), 1e30, dtype=BF16)]).to(dev)
    args = (c.ptr.to(dev), W1, dO1, Pb[:, 2:2 + N], dPb[:, 2:2 + N], dWe if T else wW)      # (T = 0: a non-null dWedge)
    if head:
        ops.tail_seg_reduce_head(*args, c.hd.to(dev), c.Wn.to(dev), dwh, dsum=ds if dsum else None)
    else:
        ops.tail_seg_reduce(args[0], None, *args[1:], dsum=ds if dsum else None)
    assert bool(torch.isnan(dPb[:, :2]).all()) and bool(torch.isnan(dPb[:, 2 + N:]).all()), "dP rows outside the view"
    guard_intact(wW, "dWedge")
    assert bool(torch.isnan(wS[-1] if dsum else wS).all()) and bool(torch.isnan(wH[-1] if head else wH).all())
    out = {"dP": dPb[:, 2:2 + N].cpu(), "dWedge": dWe.cpu()}
    if dsum:
        out["dsum"] = ds.cpu()
    if head:
        out["dwh"] = dwh.cpu()
    return out


def _tsm_names(head, dsum):
    return ("dP", "dWedge") + (("dsum",) if dsum else ()) + (("dwh",) if head else ())


@gpu
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("dsum", [False, True])
@pytest.mark.parametrize("graph", list(TSM_GRAPHS))
def test_tail_seg_mfma8_exact_integers_bitwise(graph, dsum, head, cuda):
    """Family A: dP, dWedge, dsum and dwh bitwise the fp64 index_add on the same bf16 rows; twice."""
    c = tsm_case(graph, "int")
    refs = tsm_ref(c, head)
    what = f"tail_seg_mfma8<dsum={dsum}, head={head}> {graph} int"
    a, b = run_tsm(c, cuda, head, dsum), run_tsm(c, cuda, head, dsum)
    for k in _tsm_names(head, dsum):
        assert_bitwise(a[k], refs[k][0], f"{what} {k}")
        same_twice(a[k], b[k], f"{what} {k}")


@gpu
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("kind", ["single", "dense"])
@pytest.mark.parametrize("graph", ["edges", "n1", "n5"])
def test_tail_seg_mfma8_per_element(graph, kind, head, cuda):
    """Families B and C against fp64 directly (the HEAD form too, not via the unfused pair), then head_dz on the
    kernel's own dWedge and dwh at the step-kernel module's bar."""
    c = tsm_case(graph, kind)
    refs = tsm_ref(c, head)
    what = f"tail_seg_mfma8<head={head}> {graph} {kind}"
    a = run_tsm(c, cuda, head, True)
    for k in _tsm_names(head, True):
        assert_within(a[k], *refs[k], f"{what} {k}")
    if head and c.T:
        g = _gen(c.N, c.T, 71)
        h = torch.randint(0, c.N, (c.T,), generator=g)
        hperm = torch.argsort(h, stable=True)
        node_k = h[hperm].contiguous()
        S = torch.softmax(torch.randn(c.N, c.R, generator=g), -1)
        i = dict(n=c.N, T=c.T, R=c.R, D=D, hperm=hperm, node_k=node_k, S=S, Wn=torch.sigmoid(S), dWedge=a["dWedge"],
                 dwh=a["dwh"], hptr=torch.searchsorted(node_k, torch.arange(c.N + 1), right=False).to(I32))
        w, dz = guarded(cuda, c.N, c.R)
        ops.head_dz(S.to(cuda), i["Wn"].to(cuda), i["hptr"].to(cuda), hperm.to(I32).to(cuda), a["dWedge"].to(cuda),
                    a["dwh"].to(cuda), dz)
        guard_intact(w, "head_dz")
        assert_within(dz, *K.head_dz_ref(i)["dz"], what + " head_dz")


def test_selfcheck_tail_seg_mfma8_bounds():
    for head in (False, True):
        ci = tsm_case("edges", "int")
        ri, ei = tsm_ref(ci, head), tsm_emul(ci, head)
        for k in _tsm_names(head, True):
            assert float(ri[k][0].abs().max()) < LIM
            assert_bitwise(ei[k], ri[k][0], f"cpu emulation tail_seg_mfma8 int {k}")
        for kind in ("single", "dense"):
            c = tsm_case("edges", kind)
            refs, em = tsm_ref(c, head), tsm_emul(c, head)
            for k in _tsm_names(head, True):
                assert_within(em[k], *refs[k], f"cpu emulation tail_seg_mfma8 {kind} head={head} {k}")
            for piece in (0, 1, 2):
                mut = tsm_emul(c, head, drop_piece=piece)
                for k in ("dP", "dWedge") + (("dwh",) if head else ()):
                    out = (mut[k].double() - refs[k][0]).abs() > refs[k][1]
                    live = refs[k][1] > 0
                    print(f"COVER tail_seg_mfma8 {kind} head={head}: piece {piece} of the split operand dropped trips "
                          f"{100 * share(out[live]):.0f}% of {k}")
                    # the third piece (<= 2^-16 of a term) is family B's to see: 256 dense terms hide it
                    assert bool(out.any()) or (kind == "dense" and piece == 2), (kind, piece, k)
            last = int(c.ptr[7]) - 1                          # the last edge of the 65-edge segment: its ragged chunk
            mut = tsm_ref(c, head, drop_edge=last)
            for k in ("dP", "dsum", "dWedge"):
                assert rejects(mut[k][0], *refs[k]), k


# =============================================================================================================
# The VALU bf16 forms: iddgcn_tail_seg_reduce_bf16 (R < 8, or h_idx), iddgcn_combine_bf16, iddgcn_distmult_bce(_heads)_bf16
# =============================================================================================================
@gpu
@pytest.mark.parametrize("R,h_idx,case",
                         [(R, h, case) for case in K.GRAPHS
                          for R, h in [(1, False), (2, False), (4, True), (7, False), (8, True)]] +
                         [(3, True, "tiny"), (5, False, "tiny"), (6, True, "tiny")])
def test_tail_seg_reduce_bf16_valu_vs_fp64(R, h_idx, case, cuda):
    """tail_seg_reduce_kernel<256, R, BF>, every R = 1 .. 8: the step-kernel module's bound builder fed the widened
    bf16 rows; with and without dsum, twice."""
    N, T, t, ptr, h, W, dO, P = K.tail_inputs(case, R, D, 13 * R + len(case))
    dO = dO.to(BF16)
    if not h_idx:
        W, h = W[h], None
    refs = K.tail_ref(N, t, ptr, h, W, dO.float(), P)
    what = f"tail_seg_reduce_bf16 {case} R{R} h_idx={h_idx}"
    a = K.run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=True)
    K.check_all(a, refs, what)
    K._same(a, K.run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=True), ("dP", "dsum", "dWedge"), what + " run twice")
    K._same(a, K.run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=False), ("dP", "dWedge"), what + " without dsum")


@gpu
@pytest.mark.parametrize("R", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_combine_bf16_per_element(R, cuda):
    """iddgcn_combine_bf16 (the run form writing bf16): the fp64 sigmoid with the combine bound of test_gpu_mfma_gemms
    carried through it, then the bf16 interval."""
    for M in (1, 63, 65, 785):
        c = G.comb_case(D, M, R, "run")
        whole, out = guarded(cuda, M, D, dtype=BF16)
        idx = c.y_idx.to(I32).to(cuda)
        ops.combine(c.Y.to(cuda), c.coef.to(cuda), c.V.to(cuda), out, y_idx=idx, v_idx=idx)
        what = f"combine_bf16 R{R} M{M}"
        guard_intact(whole, what)
        assert_bf16_interval(out, *G.comb_ref(c), what)


def test_selfcheck_combine_bf16_bound():
    for R in (0, 2, 8):
        c = G.comb_case(D, 65, R, "run")
        ref, bound = G.comb_ref(c)
        z = c.Y[c.y_idx]
        for r in range(R):
            z = z + c.coef[:, r:r + 1] * c.V[r][c.v_idx]
        y32 = 1.0 / (1.0 + torch.exp(-z))
        assert assert_bf16_interval(y32.to(BF16), ref, bound, f"cpu-fp32 combine_bf16 R{R}") <= AMBIGUOUS_MAX
        lo, hi = bf16_interval(ref, bound)
        assert rejects_interval(trunc_bf16(y32), lo, hi)
        m = SimpleNamespace(**vars(c))
        m.y_idx = c.y_idx.clone()
        m.y_idx[7] = (m.y_idx[7] + 1) % c.N
        assert rejects_interval(to_bf16(G.comb_ref(m)[0]), lo, hi)


def dm_bf_case(R, T):
    """The step-kernel module's DistMult case (heads, relations, scale) with inputs scaled for the bf16 bar: every
    relation row of ONE sign (even relations positive, odd negative), so a logit's terms do not cancel, |s| ~ 1.25 and
    the relative bound of ds and do stays near gamma(D) |s| ~ 2e-5 (the do interval a single bf16 value on ~99% of
    the elements; with the module's mixed-sign rel it is ambiguous on 7% / 18%).  Every 20th edge saturated (|s| in
    [22, 32], both labels, both signs through the relation), as there.  The tail rows are the values the bf16 table
    stores, widened back to fp32 for the reference builder."""
    c = K.dm_case(D, R, T)
    g = _gen(R, T, 83)
    sign = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0)
    c.rel = sign[:, None] * (0.25 + 0.75 * torch.rand(R, D, generator=g)) / 32
    Xt = 0.05 + 0.9 * torch.rand(T, D, generator=g)
    s = (c.Xh.double()[c.h] * c.rel.double()[c.r] * Xt.double()).sum(1)
    want = torch.arange(T) % 20 == 7
    k = torch.cumsum(want.long(), 0) - 1
    c.y = torch.where(want, (k % 2).float(), (torch.rand(T, generator=g) < 0.5).float())
    fac = torch.where(want, (22.0 + 10.0 * torch.rand(T, generator=g, dtype=F64)) / s.abs(), torch.ones_like(s))
    c.Xt = (Xt.double() * fac[:, None]).float().to(BF16).float()
    c.want_sat = want
    return c


def run_dm_bf(c, dev, heads, train=True, in_place=False):
    T, R, N = c.T, c.R, c.N
    d = K._dm_dev(c, dev)
    nb = ops.distmult_blocks(T)
    wholes, bufs = {}, {}
    for k, shape in (("p", (T,)), ("s", (T,)), ("ds", (T,)), ("dXh", (N, D)), ("drel_slab", (nb * R * D,)),
                     ("loss_slab", (nb,))):
        wholes[k], bufs[k] = guarded(dev, *shape)
    wholes["do"], bufs["do"] = guarded(dev, T, D, dtype=BF16)
    Xt = d.Xt.to(BF16)
    if in_place:
        bufs["do"].copy_(Xt)
        Xt = bufs["do"]
    if heads:
        ops.distmult_bce_heads(d.hptr, d.hperm, d.Xh, Xt, d.r, d.rel, d.y if train else None, bufs["do"], bufs["dXh"],
                               bufs["drel_slab"], bufs["loss_slab"], scale=c.scale, p_out=bufs["p"], s_out=bufs["s"],
                               ds_out=bufs["ds"])
    else:
        wholes.pop("dXh"), bufs.pop("dXh")
        ops.distmult_bce(d.Xh, d.h, Xt, d.r, d.rel, y=d.y, scale=c.scale, p_out=bufs["p"], s_out=bufs["s"],
                         ds_out=bufs["ds"], do_out=bufs["do"], drel_slab=bufs["drel_slab"], loss_slab=bufs["loss_slab"])
    return K._dm_collect(c, nb, bufs, wholes, "distmult_bf16")


def check_dm_bf(got, refs, what, names):
    for k in names:
        if k == "do":
            assert_bf16_interval(got[k], refs[k][0], refs[k][1], f"{what} do")
        else:
            assert_within(got[k], refs[k][0], refs[k][1], f"{what} {k}")


DM_BF_RAW = ("p", "s", "ds", "do", "drel_slab", "loss_slab")


@gpu
@pytest.mark.parametrize("R,T", [(R, T) for T in (1, 255, 257, 3001) for R in (2, 8)] + [(1, 257), (4, 257)])
def test_distmult_bf16_training_vs_fp64(R, T, cuda):
    """iddgcn_distmult_bce_bf16 and _heads_bf16, training seed: s, p, ds, drel, the loss and dXh per element at the
    step-kernel module's bounds, the bf16 do inside its interval, do_out aliasing Xt and not; twice.  R = 1, 2, 4, 8
    are the four relation-slot instantiations of distmult_heads_kernel<256, RT, BF>."""
    c = dm_bf_case(R, T)
    refs = K.dm_ref(c, True)
    what = f"distmult_bf16 R{R} T{T}"
    plain = run_dm_bf(c, cuda, heads=False)
    check_dm_bf(plain, refs, what + " plain", ("s", "p", "ds", "do", "drel", "loss"))
    K._same(plain, run_dm_bf(c, cuda, heads=False), DM_BF_RAW, what + " plain run twice")
    heads = run_dm_bf(c, cuda, heads=True)
    check_dm_bf(heads, refs, what + " heads", K.DM_NAMES)
    K._same(heads, run_dm_bf(c, cuda, heads=True), DM_BF_RAW + ("dXh",), what + " heads run twice")
    inpl = run_dm_bf(c, cuda, heads=True, in_place=True)
    check_dm_bf(inpl, refs, what + " heads in place", K.DM_NAMES)
    K._same(heads, inpl, DM_BF_RAW + ("dXh",), what + " heads in place vs not")
    sat = refs["sat"]
    assert bool((heads["ds"][sat] == 0).all()) and bool((heads["do"][sat] == 0).all())


@gpu
@pytest.mark.parametrize("T", [257, 3001])
@pytest.mark.parametrize("R", [2, 8])
def test_distmult_heads_bf16_prediction_seed_vs_fp64(R, T, cuda):
    c = dm_bf_case(R, T)
    refs = K.dm_ref(c, False)
    what = f"distmult_heads_bf16(pred) R{R} T{T}"
    a = run_dm_bf(c, cuda, heads=True, train=False)
    check_dm_bf(a, refs, what, K.DM_NAMES)
    b = run_dm_bf(c, cuda, heads=True, train=False, in_place=True)
    check_dm_bf(b, refs, what + " in place", K.DM_NAMES)
    K._same(a, b, DM_BF_RAW + ("dXh",), what + " in place vs not")


@pytest.mark.parametrize("train", [True, False])
def test_selfcheck_distmult_bf16_bounds(train):
    """The fp32 emulation on the widened bf16 rows inside every bar; the do interval ambiguous on at most 5%; a
    truncated do and one dropped block of edges refused."""
    c = dm_bf_case(2, 255)
    refs = K.dm_ref(c, train)
    em = K.dm_emul32(c, train)
    K.check_all(em, refs, f"cpu-fp32 distmult on bf16 rows train{train}", K.DM_NAMES)
    amb = assert_bf16_interval(em["do"].to(BF16), refs["do"][0], refs["do"][1], f"cpu-fp32 distmult_bf16 do train{train}")
    assert amb <= AMBIGUOUS_MAX
    lo, hi = bf16_interval(*refs["do"])
    out = outside_interval(trunc_bf16(em["do"]), lo, hi)
    print(f"COVER distmult_bf16 do train{train}: a truncated output trips {100 * share(out):.0f}% of the elements")
    assert bool(out.any())
    dropped = K.dm_ref(c, train, omit=K._last_block(c.T))
    assert rejects_interval(to_bf16(dropped["do"][0]), lo, hi)


# =============================================================================================================
# The precision strings on the bf16 entry points, and row_gemm = "exact4" on bf16 features
# =============================================================================================================
ALL_PRECS = ("exact", "split", "exact4", "bf16x3", "bf16")


@gpu
def test_bf16_entry_points_precision_matrix(cuda):
    """include/iddgcn.h: iddgcn_rowgemm_bf16 takes every precision (IDDGCN_GEMM_BF16: bf16 weights; any other: the
    hi + lo pair, so all of those are bitwise one another); iddgcn_sigma_tn_bf16 takes exact / split / bf16x3 (hi + lo)
    and bf16, anything else is refused with nothing written; iddgcn_gemm_tn_bf16 has no precision argument, and
    ops.gemm_tn refuses the row-GEMM forms "exact4" and "bf16" before the call; iddgcn_rowgemm_f32 refuses "bf16"."""
    c = bf_case(65, "dsig", "dense")
    outs = {p: _bf_row_once(c, cuda, p, f"rowgemm_bf16[{p}]") for p in ALL_PRECS}
    for p in ("split", "exact4", "bf16x3"):
        assert torch.equal(outs[p], outs["exact"]), p
    assert not torch.equal(outs["bf16"], outs["exact"])
    s = stnb_case(65, "dense")
    souts = {}
    for p in ALL_PRECS:
        slab = torch.full((ops.sigma_tn_slab_floats(s.M),), NAN, device=cuda)
        dS = torch.full((D, D), NAN, device=cuda)
        X = s.X.to(cuda).clone()
        if p == "exact4":
            with pytest.raises(L.IddgcnError):
                ops.sigma_tn(s.dO.to(cuda), X, s.S.to(cuda), dS, slab, precision=p)
            assert torch.equal(X.cpu(), s.X) and bool(torch.isnan(dS).all()) and bool(torch.isnan(slab).all())
            continue
        ops.sigma_tn(s.dO.to(cuda), X, s.S.to(cuda), dS, slab, precision=p)
        souts[p] = (X.cpu(), dS.cpu())
    for p in ("split", "bf16x3"):
        assert torch.equal(souts[p][0], souts["exact"][0]) and torch.equal(souts[p][1], souts["exact"][1]), p
    assert torch.equal(souts["bf16"][1], souts["exact"][1]) and not torch.equal(souts["bf16"][0], souts["exact"][0])
    t = tnb_case(65, "dense", False)
    touts = {}
    for p in ALL_PRECS:
        slab = torch.full((ops.tn_blocks(t.M, D) * D * D,), NAN, device=cuda)
        C = torch.full((D, D), NAN, device=cuda)
        if p in ("exact4", "bf16"):
            with pytest.raises(L.IddgcnError):
                ops.gemm_tn(t.A.to(cuda), t.B.to(cuda), C, slab, precision=p)
            assert bool(torch.isnan(C).all())
            continue
        ops.gemm_tn(t.A.to(cuda), t.B.to(cuda), C, slab, precision=p)
        touts[p] = C.cpu()
    assert torch.equal(touts["split"], touts["exact"]) and torch.equal(touts["bf16x3"], touts["exact"])
    with pytest.raises(L.IddgcnError):
        ops.rowgemm(torch.rand(64, D, device=cuda), torch.randn(D, D, device=cuda), torch.empty(64, D, device=cuda),
                    precision="bf16")


def test_edge_gemm_maps_exact4_on_bf16_features():
    """Engine.edge_gemm without a device: the property alone (no kernel runs)."""
    from iddgcn_amd.engine import Engine
    e = Engine.__new__(Engine)
    e._gemm, e.D = "exact", 256
    for feat, mfma, row, want in (("bf16", "hilo", "exact4", "exact"), ("bf16", "hilo", "split", "split"),
                                  ("bf16", "bf16", "exact4", "bf16"), ("f32", "hilo", "exact4", "exact"),
                                  ("f32", "hilo", "bf16x3", "bf16x3"), ("bf16", "hilo", None, "exact")):
        e.features, e.edge_mfma, e._row_gemm = feat, mfma, row
        assert e.edge_gemm == want, (feat, mfma, row)
    e.D, e._row_gemm = 64, "exact4"                  # the register-staged kernel takes the four chains on every form
    assert e.edge_gemm == "exact4" and e._epilogue_gemm == "exact4"


@gpu
@pytest.mark.parametrize("features", ["bf16", "f32"])
def test_step_with_row_gemm_exact4_at_d256(features, cuda):
    """D = 256 with row_gemm = "exact4": the step runs and is bitwise the row_gemm = "exact" step.  features="bf16":
    the fused sigma' + dS pass takes no four-chain precision, and on bf16 tables "exact4" means the hi + lo weights
    "exact" means.  Either feature type: the four-chain kernel at D = 256 is the plain form only and iddgcn_rowgemm_f32
    refuses it on the forms with coefficients or a sigma' operand (every edge GEMM, the head chain's fused forward
    and backward at R <= 2), which therefore run the exact kernel under either name: loss, probabilities and every
    gradient bitwise."""
    from iddgcn_amd.engine import Engine, FlatParams
    from iddgcn_amd.graph import get_adj_mats
    from iddgcn_amd.utils import synthetic_graph
    N, R = 500, 2
    pos, neg = synthetic_graph(N, R, 4000, seed=7)
    tri = np.concatenate([pos, neg])
    lab = np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])
    rng = np.random.default_rng(3)
    params = {"E": rng.standard_normal((N, D)) / np.sqrt(D), "rel": rng.standard_normal((R, D))}
    for l in (1, 2, 3):
        params.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / np.sqrt(D),
                       f"Wa{l}": rng.standard_normal((D, R)) / np.sqrt(D), f"ba{l}": rng.standard_normal(R) * 0.1})
    out = {}
    for mode in ("exact", "exact4"):
        eng = Engine(N, R, D, cuda, features=features)
        eng.row_gemm = mode
        assert eng.sigma_tn_fused == (features == "bf16") and eng.edge_gemm == "exact"
        P, Gr = FlatParams(N, R, D, cuda), FlatParams(N, R, D, cuda)
        P.load(params)
        loss, p = eng.loss_and_grads(P, Gr, eng.adjacency(get_adj_mats(pos, N, R)), eng.edges(tri, lab))
        out[mode] = (loss.cpu().clone(), p.cpu().clone(), {k: v.copy() for k, v in Gr.to_numpy().items()})
    (l0, p0, g0), (l1, p1, g1) = out["exact"], out["exact4"]
    assert bool(torch.isfinite(l0).all()) and float(l0) > 0
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    for k in g0:
        assert np.all(np.isfinite(g0[k])) and np.any(g0[k] != 0), k
        assert np.array_equal(g0[k], g1[k]), k


# =============================================================================================================
# Part 2: split-fp16 operands (IDDGCN_GEMM_SPLIT_F16) and the planes tables, D = 256
# =============================================================================================================
REP16 = 2.0 ** -22            # hi + lo of a scaled value while lo is a normal fp16 (iddgcn_hip.hip: split16, split16_same)
ABS_SAME = 2.0 ** -39         # split16_same with lo subnormal: 2^-25 of the scaled value, whose row / block max >= 2^14
ABS_W = 2.0 ** -50            # split16 (lo carried at 2^11): 2^-36 of the scaled value, column max >= 2^14
SLACK = 1 + 2.0 ** -9         # second-order terms of the products of the errors above
SPLIT_ROW_FORMS = [f for f in G.ROW_FORMS]


def split_planes_encode(x):
    """x 2^15 = hi + lo as fp16 (include/iddgcn.h IDDGCN_PLANES_*): 8 column blocks of [hi[32] | lo[32]] per row."""
    xs = x.float() * 2.0 ** 15
    hi = xs.half()
    lo = (xs - hi.float()).half()
    M = x.shape[0]
    return torch.stack([hi.view(M, 8, 32), lo.view(M, 8, 32)], 2).reshape(M, 512).contiguous().view(F32)


def split_planes_decode(p):
    """The fp64 values a planes table holds: (hi + lo) 2^-15."""
    M = p.shape[0]
    h = p.contiguous().view(torch.float16).view(M, 8, 2, 32).double()
    return ((h[:, :, 0] + h[:, :, 1]) * 2.0 ** -15).reshape(M, 256)


def split_row_bound_z(c, ref, planes_a=False):
    """Family C bound of the split-fp16 row GEMM's pre-activation.  Per product a w: the pieces' relative errors and
    the dropped lo lo, 3 REP16; the absolute parts ABS_SAME rowmax |w| (A side, per-row scale; none for a planes
    table, whose decoded values are the operands) and ABS_W colmax |a| (weights, per-column scale).  Adds: 2 D into
    the hi accumulator, the combine acc_hi + 2^-11 acc_lo, the epilogue's (accumulate, R, sigma': 3), at MFMA_ADD."""
    z, Tg, Tc = ref
    A = c.A.double()
    Ar = A[c.a_idx] if c.a_idx is not None else A[:c.M]
    Bm = (c.B.double().t() if c.b_trans else c.B.double()).abs()
    n = 2 * c.D + 1 + int(c.accumulate) + c.R + (3 if c.act == "dsig" else 0)
    rowmax = Ar.abs().amax(1, keepdim=True) if c.M else Ar.abs().sum(1, keepdim=True)
    absA = 0.0 if planes_a else ABS_SAME * rowmax * Bm.sum(0, keepdim=True)
    absW = ABS_W * Ar.abs().sum(1, keepdim=True) * Bm.amax(0, keepdim=True)
    rep = (1 if planes_a else 3) * REP16
    return gam_e(n, MFMA_ADD) * (Tg + Tc) + SLACK * (rep * Tg + absA + absW)


def split_row_expect(c, ref=None, planes_a=False):
    ref = G.row_ref(c) if ref is None else ref
    bz = split_row_bound_z(c, ref, planes_a)
    z = ref[0]
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, bz * s
    if c.act == "sig":
        assert float(z.abs().max()) < 8.0
        return sigmoid_bar(z, bz)
    return z, bz


def split_row_single_bound(c):
    """Family B: one product a w per element.  a is its row's maximum (scaled into [2^14, 2^15): 22 bits, REP16); w
    within REP16 |w| + ABS_W colmax; wl al dropped (REP16); wh ah + wh al is one add, + 2^-11 (wl ah) another."""
    z, Tg, Tc = G.row_ref(c)
    A = c.A.double()
    Ar = A[c.a_idx] if c.a_idx is not None else A[:c.M]
    Bm = (c.B.double().t() if c.b_trans else c.B.double()).abs()
    b = SLACK * (3 * REP16 + 2 * MFMA_ADD) * Tg + SLACK * ABS_W * Ar.abs().sum(1, keepdim=True) * Bm.amax(0, keepdim=True)
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, s * (b * (1 + gam(3)) + gam(3) * Tg)
    return z, b + gam(c.R) * (Tg + b + Tc)


def split16_emul(y):
    """split16_same of scaled fp32 values: (hi, lo) as fp64."""
    hi = y.half().float()
    return hi.double(), (y - hi).half().double()


def split_row_emul(c, drop_lo=False):
    """The split-fp16 row GEMM in torch: per-row / per-column power-of-two scales, the three kept piece products
    summed in fp64, the scales undone, the fp32 epilogue.  drop_lo: the wl ah product left out."""
    A = c.A[c.a_idx] if c.a_idx is not None else c.A[:c.M]
    Bm = c.B.t() if c.b_trans else c.B

    def p2(m):                                                       # pow2_scale: m s in [2^14, 2^15)
        e = torch.floor(torch.log2(m.double().clamp_min(2.0 ** -111)))
        return torch.where(m > 0, 2.0 ** (14 - e), torch.ones_like(e)).float()
    sa, sw = p2(A.abs().amax(1, keepdim=True)), p2(Bm.abs().amax(0, keepdim=True))
    ah, al = split16_emul(A * sa)
    ys = Bm * sw
    wh = ys.half().float()
    wl = ((ys - wh) * 2048.0).half().double() / 2048.0
    wh = wh.double()
    zz = (ah @ wh + al @ wh + (0 if drop_lo else ah @ wl)) / sa.double() / sw.double()
    z = zz.float()
    if c.accumulate:
        z = z + c.C0
    if c.R:
        rows = torch.arange(c.M)
        cf = c.coef[rows if c.coef_idx is None else c.coef_idx]
        for r in range(c.R):
            v = c.V[r][None, :] if c.bcast else c.V[r][rows if c.v_idx is None else c.v_idx]
            z = (z.double() + cf[:, r:r + 1].double() * v.double()).float()
    if c.act == "dsig":
        z = z * (c.aux * (1.0 - c.aux))
    elif c.act == "sig":
        z = 1.0 / (1.0 + torch.exp(-z))
    return z


def _split_row_once(c, dev, what, planes=0):
    whole, C = guarded(dev, c.M, c.D)
    kw = dict(b_trans=c.b_trans, accumulate=c.accumulate, precision="split", M=c.M, planes=planes)
    if c.accumulate:
        C.copy_(c.C0)
    A = c.A
    if planes & L.PLANES_A:
        A = split_planes_encode(c.A)
    if c.act == "dsig":
        aux = split_planes_encode(c.aux) if planes & L.PLANES_AUX else c.aux
        if c.alias:
            C.copy_(aux)
        kw.update(act=L.ACT_DSIGMOID, aux=C if c.alias else aux.to(dev))
    elif c.act == "sig":
        kw.update(act=L.ACT_SIGMOID)
    if c.R:
        kw.update(coef=c.coef.to(dev), V=c.V.to(dev))
        if c.bcast:
            kw.update(v_rel_stride=c.D, v_row_stride=0)
        else:
            kw.update(v_rel_stride=c.V.shape[1] * c.D, v_idx=None if c.v_idx is None else c.v_idx.to(I32).to(dev),
                      coef_idx=None if c.coef_idx is None else c.coef_idx.to(I32).to(dev))
    if c.a_idx is not None:
        kw.update(a_idx=c.a_idx.to(I32).to(dev))
    A = A.to(dev)
    kid = ops.rowgemm_kernel_id(A, c.B.to(dev), C, **kw)
    assert 2000 <= kid < 4000, f"{what}: kernel {kid} is not a split-fp16 kernel (300-series + 2000, + 1000 planes)"
    ops.rowgemm(A, c.B.to(dev), C, **kw)
    out = C.cpu()
    guard_intact(whole, what)
    return out


def run_split_row(c, dev, what, planes=0):
    return _split_row_once(c, dev, what, planes), _split_row_once(c, dev, what + " (second run)", planes)


POW2_FORMS = ("plain", "b_trans", "dsig", "a_idx")           # no additive epilogue: the row's scale factors out


@gpu
@pytest.mark.parametrize("form", SPLIT_ROW_FORMS)
def test_rowgemm_split_exact_integers_bitwise(form, cuda):
    """Family A with precision "split": integers in [-4, 4] are fp16 values under any power-of-two scale (lo = 0),
    every product and sum exact: bitwise.  The forms without an additive epilogue also with row e scaled by 2^k,
    k = -20..20 across the rows (pow2_scale / pow2_inv): the result row is the integer row times 2^k exactly."""
    for M in G.ROW_MS:
        for vk in G._vkinds(form, M)[:3]:
            c = G.row_case(256, M, form, "int", vk)
            ref = G.row_exact(c)
            what = f"rowgemm[split] {form} int M{M} {vk}"
            a, b = run_split_row(c, cuda, what)
            assert_bitwise(a, ref, what)
            same_twice(a, b, what)
        if form in POW2_FORMS:
            c = G.row_case(256, M, form, "int", "sorted")
            ref = G.row_exact(c)
            k = 2.0 ** ((torch.arange(c.A.shape[0]) * 7) % 41 - 20).double()
            c.A = (c.A.double() * k[:, None]).float()
            kr = k[c.a_idx] if c.a_idx is not None else k[:M]
            what = f"rowgemm[split] {form} int x 2^k M{M}"
            a, _ = run_split_row(c, cuda, what)
            assert_bitwise(a, ref * kr[:, None], what)


@gpu
@pytest.mark.parametrize("mix", ["forms", "one_variant"])
def test_rowgemm_batched_split_exact_integers_bitwise(mix, cuda):
    spec = [("plain", 785), ("accumulate", 1), ("gather_R2", 33), ("dsig", 31), ("b_trans", 4097)] if mix == "forms" \
        else [("plain", 785), ("b_trans", 1), ("plain", 0), ("b_trans", 33), ("plain", 4097)]
    cases = [G.row_case(256, M, form, "int", "runs13") for form, M in spec]
    refs = [G.row_exact(c) for c in cases]
    wholes, calls = zip(*[G._batch_entry(c, cuda, "split") for c in cases])
    ops.rowgemm_batched(list(calls))
    for c, ref, w, call in zip(cases, refs, wholes, calls):
        what = f"rowgemm_batched[split] {mix} entry {c.form} M{c.M}"
        assert_bitwise(call[2], ref, what)
        guard_intact(w, what)


@gpu
@pytest.mark.parametrize("form", ["plain", "b_trans", "dsig", "a_idx", "gather_R2", "bcast_R2"])
def test_rowgemm_split_single_term(form, cuda):
    M = 2 * 256 + 17
    c = G.row_case(256, M, form, "single", "runs13")
    what = f"rowgemm[split] {form} single M{M}"
    a, b = run_split_row(c, cuda, what)
    assert_within(a, *split_row_single_bound(c), what)
    same_twice(a, b, what)


SPLIT_VARIANTS = ("dense", "row_decades", "zero_rows", "low_element")


def split_dense_case(M, form, variant):
    """Family C operands: the dense case of test_gpu_mfma_gemms, then rows spanning 12 decades, every third row zero,
    or one element per row 2^-12 below the row's maximum (its lo piece is a subnormal fp16)."""
    c = G.row_case(256, M, form, "dense", "runs13")
    g = _gen(M, SPLIT_VARIANTS.index(variant), 91)
    n = c.A.shape[0]
    if variant == "row_decades":
        c.A = c.A * 10 ** (12 * torch.rand(n, 1, generator=g) - 6)
    elif variant == "zero_rows":
        c.A[::3] = 0
    elif variant == "low_element":
        e = torch.arange(n)
        c.A[e, e % 256] = c.A.abs().amax(1) * 2.0 ** -12 * (1 + torch.rand(n, generator=g))
    return c


# (a sigmoid of rows at 1e6 saturates: the activation form runs the other variants)
SPLIT_DENSE = [(f, v) for f in ("plain", "accumulate", "dsig", "a_idx", "gather_R2", "gather_R2_sig", "bcast_R2_dsig")
               for v in SPLIT_VARIANTS if not (v == "row_decades" and f.endswith("_sig"))]


@gpu
@pytest.mark.parametrize("form,variant", SPLIT_DENSE)
def test_rowgemm_split_dense_per_element(form, variant, cuda):
    """Family C: every element within the split bound of its own terms, on rows spanning 12 decades (per-row
    scales), zero rows (exact zeros where nothing is added) and an element 2^-12 below its row's maximum."""
    for M in (1, 33, 785):
        c = split_dense_case(M, form, variant)
        what = f"rowgemm[split] {form} {variant} M{M}"
        a, b = run_split_row(c, cuda, what)
        assert_within(a, *split_row_expect(c), what)
        same_twice(a, b, what)


def test_selfcheck_split_row_bounds():
    for form in ("plain", "dsig", "gather_R2", "accumulate"):
        ci = G.row_case(256, 81, form, "int", "runs13")
        assert_bitwise(split_row_emul(ci), G.row_exact(ci), f"cpu emulation rowgemm[split] {form} int")
        for variant in SPLIT_VARIANTS:
            c = split_dense_case(81, form, variant)
            ref, bound = split_row_expect(c)
            assert_within(split_row_emul(c), ref, bound, f"cpu emulation rowgemm[split] {form} {variant}")
            mut = split_row_expect(c, G.row_ref(c, drop_k=7))[0]
            out = (mut - ref).abs() > bound.expand_as(ref)
            print(f"COVER rowgemm[split] {form} {variant}: a dropped k term trips {100 * share(out):.0f}%")
            assert bool(out.any())
    for form in ("plain", "dsig", "gather_R2"):
        c = G.row_case(256, 529, form, "single", "runs13")
        ref, bound = split_row_single_bound(c)
        assert_within(split_row_emul(c), ref, bound, f"cpu emulation rowgemm[split] {form} single")
        out = (split_row_emul(c, drop_lo=True).double() - ref).abs() > bound
        print(f"COVER rowgemm[split] {form} single: wl ah dropped trips {100 * share(out[ref != 0]):.0f}%")
        assert share(out[ref != 0]) > 0.5


# ---- gemm_tn256_x3_kernel ---------------------------------------------------------------------------------------
TN_PATTERNS = ("flat", "grow", "shrink", "zero_first", "zero_mid")


def tile_factor(M, pattern):
    """A power of two per row, constant within a 32-row tile, periodic over 5 tiles: the running block scale of a
    workgroup's row range (3 tiles per range at M = 4097 in a batch of four, 2 at M = 8225 alone) is lowered when the
    factor grows and kept when it shrinks; zero_first / zero_mid zero every fifth tile (the first of a range stays at
    S_INIT; a zero stretch inside a range)."""
    t = (torch.arange(M) // 32) % 5
    if pattern == "flat":
        return torch.ones(M, dtype=F64)
    if pattern == "grow":
        return 2.0 ** (2 * t).double()
    if pattern == "shrink":
        return 2.0 ** (2 * (4 - t)).double()
    f = 2.0 ** (2 * ((t + 2) % 5)).double()
    return torch.where(t == (0 if pattern == "zero_first" else 2), torch.zeros_like(f), f)


def tnx_case(M, kind, pattern, acc, seed=0):
    c = G.tn_case(256, M, kind, acc, seed=seed + 11 * TN_PATTERNS.index(pattern))
    f = tile_factor(M, pattern)
    c.A = (c.A.double() * f[:, None]).float()
    c.B = (c.B.double() * tile_factor(M, "shrink" if pattern == "grow" else "flat")[:, None]).float()
    c.pattern = pattern
    return c


def tnx_bound(c, T, n_partials, planes_a=False):
    """Per product: 3 REP16 relative (REP16 with a planes A); absolute ABS_SAME (block maximum) (the other operand):
    the maximum over the WHOLE table of the 32-column block, which the running maximum of a row range never exceeds.
    Adds: three products per row, the slab partials, the accumulated C, at MFMA_ADD."""
    A, B = c.A.double().abs(), c.B.double().abs()
    n = 3 * c.M + n_partials + int(c.acc)
    blk = lambda X: X.amax(0).view(8, 32).amax(1).repeat_interleave(32) if c.M else X.sum(0)      # noqa: E731
    absA = 0.0 if planes_a else ABS_SAME * blk(A)[:, None] * B.sum(0)[None, :]
    absB = ABS_SAME * A.sum(0)[:, None] * blk(B)[None, :]
    return gam_e(n, MFMA_ADD) * T + SLACK * ((1 if planes_a else 3) * REP16 * T + absA + absB)


def tnx_single_bound(c, T):
    """One product per element: two adds of the three piece products instead of 3 M."""
    A, B = c.A.double().abs(), c.B.double().abs()
    blk = lambda X: X.amax(0).view(8, 32).amax(1).repeat_interleave(32)                           # noqa: E731
    live = B[c.pi]                                                  # the B row each column of A meets
    return SLACK * ((3 * REP16 + 2 * MFMA_ADD) * T + ABS_SAME * (blk(A)[:, None] * live + A.sum(0)[:, None] * blk(B)[None, :]))


def tnx_emul(c, rpb, scale_bug_tile=None):
    """gemm_tn256_x3_kernel in torch: per row range of rpb rows and per 32-row tile the running power-of-two scale of
    every 32-column block (lowered when the tile's maximum would reach 2^15), split16_same pieces, the three kept
    products in fp64 in scaled units with the exact rescaling, the partials summed in fp64.  scale_bug_tile: the A
    block scales of that tile used a factor two too large without the accumulators being told."""
    M = c.M
    out = torch.zeros(256, 256, dtype=F64)
    for r0 in range(0, max(M, 1), rpb):
        sA = torch.full((8,), 2.0 ** 126, dtype=F64)
        sB = sA.clone()
        acc = torch.zeros(256, 256, dtype=F64)
        for t0 in range(r0, min(r0 + rpb, M), 32):
            At, Bt = c.A[t0:t0 + 32], c.B[t0:t0 + 32]
            for X, s, is_a in ((At, sA, True), (Bt, sB, False)):
                m = X.abs().amax(0).view(8, 32).amax(1).double()
                low = m * s >= 32768.0
                e = torch.floor(torch.log2(m.clamp_min(2.0 ** -140)))
                s_new = torch.where(low, 2.0 ** (14 - e), s)
                f = (s_new / s).repeat_interleave(32)
                acc = acc * (f[:, None] if is_a else f[None, :])
                s.copy_(s_new)
            sa = sA.repeat_interleave(32)
            if scale_bug_tile is not None and t0 // 32 == scale_bug_tile:
                sa = sa * 2
            ah, al = split16_emul((At.double() * sa[None, :]).float())
            bh, bl = split16_emul((Bt.double() * sB.repeat_interleave(32)[None, :]).float())
            acc = acc + ah.t() @ bh + ah.t() @ bl + al.t() @ bh
        out += (acc / sA.repeat_interleave(32)[:, None] / sB.repeat_interleave(32)[None, :]).float().double()
    if c.acc:
        out += c.C0.double()
    return out.float()


def run_tnx(c, dev, what, planes_a=False):
    outs = []
    A = split_planes_encode(c.A) if planes_a else c.A
    for _ in range(2):
        slab = torch.full((ops.tn_blocks(c.M, 256) * 256 * 256,), NAN, device=dev)
        whole, C = guarded(dev, 256, 256)
        if c.acc:
            C.copy_(c.C0)
        ops.gemm_tn(A.to(dev), c.B.to(dev), C, slab, accumulate=c.acc, a_planes=planes_a, precision="split")
        outs.append(C.cpu())
        guard_intact(whole, what)
    return outs


def run_tnx_batched(cases, dev, what):
    """Four entries in one launch: 64 row ranges each, so M = 4097 has three tiles per range."""
    slab = torch.full((sum(max(1, min(64, (c.M + 31) // 32)) for c in cases) * 256 * 256,), NAN, device=dev)
    wholes, ents = [], []
    for c in cases:
        w, C = guarded(dev, 256, 256)
        if c.acc:
            C.copy_(c.C0)
        wholes.append(w)
        ents.append((c.A.to(dev), c.B.to(dev), C, c.acc))
    ops.gemm_tn_batched(ents, slab, precision="split")
    for c, w in zip(cases, wholes):
        guard_intact(w, f"{what} entry M{c.M}")
    return [e[2].cpu() for e in ents]


def tnx_exact(c):
    """The exact result; every term is a multiple of 1 (factors >= 1) and the sum of moduli stays below 2^24, so every
    partial sum, in scaled units too (a power of two away), is exact in fp32 in any order."""
    z, T = G.tn_ref(c)
    assert float(T.max()) < LIM, "integer case leaves the exact range of fp32"
    return z


@gpu
@pytest.mark.parametrize("pattern", TN_PATTERNS)
@pytest.mark.parametrize("acc", [False, True])
def test_gemm_tn_split_exact_integers_bitwise(pattern, acc, cuda):
    """Family A: integers times powers of two per tile (growing, shrinking, zero first tiles, a zero stretch): bitwise
    from a NaN-filled slab, alone (M around the tiles, several blocks, two tiles per block at 8225) and as four entries
    of one launch (three tiles per range at 4097, an empty entry); twice."""
    for M in TNB_MS + (TNB_M2,):
        c = tnx_case(M, "int", pattern, acc)
        what = f"gemm_tn[split] int {pattern} M{M} acc{int(acc)}"
        a, b = run_tnx(c, cuda, what)
        assert_bitwise(a, tnx_exact(c), what)
        same_twice(a, b, what)
    cases = [tnx_case(M, "int", pattern, (k % 2 == 1) != acc, seed=3) for k, M in enumerate((4097, 33, 0, 2049))]
    what = f"gemm_tn_batched[split] int {pattern}"
    for c, got in zip(cases, run_tnx_batched(cases, cuda, what)):
        assert_bitwise(got, tnx_exact(c) if c.M else (c.C0.double() if c.acc else torch.zeros(256, 256, dtype=F64)),
                       f"{what} entry M{c.M} acc{int(c.acc)}")


@gpu
@pytest.mark.parametrize("pattern", TN_PATTERNS)
def test_gemm_tn_split_single_term(pattern, cuda):
    """Family B: column i of A non-zero only in row pi(i), so every element is one product and every tile's block
    maxima differ: the bound holds the block maximum's absolute term; alone and in a batch of four."""
    for M in (785, 4097, TNB_M2):
        c = tnx_case(M, "single", pattern, False)
        z, T = G.tn_ref(c)
        what = f"gemm_tn[split] single {pattern} M{M}"
        a, _ = run_tnx(c, cuda, what)
        assert_within(a, z, tnx_single_bound(c, T), what)
    cases = [tnx_case(M, "single", pattern, False, seed=5) for M in (4097, 785, 2049, 4097)]
    for c, got in zip(cases, run_tnx_batched(cases, cuda, "gemm_tn_batched[split] single")):
        z, T = G.tn_ref(c)
        assert_within(got, z, tnx_single_bound(c, T), f"gemm_tn_batched[split] single {pattern} M{c.M}")


@gpu
@pytest.mark.parametrize("pattern", TN_PATTERNS)
@pytest.mark.parametrize("acc", [False, True])
def test_gemm_tn_split_dense_per_element(pattern, acc, cuda):
    for M in SHORT_MS:
        c = tnx_case(M, "dense", pattern, acc)
        z, T = G.tn_ref(c)
        what = f"gemm_tn[split] dense {pattern} M{M} acc{int(acc)}"
        a, b = run_tnx(c, cuda, what)
        assert_within(a, z, tnx_bound(c, T, ops.tn_blocks(M, 256)), what)
        same_twice(a, b, what)
    cases = [tnx_case(M, "dense", pattern, acc, seed=7) for M in (257, 193, 129, 161)]       # up to 9 tiles: 1 per range
    for c, got in zip(cases, run_tnx_batched(cases, cuda, "gemm_tn_batched[split] dense")):
        z, T = G.tn_ref(c)
        assert_within(got, z, tnx_bound(c, T, (c.M + 31) // 32), f"gemm_tn_batched[split] dense {pattern} M{c.M}")


def test_selfcheck_tn_split_bounds():
    """The emulation with the running scales (ranges of three tiles) is bitwise on family A, inside the bars of B and
    C; a block scale off by two for one tile, and one row of the last block dropped, are refused."""
    for pattern in TN_PATTERNS:
        ci = tnx_case(257, "int", pattern, True)
        assert_bitwise(tnx_emul(ci, 96), tnx_exact(ci), f"cpu emulation tn[split] int {pattern}")
        with pytest.raises(AssertionError):
            assert_bitwise(tnx_emul(ci, 96, scale_bug_tile=4), tnx_exact(ci), "scale off by two")
        c = tnx_case(257, "dense", pattern, True)
        z, T = G.tn_ref(c)
        bound = tnx_bound(c, T, 3)
        assert_within(tnx_emul(c, 96), z, bound, f"cpu emulation tn[split] dense {pattern}")
        out = (tnx_emul(c, 96, scale_bug_tile=4).double() - z).abs() > bound
        print(f"COVER tn[split] dense {pattern}: a block scale off by two for one tile trips {100 * share(out):.0f}%")
        assert bool(out.any()) or pattern in ("zero_first",) and not bool(c.A[128:160].any())
        assert rejects(G.tn_ref(c, drop_row=256)[0], z, bound)
        c = tnx_case(785, "single", pattern, False)
        z, T = G.tn_ref(c)
        bound = tnx_single_bound(c, T)
        assert_within(tnx_emul(c, 96), z, bound, f"cpu emulation tn[split] single {pattern}")
        live_tile = int(c.pi[(c.A.abs().sum(0) > 0).nonzero()[-1]]) // 32
        out = (tnx_emul(c, 96, scale_bug_tile=live_tile).double() - z).abs() > bound
        print(f"COVER tn[split] single {pattern}: a block scale off by two for tile {live_tile} trips {100 * share(out):.1f}%")
        assert bool(out.any())
        assert rejects(G.tn_ref(c, drop_row=int(c.pi[(c.A.abs().sum(0) > 0).nonzero()[-1]]))[0], z, bound)


# ---- planes -------------------------------------------------------------------------------------------------------
def quarters(g, *shape):
    """Values of a planes table that are exact in it and in the integer arithmetic: multiples of 1/4 in [0, 1]."""
    return torch.randint(0, 5, shape, generator=g).float() / 4


def unit_rows(g, M):
    """Rows of values in [0, 1) with the maximum in [0.5, 1) (sigmoid-like), as the planes tables hold."""
    x = torch.rand(M, 256, generator=g)
    if M:
        x[:, 0] = 0.5 + 0.49 * torch.rand(M, generator=g)
    return x


@gpu
def test_planes_consumers_exact_integers_bitwise(cuda):
    """Family A against the decoded table: A planes of multiples of 1/4 (plain row GEMM, TN), the sigma' operand as
    planes of {1/4, 1/2, 3/4} (also in place over it): bitwise."""
    for M in (1, 31, 33, 785, 4097):
        g = _gen(M, 101)
        c = G.row_case(256, M, "plain", "int", "sorted")
        c.A = quarters(g, M, 256)
        assert torch.equal(split_planes_decode(split_planes_encode(c.A)), c.A.double())
        what = f"rowgemm[split, planes A] int M{M}"
        a, b = run_split_row(c, cuda, what, planes=L.PLANES_A)
        assert_bitwise(a, c.A.double() @ c.B.double(), what)
        same_twice(a, b, what)
        for form in ("dsig", "dsig_inplace"):
            c = G.row_case(256, M, form, "int", "sorted")
            if form == "dsig_inplace":
                c.aux = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (M, 256), generator=g)]
            what = f"rowgemm[split, planes aux] {form} int M{M}"
            a, b = run_split_row(c, cuda, what, planes=L.PLANES_AUX)
            assert_bitwise(a, G.row_exact(c), what)
            same_twice(a, b, what)
        for pattern in ("flat", "grow", "zero_first"):
            t = tnx_case(M, "int", pattern, False, seed=9)
            t.A = quarters(g, M, 256)
            z, T = G.tn_ref(t)
            assert float(T.max()) * 4 < LIM
            what = f"gemm_tn_planes int {pattern} M{M}"
            a, b = run_tnx(t, cuda, what, planes_a=True)
            assert_bitwise(a, z, what)
            same_twice(a, b, what)


@gpu
def test_planes_consumers_dense_per_element(cuda):
    """Family C against fp64 on the DECODED values (the A side then carries no representation error): the gathered
    forward with A planes, the sigma' backward with planes aux, the planes TN at short M."""
    for M in (1, 33, 785):
        g = _gen(M, 103)
        for form in ("plain", "gather_R2_sig", "dsig"):
            c = G.row_case(256, M, form, "dense", "runs13")
            if form == "dsig":
                c.aux = split_planes_decode(split_planes_encode(unit_rows(g, M))).float()
                pl = L.PLANES_AUX
            else:
                c.A = split_planes_decode(split_planes_encode(unit_rows(g, M))).float()
                pl = L.PLANES_A
            what = f"rowgemm[split, planes {pl}] {form} dense M{M}"
            a, _ = run_split_row(c, cuda, what, planes=pl)
            assert_within(a, *split_row_expect(c, planes_a=pl == L.PLANES_A), what)
    for M in SHORT_MS:
        t = tnx_case(M, "dense", "flat", False, seed=13)
        t.A = split_planes_decode(split_planes_encode(unit_rows(_gen(M, 107), M))).float()
        z, T = G.tn_ref(t)
        what = f"gemm_tn_planes dense M{M}"
        a, _ = run_tnx(t, cuda, what, planes_a=True)
        assert_within(a, z, tnx_bound(t, T, ops.tn_blocks(M, 256), planes_a=True), what)


@gpu
@pytest.mark.parametrize("R", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_planes_producers_per_element(R, cuda):
    """The planes-out combine (every R) and the gathered forward writing C as planes (it exists for R = 1, 2): the
    decoded output within the fp64 sigmoid's bar of test_gpu_mfma_gemms plus the encoding's 2^-24 (the encoding itself
    is test_gpu_planes.py's)."""
    for M in (1, 63, 65, 785):
        c = G.comb_case(256, M, R, "run")
        whole, out = guarded(cuda, M, 256)
        idx = c.y_idx.to(I32).to(cuda)
        ops.combine(c.Y.to(cuda), c.coef.to(cuda), c.V.to(cuda), out, y_idx=idx, v_idx=idx, planes_out=True)
        what = f"combine planes-out R{R} M{M}"
        guard_intact(whole, what)
        ref, bound = G.comb_ref(c)
        assert_within(split_planes_decode(out.cpu()), ref, bound + 2.0 ** -24, what)
    if R in (1, 2):
        for M in (1, 33, 785):
            c = G.row_case(256, M, f"gather_R{R}_sig" if R != 2 else "gather_R2_sig", "dense", "runs13")
            c.A = split_planes_decode(split_planes_encode(unit_rows(_gen(M, 109), M))).float()
            what = f"rowgemm[split, planes A | C] R{R} M{M}"
            a, _ = run_split_row(c, cuda, what, planes=L.PLANES_A | L.PLANES_C)
            ref, bound = split_row_expect(c, planes_a=True)
            assert_within(split_planes_decode(a), ref, bound + 2.0 ** -24, what)


def test_selfcheck_planes_encoding_of_the_test_values():
    g = _gen(113)
    q = quarters(g, 64, 256)
    assert torch.equal(split_planes_decode(split_planes_encode(q)), q.double())
    x = unit_rows(g, 64)
    d = split_planes_decode(split_planes_encode(x))
    assert float((d - x.double()).abs().max()) <= 2.0 ** -24
    assert torch.equal(split_planes_decode(split_planes_encode(d.float())), d)        # decoded values re-encode exactly
