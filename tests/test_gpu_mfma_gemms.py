"""Bars that can fail for the D = 256 MFMA GEMMs and their exact-f32 siblings: iddgcn_rowgemm_f32 (every form),
iddgcn_rowgemm_batched_f32, iddgcn_gemm_tn_f32, iddgcn_gemm_tn_batched_f32, iddgcn_sigma_tn_f32, iddgcn_combine_f32.

Every GPU test compares a kernel with an fp64 (or integer) torch evaluation of the same operation on the same fp32
inputs.  No bar is taken from another kernel's output.  Three families of input, each closing one way to hide an error:

  A. EXACT-INTEGER operands (integers in [-4, 4] as fp32; the sigma' operand 0.5 or from {0.25, 0.5, 0.75}, so that
     x (1 - x) is 1/4 or 3/16).  Every product and partial sum is an integer (a multiple of 1/4 for sigma_tn's dS, of
     1/16 after sigma') below 2^24, so every fp32 operation is exact in ANY order, and the values are bf16-exact (the
     second and third bf16x3 pieces are zero).  The result must be BITWISE the reference, whatever the MFMA does
     inside.  The builders assert sum |terms| < 2^24 from the reference.  Coverage and addressing, zero tolerance.
     The gathered-row addressing test (A = 0, one-hot coefficients) uses full-mantissa V rows: 0 + 1 v = v exactly.
  B. SINGLE-TERM operands (full-mantissa random values placed so that every output element is one product; all
     other terms are exact zeros, x + 0 is exact).  Exact kernels: one rounding, u |a b|.  bf16x3: split3
     (iddgcn_hip.hip, "bf16x3 operands") gives |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|, so the three dropped products are
     at most DROP1 = (2^-23 + 2^-32) |a b|, and the six kept products (sum of moduli <= (1 + 2^-7) |a b|) meet five fp32
     adds, each taken at MFMA_ADD: about 12 u |a b| in all, while a missing a0 w2, a2 w0 or a1 w1 is ~2^-16 |a b|.
  C. DENSE random operands at short lengths, per element: with T the sum of the moduli of the element's terms,
         bound = (gamma_e(n) + DROP) T,   gamma_e(n) = n e / (1 - n e)
     n = the roundings on the longest path (row forms: D, or 6 D for bf16x3, + accumulate + R + 3 for sigma'
     (1 - x, x (1 - x), the product); TN: M, or 6 M, + the slab partials + accumulate), e = u and DROP = 0 for the exact
     kernels (any summation order is covered), e = MFMA_ADD and DROP = 2 u (1 + 2^-7) for bf16x3.

MFMA_ADD = 2 u is the module's ONE ASSUMPTION about the hardware, and it is assumed, not measured: the order and
rounding of the fp32 adds inside v_mfma_f32_16x16x32_bf16 are not documented, so each add is taken to err by at most
one fp32 ulp of the running sum (truncation as well as round-to-nearest).  Families A and B do not depend on it
beyond B's five adds.

Sigmoid forms (ACT_SIGMOID of the row GEMMs, combine): sigmoid_fast is v_rcp_f32(1 + __expf(-x)).  The bound on z is
carried through the monotone fp64 sigmoid (evaluated at z -+ bound) and sig_fast_rel(z) sigma(z) is added, built from
the kernel source's "~2 ulp" for the instruction pair, one ulp = 2 u:  (1 - sigma) (2 u [v_exp_f32] + |x| u [the
rounding of x log2 e, through exp]) + u [1 + t] + 2 u [v_rcp_f32]; 4 u at x = 0.  It is checked on its own by
test_sigmoid_fast_allowance (combine with R = 0 on a grid of arguments: no GEMM in front of it).

What the bars replace (the old references replayed in fp64 on the CPU, same seeds and shapes):
    test_rowgemm_plain D = 256           max|ref| 78     old limit 2.5e-2 on every element (terms of order 1)
    test_gemm_tn D = 256, M = 5003       max|ref| 320    old limit 4.5e-2
    test_rowgemm_bf16x3_vs_fp64, test_gemm_tn_bf16x3_vs_fp64, test_gemm_tn_batched, test_gpu_sigma_tn_b3,
    test_gpu_rowgemm_b3_ksplit           max(1.25 x the exact kernel's own max-norm error, 1e-6) of max|ref|: moves
                                         with any error the two kernels share (epilogue, index arithmetic)
    R > 2 gathered forward               2e-5 of max|ref| = 1 AFTER the sigmoid; A ~ U(0, 1), S ~ N(0, 1): std of
                                         z = 9.9, 28% of the outputs within 2e-5 of 0 or 1 (any z of that sign passes),
                                         half of all outputs with a slope below 1e-3
Here a family C row bound at D = 256 is 1.8e-4 T (exact kernels: 1.5e-5 T) against a dropped k term of ~4e-3 T.

Worst observed |err| / bound on an MI355X over all forms, M and v_idx patterns of each kernel (1 = at the bound;
families A: every case bitwise):
    row GEMM, family C (dense)   v3 exact (300-382) linear / sigma' 0.023, sigmoid 0.051; four-chain (4300) 0.0082;
                                 register kernel (100, D = 64) 0.076, sigmoid 0.13; bf16x3 (500-520) 0.00070, sigmoid
                                 0.00097
    row GEMM, family B (single)  exact kernels 0.997 (one rounding: up to half an ulp of u |a b|); bf16x3 plain 0.13,
                                 sigma' 0.21, gathered combine 0.95 (its R fused multiply-adds dominate that bound)
    gemm_tn                      dense: exact 0.56 (D = 256), 0.60 (D = 32, 64), bf16x3 0.14; single: exact 0.998,
                                 bf16x3 0.19
    sigma_tn (bf16x3)            dS dense 0.074, single 0.19; dX 0.00048
    combine                      generic 0.50, dense rows 0.56, run form 0.58
    sigmoid_fast (combine R = 0) 0.64 of sig_fast_rel on both kernels; the worst relative error on the grid is 21.7 u,
                                 which only the |x| u term admits (large negative x: 25 u allowed at -20, 35 u at -30).
                                 The source's "~2 ulp" stands; no measured constant was needed
The bf16x3 ratios of family C are small because gamma_e(6 D) with MFMA_ADD = 2 u grows like n while the hardware's
errors do not all align; the bound is kept as derived.  What makes it bite is the short sum: at D = 256 it is 1.8e-4 T,
a dropped k term ~4e-3 T (refused on ~90% of the elements in the CPU self-check, 98% for the exact kernels).

The tests without the `gpu` mark evaluate every bound builder on the CPU: a fp32 torch evaluation of the same
operation on the tests' own inputs (for bf16x3 a torch emulation of split3 and the six products, summed in fp64) must
lie inside, and deliberate errors must be refused: a dropped k term, a gathered row replaced by its neighbour, the
last ragged tile left at its sentinel, one of the three low piece products dropped, one row of the last TN block
dropped.
"""
import math
from types import SimpleNamespace

import pytest
import torch

from bounds import NAN, U, assert_within, gam, guard_intact, guarded, rejects
from iddgcn_amd import _lib as L
from iddgcn_amd import ops

gpu = pytest.mark.gpu
F64, F32, I32 = torch.float64, torch.float32, torch.int32
MFMA_ADD = 2.0 * U                          # ASSUMED: one fp32 ulp of the running sum per add inside a bf16 MFMA
DROP3 = 2.0 * U * (1 + 2.0 ** -7)           # the three dropped piece products of every term, relative to sum |terms|
DROP1 = 2.0 ** -23 + 2.0 ** -32             # the same for ONE product: |a1 w2| + |a2 w1| + |a2 w2|
B3_SINGLE = DROP1 + (1 + 2.0 ** -7) * 5 * MFMA_ADD / (1 - 5 * MFMA_ADD)       # + five adds of the six kept products
LIM = 2.0 ** 24
ROW_MS = (1, 5, 31, 32, 33, 785, 4097)      # 785 = 32 * 8 * 3 + 17: several row ranges plus a ragged tile
TN_MS = (1, 15, 16, 17, 31, 33, 785, 4097)
SHORT_MS = (1, 15, 17, 33, 257)
VKINDS = ("sorted", "runs13", "random", "identity", "onerun")


def gam_e(n, e):
    ne = n * e
    return ne / (1 - ne)


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def assert_bitwise(got, ref, what):
    """got (fp32) == ref (fp64 values that are fp32-exact), every element; a NaN sentinel fails."""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    bad = ~(g == ref)
    if bad.any():
        at = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ from the exact reference, first at "
                             f"{at}: got {float(g[at])!r}, ref {float(ref[at])!r}")


def refuses(cand, ref, bound):
    """The bar refuses `cand`: an element out of bound, or one that is not finite (a sentinel never overwritten)."""
    try:
        assert_within(cand, ref, bound, "mutant")
    except AssertionError:
        return True
    return False


# =============================================================================================================
# sigmoid_fast
# =============================================================================================================
def sig_fast_rel(x):
    """Relative allowance of sigmoid_fast at the fp32 argument x (fp64 tensor), from the source's "~2 ulp" for the
    v_exp_f32 + v_rcp_f32 pair: the exp's ulp and the |x| u of its argument's scaling act on t = e^-x, to which
    sigma = 1 / (1 + t) has relative sensitivity 1 - sigma; then the rounding of 1 + t and the rcp's ulp."""
    q = torch.sigmoid(-x)
    return q * (2 * U + x.abs() * U) + U + 2 * U


def sigmoid_bar(z, bz):
    """sigma(z) and its bound for a pre-activation known within bz: the monotone fp64 sigmoid at both ends of
    [z - bz, z + bz], plus the activation's own allowance at the worse end."""
    s = torch.sigmoid(z)
    up, dn = torch.sigmoid(z + bz), torch.sigmoid(z - bz)
    rel = torch.maximum(sig_fast_rel(z + bz), sig_fast_rel(z - bz))
    return s, torch.maximum(up - s, s - dn) + rel * up


def sig_grid(D=256):
    """fp32 arguments in [-30, 30]: a uniform sweep, dense points in [-1, 1], and +-2^-k down to 2^-20 (with 0)."""
    n = 64 * D
    a = torch.linspace(-30, 30, n // 2, dtype=F64)
    b = torch.linspace(-1, 1, n // 4, dtype=F64)
    k = torch.arange(n // 4, dtype=F64)
    c = torch.where(k % 2 == 0, 1.0, -1.0) * 2.0 ** -(k // 2 % 21) * (1 + (k // 42) / (n // 4))
    c[0] = 0.0
    return torch.cat([a, b, c]).float().view(-1, D)


def test_selfcheck_sigmoid_allowance():
    x = sig_grid()
    ref = torch.sigmoid(x.double())
    bound = sig_fast_rel(x.double()) * ref
    assert float(x.min()) == -30 and float(x.max()) == 30 and bool((x == 0).any())
    assert_within(1.0 / (1.0 + torch.exp(-x)), ref, bound, "cpu-fp32 sigmoid on the grid")
    assert 3.9 * U < float(sig_fast_rel(torch.zeros(1, dtype=F64))) <= 4 * U
    assert rejects(ref * (1 + 1e-6), ref, bound) and rejects(torch.sigmoid(x.double() * (1 + 1e-5)), ref, bound)
    # the propagated form: an argument off by more than its bound is refused, one inside it is not
    z = x.double()[::4]
    s, b = sigmoid_bar(z, 1e-6 * (1 + z.abs()))
    assert not rejects(torch.sigmoid(z + 0.9e-6 * (1 + z.abs())), s, b)
    assert rejects(torch.sigmoid(z + 4e-6 * (1 + z.abs())), s, b)


@gpu
@pytest.mark.parametrize("form", ["generic", "run"])
def test_sigmoid_fast_allowance(form, cuda):
    """combine with R = 0 is sigmoid_fast of Y alone (no GEMM, no sum in front): its error against the fp64 sigmoid of
    the same fp32 arguments within sig_fast_rel, on both combine kernels (generic; the D = 256 run form)."""
    x = sig_grid()
    M, D = x.shape
    ref = torch.sigmoid(x.double())
    whole, out = guarded(cuda, M, D)
    idx = torch.arange(M, dtype=I32, device=cuda) if form == "run" else None
    ops.combine(x.to(cuda), torch.empty(M, 0, device=cuda), torch.empty(0, M, D, device=cuda), out, y_idx=idx, v_idx=idx)
    guard_intact(whole, "combine R = 0")
    err = (out.cpu().double() - ref).abs() / ref
    near = float(err[x.abs() <= 1].max()) / U
    print(f"SIGFAST {form}: worst relative error {float(err.max()) / U:.3f} u; within |x| <= 1: {near:.3f} u")
    assert_within(out, ref, sig_fast_rel(x.double()) * ref, f"sigmoid_fast via combine R0 ({form})")


# =============================================================================================================
# Row GEMM: forms, inputs, reference
# =============================================================================================================
def _row_forms():
    """name -> (options, {precision: the kernel id at D = 256 as include/iddgcn.h documents it}).  bf16x3 forms its
    kernel does not take (a_idx, coef_idx, R > 2, accumulate with broadcast V) name the exact kernel that runs."""
    F = {}

    def add(name, exact, b3, exact4=None, **opt):
        ids = {"exact": exact, "bf16x3": b3}
        if exact4:
            ids["exact4"] = exact4
        F[name] = (opt, ids)
    add("plain", 300, 500, 4300)
    add("b_trans", 300, 500, 4300, b_trans=True)
    add("accumulate", 300, 501, 4300, accumulate=True)
    add("dsig", 301, 501, b_trans=True, act="dsig", aux="mixed")
    add("dsig_inplace", 301, 501, b_trans=True, act="dsig", aux="half", alias=True)
    for R in (1, 2, 3, 4, 5, 8):
        nv = R if R <= 2 else 4 if R <= 4 else 8
        add(f"gather_R{R}", 302 + 10 * nv, 500 + 10 * R if R <= 2 else 302 + 10 * nv, R=R, vmode="gather")
    add("coef_idx", 322, 322, R=2, vmode="gather", coef_idx=True)
    add("a_idx", 300, 300, 4300, a_idx=True)
    for R in (1, 2, 4, 8):
        for dsig in (False, True):
            for acc in (False, True):
                ex = 302 + int(dsig) + (8 if R > 2 else 0)
                extra = dict(act="dsig", aux="mixed") if dsig else {}
                add(f"bcast_R{R}" + ("_dsig" if dsig else "") + ("_acc" if acc else ""), ex,
                    502 + int(dsig) if R <= 2 and not acc else ex, b_trans=True, R=R, vmode="bcast", accumulate=acc, **extra)
    return F


ROW_FORMS = _row_forms()
# the activation forms (family C only: a sigmoid output is no integer)
SIG_FORMS = {"plain_sig": (dict(act="sig"), {"exact": 300, "bf16x3": 500}),
             "accumulate_sig": (dict(act="sig", accumulate=True), {"exact": 300, "bf16x3": 300}),
             "coef_idx_sig": (dict(act="sig", R=2, vmode="gather", coef_idx=True), {"exact": 322, "bf16x3": 322})}
for _R in (1, 2, 3, 8):
    SIG_FORMS[f"gather_R{_R}_sig"] = (dict(ROW_FORMS[f"gather_R{_R}"][0], act="sig"), ROW_FORMS[f"gather_R{_R}"][1])
ALL_FORMS = {**ROW_FORMS, **SIG_FORMS}
NAMED_IDS = {100, 300, 301, 302, 303, 310, 311, 312, 322, 342, 382, 500, 501, 502, 503, 510, 520, 4300}


def test_selfcheck_every_named_kernel_id_has_a_family_a_case():
    ids = {100} | {k for _, by in ROW_FORMS.values() for k in by.values()}
    assert ids == NAMED_IDS, sorted(ids ^ NAMED_IDS)


def v_index(kind, M, g):
    """(v_idx or None, table rows N).  sorted: runs of ~4 equal rows; runs13: runs of 1-3 (~16 distinct rows per 32-row
    tile: past the 7 the capped LDS slabs keep, the rest come from L2); random: unsorted, 32 distinct rows per full
    tile; identity: no v_idx, 32 distinct rows per tile; onerun: one row for every edge (a run spanning all tiles)."""
    if kind == "identity":
        return None, M
    if kind == "sorted":
        N = max(1, M // 4)
        return torch.randint(0, N, (M,), generator=g).sort().values, N
    if kind == "runs13":
        idx = torch.repeat_interleave(torch.arange(M), torch.randint(1, 4, (M,), generator=g))[:M]
        return idx, int(idx.max()) + 1
    if kind == "random":
        N = max(M, 40)
        return torch.randperm(N, generator=g)[:M], N
    return torch.full((M,), 1, dtype=torch.int64), 3


def row_case(D, M, form, kind, vkind="sorted"):
    """CPU fp32 operands of one row GEMM.  kind: "int" (family A), "single" (family B: A row e non-zero only in column
    e mod D), "dense" (family C: S / 16, X in [0.05, 0.95], |z| of the activation forms within +-8)."""
    opt = ALL_FORMS[form][0]
    g = _gen(D, M, sorted(ALL_FORMS).index(form), VKINDS.index(vkind), len(kind))
    c = SimpleNamespace(D=D, M=M, form=form, kind=kind, b_trans=opt.get("b_trans", False),
                        accumulate=opt.get("accumulate", False), act=opt.get("act", "none"), alias=opt.get("alias", False),
                        R=opt.get("R", 0), bcast=opt.get("vmode") == "bcast", a_idx=None, coef_idx=None, v_idx=None,
                        C0=None, aux=None, coef=None, V=None)
    integer = kind == "int"
    rn = (lambda *s: ints(g, *s)) if integer else (lambda *s: torch.randn(*s, generator=g))
    NA = M + 5 if opt.get("a_idx") else M
    if kind == "single":
        c.A = torch.zeros(NA, D)
        e = torch.arange(NA)
        c.A[e, e % D] = torch.randn(NA, generator=g)
        c.B = torch.randn(D, D, generator=g)
    else:
        c.A = torch.rand(NA, D, generator=g) if (c.act == "sig" and not integer) else rn(NA, D)
        c.B = rn(D, D) if integer else rn(D, D) / 16
    if opt.get("a_idx"):
        c.a_idx = torch.randint(0, NA, (M,), generator=g)
    if c.accumulate:
        c.C0 = rn(M, D)
    if c.act == "dsig":
        if integer:
            c.aux = torch.full((M, D), 0.5) if opt["aux"] == "half" else \
                torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (M, D), generator=g)]
        else:
            c.aux = 0.05 + 0.9 * torch.rand(M, D, generator=g)
    if c.R:
        if c.bcast:
            c.coef, c.V = rn(M, c.R), rn(c.R, D)
        else:
            c.v_idx, N = v_index(vkind, M, g)
            c.V = rn(c.R, N, D) * (0.5 if c.act == "sig" else 1.0)
            if opt.get("coef_idx"):
                c.coef = rn(N, c.R) if integer else torch.rand(N, c.R, generator=g)
                c.coef_idx = torch.randint(0, N, (M,), generator=g)
            else:
                c.coef = rn(M, c.R) if integer else torch.rand(M, c.R, generator=g)
    return c


def row_ref(c, drop_k=None):
    """fp64 pre-activation z, and the sums of moduli of its terms: Tg of the GEMM's products, Tc of the accumulated C
    and the combine terms.  drop_k: the reference with the k-th product of every element left out (a mutant)."""
    A = c.A.double()
    Ar = A[c.a_idx] if c.a_idx is not None else A[:c.M]
    Bm = c.B.double().t() if c.b_trans else c.B.double()
    if drop_k is not None:
        Ar = Ar.clone()
        Ar[:, drop_k] = 0
    z, Tg = Ar @ Bm, Ar.abs() @ Bm.abs()
    Tc = torch.zeros_like(z)
    if c.accumulate:
        z, Tc = z + c.C0.double(), Tc + c.C0.double().abs()
    if c.R:
        rows = torch.arange(c.M)
        cf, Vd = c.coef.double()[rows if c.coef_idx is None else c.coef_idx], c.V.double()
        for r in range(c.R):
            v = Vd[r][None, :] if c.bcast else Vd[r][rows if c.v_idx is None else c.v_idx]
            t = cf[:, r:r + 1] * v
            z, Tc = z + t, Tc + t.abs()
    return z, Tg, Tc


def row_expect(c, b3, ref=None):
    """(reference, bound) of family C for the case, in the arithmetic of the kernel that runs (b3: the bf16x3 kernel)."""
    z, Tg, Tc = row_ref(c) if ref is None else ref
    n = (6 if b3 else 1) * c.D + int(c.accumulate) + c.R + (3 if c.act == "dsig" else 0)
    bz = (gam_e(n, MFMA_ADD) + DROP3 if b3 else gam_e(n, U)) * (Tg + Tc)
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, bz * s
    if c.act == "sig":
        assert float(z.abs().max()) < 8.0, "a saturated pre-activation"
        return sigmoid_bar(z, bz)
    return z, bz


def row_exact(c):
    """Family A: the exact result; asserts that every partial sum of moduli stays below 2^24 (x 3 for the 3/16)."""
    z, Tg, Tc = row_ref(c)
    assert z.numel() == 0 or float((Tg + Tc).max()) * 3 < LIM, "integer case leaves the exact range of fp32"
    if c.act == "dsig":
        z = z * (c.aux.double() * (1 - c.aux.double()))
    assert bool((z.float().double() == z).all())
    return z


def row_single_bound(c, b3):
    """Family B: every GEMM element is one product a b (Tg = |a b|): one rounding (exact) or B3_SINGLE (bf16x3), then
    the epilogue's roundings: 3 for sigma', R fused multiply-adds for the linear combine."""
    z, Tg, Tc = row_ref(c)
    base = B3_SINGLE if b3 else U
    if c.act == "dsig":
        s = c.aux.double() * (1 - c.aux.double())
        return z * s, s * Tg * (base * (1 + gam(3)) + gam(3))
    return z, base * Tg + gam(c.R) * (Tg * (1 + base) + Tc)


def emul_row32(c, b3):
    """The operation in fp32 torch on the CPU; b3: split3 by .to(bfloat16), the six kept products, summed in fp64."""
    A = c.A[c.a_idx] if c.a_idx is not None else c.A[:c.M]
    Bm = c.B.t() if c.b_trans else c.B
    z = six_products(A, Bm).float() if b3 else A @ Bm
    if c.accumulate:
        z = z + c.C0
    if c.R:
        rows = torch.arange(c.M)
        cf = c.coef[rows if c.coef_idx is None else c.coef_idx]
        for r in range(c.R):           # fmaf as the kernels' epilogues: the fp32 x fp32 product is exact in fp64
            v = c.V[r][None, :] if c.bcast else c.V[r][rows if c.v_idx is None else c.v_idx]
            z = (z.double() + cf[:, r:r + 1].double() * v.double()).float()
    if c.act == "dsig":
        z = z * (c.aux * (1.0 - c.aux))
    elif c.act == "sig":
        z = 1.0 / (1.0 + torch.exp(-z))
    return z


def split3(x):
    b0 = x.to(torch.bfloat16).float()
    r1 = x - b0
    b1 = r1.to(torch.bfloat16).float()
    b2 = r1 - b1
    assert bool((b2.to(torch.bfloat16).float() == b2).all()), "the third piece is not a bf16 value"
    assert bool(((b0.double() + b1.double() + b2.double()) == x.double()).all()), "the split is not exact"
    return b0.double(), b1.double(), b2.double()


def six_products(A, Bm, drop=None):
    """sum_k of a0 w0 + a0 w1 + a1 w0 + a1 w1 + a0 w2 + a2 w0 in fp64 (A: rows x k, Bm: k x columns); drop: one
    (i, j) piece product left out."""
    a, w = split3(A), split3(Bm)
    return sum(a[i] @ w[j] for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)) if (i, j) != drop)


def run_row(c, dev, precision, kid, what):
    """One rowgemm into a NaN-guarded C after asserting the kernel id; returns the CPU copy of C."""
    whole, C = guarded(dev, c.M, c.D)
    kw = dict(b_trans=c.b_trans, accumulate=c.accumulate, precision=precision, M=c.M)
    if c.accumulate:
        C.copy_(c.C0)
    if c.act == "dsig":
        if c.alias:
            C.copy_(c.aux)
        kw.update(act=L.ACT_DSIGMOID, aux=C if c.alias else c.aux.to(dev))
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
    A, B = c.A.to(dev), c.B.to(dev)
    got = ops.rowgemm_kernel_id(A, B, C, **kw)
    assert got == kid, f"{what}: kernel id {got}, the case names {kid}"
    ops.rowgemm(A, B, C, **kw)
    out = C.cpu()
    guard_intact(whole, what)
    return out


def is_b3(kid):
    """The kernel id names the bf16x3 row GEMM (500 + 10 NV + aux (+ 2)); 300-series, 100 and 4300 are exact f32."""
    return 500 <= kid < 600


def _precisions(form, D):
    return [p for p in ("exact", "exact4", "bf16x3") if p in ALL_FORMS[form][1]] if D == 256 else ["exact"]


def _vkinds(form, M):
    if ALL_FORMS[form][0].get("vmode") != "gather":
        return ("sorted",)
    return VKINDS if M <= 785 else ("identity", "runs13")


# ---- family A ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [256, 128, 64, 32])
@pytest.mark.parametrize("form", list(ROW_FORMS))
def test_rowgemm_exact_integers_bitwise(form, D, cuda):
    """Family A, every form x M x v_idx pattern x precision (D = 256: exact, exact4 where the form exists, bf16x3;
    narrower widths: the register kernel): bitwise the integer reference, the guard row untouched, the kernel id
    the one the form names."""
    for M in ROW_MS:
        for vk in _vkinds(form, M):
            c = row_case(D, M, form, "int", vk)
            ref = row_exact(c)
            for prec in _precisions(form, D):
                kid = ALL_FORMS[form][1][prec] if D == 256 else 100
                what = f"rowgemm[{prec}:{kid}] {form} int D{D} M{M} {vk}"
                assert_bitwise(run_row(c, cuda, prec, kid, what), ref, what)


@gpu
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 8])
def test_rowgemm_gathered_row_addressing(R, cuda):
    """A = 0 and a one-hot coefficient 1.0 in relation r: the linear output row is bitwise V[r][v_idx[e]] (full-mantissa
    V: 0 + 1 v is exact, 0 v' adds nothing), for every r < R, every v_idx pattern (runs13 / identity / random: more than
    7 distinct rows per relation per tile, the rows read from L2; random: 32 unsorted distinct rows), M = 33 and 785,
    the exact kernel (v3; D = 64: the register kernel) and, R <= 2, the bf16x3 kernel."""
    form = f"gather_R{R}"
    for D, M in ((256, 785), (256, 33), (64, 785)):
        for vk in VKINDS:
            g = _gen(R, D, M, VKINDS.index(vk))
            c = row_case(D, M, form, "int", vk)
            c.A.zero_()
            c.V = torch.randn(c.V.shape, generator=g)
            rows = torch.arange(M) if c.v_idx is None else c.v_idx
            if vk in ("runs13", "identity", "random"):
                assert max(len(set(rows[t:t + 32].tolist())) for t in range(0, M, 32)) > (7 if vk == "runs13" else 31)
            for r in range(R):
                c.coef = torch.zeros(M, R)
                c.coef[:, r] = 1.0
                for prec in (_precisions(form, D) if R <= 2 else ["exact"]):
                    kid = ALL_FORMS[form][1][prec] if D == 256 else 100
                    what = f"rowgemm[{prec}:{kid}] one-hot r{r} of R{R} D{D} M{M} {vk}"
                    assert_bitwise(run_row(c, cuda, prec, kid, what), c.V[r][rows].double(), what)


def _batch_entry(c, dev, precision):
    whole, C = guarded(dev, c.M, c.D)
    kw = dict(b_trans=c.b_trans, accumulate=c.accumulate, precision=precision, M=c.M)
    if c.accumulate:
        C.copy_(c.C0)
    if c.act == "dsig":
        kw.update(act=L.ACT_DSIGMOID, aux=c.aux.to(dev))
    if c.R:
        kw.update(coef=c.coef.to(dev), V=c.V.to(dev), v_rel_stride=c.V.shape[1] * c.D,
                  v_idx=None if c.v_idx is None else c.v_idx.to(I32).to(dev))
    return whole, (c.A.to(dev), c.B.to(dev), C, kw)


@gpu
@pytest.mark.parametrize("D,precision", [(256, "exact"), (256, "bf16x3"), (64, "exact")])
@pytest.mark.parametrize("mix", ["forms", "one_variant"])
def test_rowgemm_batched_exact_integers_bitwise(mix, D, precision, cuda):
    """rowgemm_batched, family A: a batch mixing forms and row counts (one entry M = 1; D = 256: one call per entry,
    D = 64: one launch) and a batch of one v3 variant (D = 256 exact: ONE launch, blockIdx.y = entry; an empty entry
    among them): each entry bitwise its integer reference, each guard row intact."""
    spec = [("plain", 785), ("accumulate", 1), ("gather_R2", 33), ("dsig", 31), ("b_trans", 4097)] if mix == "forms" \
        else [("plain", 785), ("b_trans", 1), ("plain", 0), ("b_trans", 33), ("plain", 4097)]
    cases = [row_case(D, M, form, "int", "runs13") for form, M in spec]
    refs = [row_exact(c) for c in cases]
    wholes, calls = zip(*[_batch_entry(c, cuda, precision) for c in cases])
    ops.rowgemm_batched(list(calls))
    for c, ref, w, call in zip(cases, refs, wholes, calls):
        what = f"rowgemm_batched[{precision}] {mix} entry {c.form} D{D} M{c.M}"
        assert_bitwise(call[2], ref, what)
        guard_intact(w, what)


# ---- family B ---------------------------------------------------------------------------------------------
SINGLE_FORMS = ("plain", "b_trans", "dsig", "gather_R1", "gather_R2", "gather_R8")


@gpu
@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("form", SINGLE_FORMS)
def test_rowgemm_single_term(form, D, cuda):
    """Family B: A row e non-zero only in column e mod D, M = 2 D + 17 (every k live in more than one tile position):
    each GEMM element one product of full-mantissa values.  Exact kernels within u |a b| (+ the epilogue's roundings),
    bf16x3 within B3_SINGLE |a b|: a missing low piece product (2^-16 |a b|) is 20 bounds away."""
    M = 2 * D + 17
    c = row_case(D, M, form, "single", "runs13")
    for prec in _precisions(form, D):
        kid = ALL_FORMS[form][1][prec] if D == 256 else 100
        what = f"rowgemm[{prec}:{kid}] {form} single D{D} M{M}"
        ref, bound = row_single_bound(c, is_b3(kid))
        assert_within(run_row(c, cuda, prec, kid, what), ref, bound, what)


# ---- family C ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("form", list(ALL_FORMS))
def test_rowgemm_dense_per_element(form, D, cuda):
    """Family C: dense operands, every element against (gamma_e(n) + DROP) T of its own terms; the activation forms
    with the bound carried through the sigmoid (S / 16: |z| < 8, nothing saturated)."""
    for M in (1, 33, 785):
        c = row_case(D, M, form, "dense", "runs13" if M != 33 else "random")
        ref = row_ref(c)
        for prec in _precisions(form, D):
            kid = ALL_FORMS[form][1][prec] if D == 256 else 100
            what = f"rowgemm[{prec}:{kid}] {form} dense D{D} M{M}"
            assert_within(run_row(c, cuda, prec, kid, what), *row_expect(c, is_b3(kid), ref), what)


# ---- CPU self-checks of the row bars -------------------------------------------------------------------------
def _neighbour_rows(c):
    """The case with one gathered row replaced by its neighbour in the table."""
    m = SimpleNamespace(**vars(c))
    rows = torch.arange(c.M) if c.v_idx is None else c.v_idx.clone()
    e = c.M // 2
    rows[e] = rows[e] + 1 if int(rows[e]) + 1 < c.V.shape[1] else rows[e] - 1
    m.v_idx = rows
    return m, e


@pytest.mark.parametrize("form", list(ROW_FORMS))
def test_selfcheck_rowgemm_integer_reference(form):
    """Family A on the CPU: fp32 torch (any order) is bitwise the reference; a dropped k term, a neighbour's gathered
    row and a last ragged tile left at its sentinel are each refused."""
    D, M = 64, 785
    c = row_case(D, M, form, "int", "runs13")
    ref = row_exact(c)
    assert_bitwise(emul_row32(c, False), ref, f"cpu-fp32 {form}")
    assert_bitwise(emul_row32(c, True), ref, f"cpu bf16x3 emulation {form}")      # integers: pieces 1 and 2 are zero
    z = row_ref(c, drop_k=D - 1)[0]
    with pytest.raises(AssertionError):
        assert_bitwise((z * (c.aux.double() * (1 - c.aux.double())) if c.act == "dsig" else z).float(), ref, "dropped k")
    cand = ref.float().clone()
    cand[M - M % 32:] = NAN
    with pytest.raises(AssertionError):
        assert_bitwise(cand, ref, "ragged tile at its sentinel")
    if c.R and not c.bcast:
        m, e = _neighbour_rows(c)
        with pytest.raises(AssertionError):
            assert_bitwise(row_exact(m).float(), ref, "neighbour row")


@pytest.mark.parametrize("b3", [False, True])
@pytest.mark.parametrize("form", ["plain", "accumulate", "dsig", "gather_R2", "gather_R8", "bcast_R2_dsig", "a_idx",
                                  "plain_sig", "gather_R2_sig", "gather_R8_sig", "coef_idx_sig"])
def test_selfcheck_rowgemm_dense_bound(form, b3):
    """Family C on the CPU: the fp32 evaluation (b3: the six-product emulation) inside the bound; refused: one k term
    dropped, one gathered row replaced by its neighbour, the last ragged tile left at NaN."""
    D, M = 256, 81
    c = row_case(D, M, form, "dense", "runs13")
    ref, bound = row_expect(c, b3)
    assert_within(emul_row32(c, b3), ref, bound, f"cpu {'bf16x3 emulation' if b3 else 'fp32'} {form} dense")
    mut = row_expect(c, b3, row_ref(c, drop_k=7))[0]
    assert rejects(mut, ref, bound), "a dropped k term passes"
    frac = float(((mut - ref).abs() > bound).double().mean())
    print(f"COVER {form} b3={b3}: a dropped k term is refused on {100 * frac:.0f}% of the elements")
    assert frac > 0.5
    cand = ref.clone()
    cand[M - M % 32:] = NAN
    assert refuses(cand, ref, bound)
    if c.R and not c.bcast:
        m, e = _neighbour_rows(c)
        mut = row_expect(m, b3)[0]
        assert rejects(mut, ref, bound) and not rejects(mut[:e], ref[:e], bound[:e]), "a neighbour's row passes"


def test_selfcheck_constants():
    # the CPU figure of the bf16x3 row bound at D = 256 with one accumulate and one combine term; B3_SINGLE ~ 12 u
    assert abs(gam_e(6 * 256 + 2, MFMA_ADD) + DROP3 - 1.83e-4) < 1e-6
    assert 12 * U < B3_SINGLE < 12.2 * U
    assert 20 * B3_SINGLE < 2.0 ** -16             # a missing low piece product (~2^-16 |a b|) is twenty bounds out


@pytest.mark.parametrize("form", SINGLE_FORMS)
def test_selfcheck_rowgemm_single_term_bound(form):
    """Family B on the CPU: fp32 torch inside the exact bar; the six-product emulation inside the bf16x3 bar at a
    fraction of the truncation term; each low piece product dropped is refused on most elements; a dropped k term
    (one output column of zeros per row group) is refused."""
    D = 64
    M = 2 * D + 17
    c = row_case(D, M, form, "single", "runs13")
    ref, bound = row_single_bound(c, False)
    assert_within(emul_row32(c, False), ref, bound, f"cpu-fp32 {form} single")
    ref3, bound3 = row_single_bound(c, True)
    assert_within(emul_row32(c, True), ref3, bound3, f"cpu bf16x3 emulation {form} single")
    zero_k = SimpleNamespace(**vars(c))
    zero_k.A = c.A.clone()
    zero_k.A[:, 5] = 0
    assert rejects(emul_row32(zero_k, False), ref, bound) and rejects(emul_row32(zero_k, True), ref3, bound3)
    if form in ("plain", "b_trans"):
        Bm = c.B.t() if c.b_trans else c.B
        full = six_products(c.A, Bm)
        trunc = (full - ref3).abs() / (2 * U * ref3.abs()).clamp_min(1e-300)
        print(f"COVER {form}: six-product truncation at most {float(trunc.max()):.3f} of 2 u |a b|")
        for drop in ((0, 2), (2, 0), (1, 1)):
            out = ((six_products(c.A, Bm, drop=drop) - ref3).abs() > bound3).double().mean()
            print(f"COVER {form}: dropping a{drop[0]} w{drop[1]} puts {100 * float(out):.0f}% of the elements out of bound")
            assert float(out) > 0.5


# =============================================================================================================
# TN GEMM, gemm_tn_batched, sigma_tn
# =============================================================================================================
def first_m(pred):
    M = 1
    while not pred(M):
        M += 1
    return M


def spread_rows(M, D):
    """pi(i): the row of column i's single non-zero: spread over all rows, the first and the last (ragged) included."""
    pi = (torch.arange(D) * M) // D
    pi[D - 1] = M - 1
    return pi


def tn_case(D, M, kind, acc, seed=0):
    g = _gen(D, M, len(kind), int(acc), seed)
    c = SimpleNamespace(D=D, M=M, acc=acc, kind=kind, pi=None)
    if kind == "int":
        c.A, c.B, c.C0 = ints(g, M, D), ints(g, M, D), ints(g, D, D)
    elif kind == "single":
        c.pi = spread_rows(M, D)
        c.A = torch.zeros(M, D)
        c.A[c.pi, torch.arange(D)] = torch.randn(D, generator=g)
        c.B, c.C0 = torch.randn(M, D, generator=g), torch.zeros(D, D)
    else:
        c.A, c.B, c.C0 = torch.rand(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(D, D, generator=g)
    return c


def tn_ref(c, drop_row=None):
    A, B = c.A.double(), c.B.double()
    if drop_row is not None:
        A = A.clone()
        A[drop_row] = 0
    z, T = A.t() @ B, A.abs().t() @ B.abs()
    if c.acc:
        z, T = z + c.C0.double(), T + c.C0.double().abs()
    return z, T


def tn_exact(c):
    z, T = tn_ref(c)
    assert float(T.max()) < LIM, "integer case leaves the exact range of fp32"
    return z


def tn_bound(c, T, b3, n_partials):
    """Family C: M products (6 M piece products) per element, the slab partials summed, the accumulated C."""
    n = (6 if b3 else 1) * c.M + n_partials + int(c.acc)
    return (gam_e(n, MFMA_ADD) + DROP3 if b3 else gam_e(n, U)) * T


def tn_single_bound(c, T, b3):
    return (B3_SINGLE if b3 else U) * T


def run_tn(c, dev, precision, what):
    D = c.D
    slab = torch.full((ops.tn_blocks(c.M, D) * D * D,), NAN, device=dev)
    whole, C = guarded(dev, D, D)
    if c.acc:
        C.copy_(c.C0)
    ops.gemm_tn(c.A.to(dev), c.B.to(dev), C, slab, accumulate=c.acc, precision=precision)
    out = C.cpu()
    guard_intact(whole, what)
    return out


TN_MODES = [(256, "exact"), (256, "bf16x3"), (64, "exact"), (32, "exact")]


@gpu
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("D,precision", TN_MODES)
def test_gemm_tn_exact_integers_bitwise(D, precision, acc, cuda):
    """Family A: C (+)= A^T B bitwise the integer reference from a NaN-filled slab into a NaN-guarded C, for M around
    the 16- and 32-row tiles, several blocks with a ragged last one, and the smallest M with three slab partials."""
    m3 = first_m(lambda m: ops.tn_blocks(m, D) >= 3)
    assert ops.tn_blocks(m3 - 1, D) == 2
    for M in TN_MS + (m3,):
        c = tn_case(D, M, "int", acc)
        what = f"gemm_tn[{precision}] int D{D} M{M} acc{int(acc)}"
        assert_bitwise(run_tn(c, cuda, precision, what), tn_exact(c), what)


@gpu
@pytest.mark.parametrize("D,precision", TN_MODES)
def test_gemm_tn_batched_exact_integers_bitwise(D, precision, cuda):
    """Family A: four entries of different M, one empty, accumulate mixed, one NaN-filled slab: each C bitwise its
    reference (the empty entry: zeros, or its old C when accumulating), each guard intact; both orders of the
    accumulate flags, so the empty entry meets both."""
    for flip in (False, True):
        cases = [tn_case(D, M, "int", (k % 2 == 1) != flip, seed=9) for k, M in enumerate((785, 33, 0, 4097))]
        slab = torch.full((sum(max(1, ops.tn_blocks(c.M, D)) for c in cases) * D * D,), NAN, device=cuda)
        wholes, ents = [], []
        for c in cases:
            w, C = guarded(cuda, D, D)
            if c.acc:
                C.copy_(c.C0)
            wholes.append(w)
            ents.append((c.A.to(cuda), c.B.to(cuda), C, c.acc))
        ops.gemm_tn_batched(ents, slab, precision=precision)
        for c, w, e in zip(cases, wholes, ents):
            what = f"gemm_tn_batched[{precision}] int D{D} entry M{c.M} acc{int(c.acc)}"
            assert_bitwise(e[2], tn_exact(c), what)
            guard_intact(w, what)


@gpu
@pytest.mark.parametrize("D,precision", TN_MODES)
def test_gemm_tn_single_term(D, precision, cuda):
    """Family B: column i of A non-zero only in row pi(i), the rows spread over every block and the ragged last tile:
    C[i][j] = A[pi(i)][i] B[pi(i)][j], one product per element."""
    for M in (785, 4097):
        c = tn_case(D, M, "single", False)
        z, T = tn_ref(c)
        what = f"gemm_tn[{precision}] single D{D} M{M}"
        assert_within(run_tn(c, cuda, precision, what), z, tn_single_bound(c, T, precision == "bf16x3"), what)


@gpu
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("D,precision", TN_MODES)
def test_gemm_tn_dense_per_element(D, precision, acc, cuda):
    """Family C at short M only (a wrong term must be larger than the bound); the long sums are families A and B."""
    for M in SHORT_MS:
        c = tn_case(D, M, "dense", acc)
        z, T = tn_ref(c)
        what = f"gemm_tn[{precision}] dense D{D} M{M} acc{int(acc)}"
        assert_within(run_tn(c, cuda, precision, what), z, tn_bound(c, T, precision == "bf16x3", ops.tn_blocks(M, D)), what)


def test_selfcheck_tn_bounds():
    D = 64
    for M in (1, 17, 257):                       # family A and C on the CPU
        ci = tn_case(D, M, "int", True)
        assert_bitwise((ci.A.t() @ ci.B + ci.C0), tn_exact(ci), f"cpu-fp32 tn int M{M}")
        c = tn_case(D, M, "dense", True)
        z, T = tn_ref(c)
        nb = (M + 31) // 32
        assert_within(c.A.t() @ c.B + c.C0, z, tn_bound(c, T, False, nb), f"cpu-fp32 tn dense M{M}")
        assert_within(six_products(c.A.t().contiguous(), c.B).float() + c.C0, z, tn_bound(c, T, True, nb),
                      f"cpu bf16x3 emulation tn dense M{M}")
        for b3 in (False, True):
            assert rejects(tn_ref(c, drop_row=M - 1)[0], z, tn_bound(c, T, b3, nb)), "a dropped row passes"
    with pytest.raises(AssertionError):
        assert_bitwise(tn_ref(ci, drop_row=256)[0].float(), tn_exact(ci), "dropped row")
    # family B: one row of the last block dropped: the columns whose single term lives there go to zero
    c = tn_case(D, 785, "single", False)
    z, T = tn_ref(c)
    assert bool(((c.A != 0).sum(0) == 1).all()) and int(c.pi[-1]) == 784 and int(c.pi[0]) == 0
    assert len(set((c.pi // 32).tolist())) == (785 + 31) // 32          # every 32-row tile holds a live row
    for b3 in (False, True):
        bound = tn_single_bound(c, T, b3)
        emul = six_products(c.A.t().contiguous(), c.B) if b3 else c.A.t() @ c.B
        assert_within(emul.float(), z, bound, f"cpu tn single b3={b3}")
        assert rejects(tn_ref(c, drop_row=784)[0], z, bound)
    for drop in ((0, 2), (2, 0), (1, 1)):
        assert rejects(six_products(c.A.t().contiguous(), c.B, drop=drop), z, tn_single_bound(c, T, True))


# ---- sigma_tn -------------------------------------------------------------------------------------------------
def stn_case(M, kind):
    D = 256
    g = _gen(M, len(kind), 31)
    c = SimpleNamespace(D=D, M=M, kind=kind, pi=None)
    if kind == "int":
        c.X = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (M, D), generator=g)]
        c.dO, c.S = ints(g, M, D), ints(g, D, D)
    else:
        c.X = 0.05 + 0.9 * torch.rand(M, D, generator=g)
        c.dO, c.S = torch.randn(M, D, generator=g), torch.randn(D, D, generator=g) / 16
        if kind == "single":
            c.pi = spread_rows(M, D)
            keep = torch.zeros(M, D, dtype=torch.bool)
            keep[c.pi, torch.arange(D)] = True
            c.X = torch.where(keep, c.X, torch.zeros(()))
    return c


def stn_ref(c):
    """dS = X^T dO and dX = (dO S^T) x (1 - x) in fp64, with the sums of moduli of their terms."""
    X, dO, S = c.X.double(), c.dO.double(), c.S.double()
    s = X * (1 - X)
    return {"dS": (X.t() @ dO, X.abs().t() @ dO.abs()), "dX": ((dO @ S.t()) * s, (dO.abs() @ S.abs().t()) * s)}


def run_stn(c, dev, what):
    D = c.D
    nfl = ops.sigma_tn_slab_floats(c.M)
    slab = torch.full((nfl,), NAN, device=dev)
    wS, dS = guarded(dev, D, D)
    wX, X = guarded(dev, c.M, D)
    X.copy_(c.X)
    ops.sigma_tn(c.dO.to(dev), X, c.S.to(dev), dS, slab, precision="bf16x3")
    out = {"dS": dS.cpu(), "dX": X.cpu()}
    guard_intact(wS, what + " dS")
    guard_intact(wX, what + " dX")
    return out, nfl // (D * D)


@gpu
def test_sigma_tn_exact_integers_bitwise(cuda):
    """Family A on fp32 tables: dX (over X) and dS both bitwise, slab and dS prefilled with NaN; M = 0 gives dS = 0.
    sigma_tn_slab_floats counts ranges in multiples of 8 (8 for every M here, M = 0 included: ranges without rows write
    zero partials), so the smallest M with three ranges THAT HOLD ROWS (three 32-row tiles) is added."""
    m3 = first_m(lambda m: ops.sigma_tn_slab_floats(m) >= 3 * 256 * 256 and (m + 31) // 32 >= 3)
    for M in (0, 1, 31, 33, 785, 4097, m3):
        c = stn_case(M, "int")
        refs = stn_ref(c)
        assert float(refs["dS"][1].max() if M else 0) < LIM and float(refs["dX"][1].max() if M else 0) * 16 < LIM
        out, _ = run_stn(c, cuda, f"sigma_tn int M{M}")
        for k in ("dS", "dX"):
            assert_bitwise(out[k], refs[k][0], f"sigma_tn[bf16x3] int M{M} {k}")


@gpu
def test_sigma_tn_single_term_and_dense(cuda):
    """Family B (X column i non-zero only in row pi(i): dS one product per element) at long M, and family C at short
    M: dS within (gamma_e(6 M + ranges) + DROP) T, dX within the bf16x3 row bound of its sigma' form."""
    for kind, Ms in (("single", (785, 4097)), ("dense", SHORT_MS)):
        for M in Ms:
            c = stn_case(M, kind)
            refs = stn_ref(c)
            out, nr = run_stn(c, cuda, f"sigma_tn {kind} M{M}")
            bS = B3_SINGLE * refs["dS"][1] if kind == "single" else (gam_e(6 * M + nr, MFMA_ADD) + DROP3) * refs["dS"][1]
            assert_within(out["dS"], refs["dS"][0], bS, f"sigma_tn[bf16x3] {kind} M{M} dS")
            assert_within(out["dX"], refs["dX"][0], (gam_e(6 * 256 + 3, MFMA_ADD) + DROP3) * refs["dX"][1],
                          f"sigma_tn[bf16x3] {kind} M{M} dX")


def test_selfcheck_sigma_tn_bounds():
    for M in (1, 33, 257):
        ci = stn_case(M, "int")
        ri = stn_ref(ci)
        assert_bitwise(ci.X.t() @ ci.dO, ri["dS"][0], "cpu-fp32 sigma_tn int dS")
        assert_bitwise((ci.dO @ ci.S.t()) * (ci.X * (1 - ci.X)), ri["dX"][0], "cpu-fp32 sigma_tn int dX")
        c = stn_case(M, "dense")
        refs = stn_ref(c)
        bS = (gam_e(6 * M + 8, MFMA_ADD) + DROP3) * refs["dS"][1]
        bX = (gam_e(6 * 256 + 3, MFMA_ADD) + DROP3) * refs["dX"][1]
        assert_within(six_products(c.X.t().contiguous(), c.dO).float(), refs["dS"][0], bS, "cpu emulation sigma_tn dS")
        assert_within(six_products(c.dO, c.S.t().contiguous()).float() * (c.X * (1 - c.X)), refs["dX"][0], bX,
                      "cpu emulation sigma_tn dX")
        m = SimpleNamespace(**vars(c))
        m.dO = c.dO.clone()
        m.dO[M - 1] = 0                              # the last row dropped from both products
        assert rejects(stn_ref(m)["dS"][0], refs["dS"][0], bS) and rejects(stn_ref(m)["dX"][0], refs["dX"][0], bX)
    c = stn_case(785, "single")
    refs = stn_ref(c)
    assert bool(((c.X != 0).sum(0) == 1).all())
    assert_within(six_products(c.X.t().contiguous(), c.dO).float(), refs["dS"][0], B3_SINGLE * refs["dS"][1],
                  "cpu emulation sigma_tn single dS")
    assert rejects(six_products(c.X.t().contiguous(), c.dO, drop=(1, 1)), refs["dS"][0], B3_SINGLE * refs["dS"][1])


# =============================================================================================================
# combine
# =============================================================================================================
def comb_case(D, M, R, mode):
    """mode: "run" (y_idx is v_idx, per-edge coefficients: the D = 256 run kernel), "generic" (three index arrays),
    "noidx" (dense rows)."""
    g = _gen(D, M, R, len(mode), 77)
    N = M if mode == "noidx" else max(2, M // 3)
    c = SimpleNamespace(D=D, M=M, R=R, mode=mode, N=N, Y=torch.randn(N, D, generator=g),
                        V=torch.randn(R, N, D, generator=g) * 0.5, y_idx=None, v_idx=None, coef_idx=None)
    if mode == "run":
        c.y_idx = c.v_idx = torch.randint(0, N, (M,), generator=g).sort().values
    elif mode == "generic":
        c.y_idx, c.v_idx, c.coef_idx = (torch.randint(0, N, (M,), generator=g) for _ in range(3))
    c.coef = torch.rand(N if mode == "generic" else M, R, generator=g)
    return c


def comb_ref(c):
    """z = Y + sum_r coef V_r: R products and R adds on the longest path (a multiply-add may or may not be fused)."""
    rows = torch.arange(c.M)
    sel = lambda i: rows if i is None else i                                   # noqa: E731
    z = c.Y.double()[sel(c.y_idx)]
    T = z.abs()
    cf = c.coef.double()[sel(c.coef_idx)]
    for r in range(c.R):
        t = cf[:, r:r + 1] * c.V.double()[r][sel(c.v_idx)]
        z, T = z + t, T + t.abs()
    assert float(z.abs().max()) < 8.0
    return sigmoid_bar(z, gam(2 * c.R) * T)


COMB_CASES = [(256, 0, "run"), (256, 2, "run"), (256, 8, "run"), (256, 3, "generic"), (256, 2, "noidx"), (64, 0, "noidx"),
              (64, 2, "generic"), (32, 8, "generic"), (128, 1, "run")]


@gpu
@pytest.mark.parametrize("D,R,mode", COMB_CASES)
def test_combine_per_element(D, R, mode, cuda):
    for M in (1, 63, 65, 785):
        c = comb_case(D, M, R, mode)
        whole, out = guarded(cuda, M, D)
        ix = {k: None if getattr(c, k) is None else getattr(c, k).to(I32).to(cuda) for k in ("y_idx", "v_idx", "coef_idx")}
        if mode == "run":
            ix["v_idx"] = ix["y_idx"]
        ops.combine(c.Y.to(cuda), c.coef.to(cuda), c.V.to(cuda), out, **ix)
        what = f"combine {mode} D{D} R{R} M{M}"
        guard_intact(whole, what)
        assert_within(out, *comb_ref(c), what)


def test_selfcheck_combine_bound():
    for D, R, mode in COMB_CASES:
        c = comb_case(D, 65, R, mode)
        ref, bound = comb_ref(c)
        rows = torch.arange(c.M)
        sel = lambda i: rows if i is None else i                               # noqa: E731
        z = c.Y[sel(c.y_idx)]
        for r in range(R):
            z = z + c.coef[sel(c.coef_idx)][:, r:r + 1] * c.V[r][sel(c.v_idx)]
        assert_within(1.0 / (1.0 + torch.exp(-z)), ref, bound, f"cpu-fp32 combine {mode} D{D} R{R}")
        m = SimpleNamespace(**vars(c))
        m.y_idx = sel(c.y_idx).clone()
        m.y_idx[7] = (m.y_idx[7] + 1) % c.N                  # one Y row replaced by its neighbour
        assert rejects(comb_ref(m)[0], ref, bound)
        if R:
            m = SimpleNamespace(**vars(c))
            m.V = c.V.clone()
            m.V[R - 1] = 0                                   # the last relation's term dropped
            assert rejects(comb_ref(m)[0], ref, bound)


def test_selfcheck_old_bars_replayed():
    """The figures of the module docstring: the max-norm limits of tests/test_gpu_kernels.py beside max|ref|."""
    g = torch.Generator().manual_seed(7 * 256)
    A, B = torch.randn(1008, 256, generator=g, dtype=F64), torch.randn(256, 256, generator=g, dtype=F64)
    mx = float((A @ B).abs().max())
    print(f"OLD test_rowgemm_plain D256: max|ref| {mx:.3g}, old limit {2e-5 * math.sqrt(256) * (1 + mx):.3g}")
    assert 2e-5 * 16 * (1 + mx) > 1e-2
    g = torch.Generator().manual_seed(17 + 256)
    A, B = torch.randn(5003, 256, generator=g, dtype=F64), torch.randn(5003, 256, generator=g, dtype=F64)
    C = torch.randn(256, 256, generator=g, dtype=F64)
    mx = float((C + A.t() @ B).abs().max())
    print(f"OLD test_gemm_tn D256 M5003: max|ref| {mx:.3g}, old limit {2e-6 * math.sqrt(5003) * (1 + mx):.3g}")
    assert 2e-6 * math.sqrt(5003) * (1 + mx) > 3e-2
    g = torch.Generator().manual_seed(100 + 8 + len("random"))
    A = torch.rand(4096, 256, generator=g, dtype=F64)
    S = torch.randn(256, 256, generator=g, dtype=F64)
    z = A @ S
    sat = float(((torch.sigmoid(z) < 2e-5) | (torch.sigmoid(z) > 1 - 2e-5)).double().mean())
    print(f"OLD sigmoid forward, A ~ U(0,1), S ~ N(0,1): std z {float(z.std()):.2f}, {100 * sat:.0f}% within 2e-5 of 0 / 1")
    assert float(z.std()) > 8
