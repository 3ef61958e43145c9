"""Per-element, derived bars for the exact-f32 kernels of a training step.

Every GPU test here compares a HIP kernel with an fp64 evaluation of the same operation on the same fp32 inputs,
element by element, against a bound built from the reference's own terms by standard fp32 forward-error analysis
(u = 2^-24, gamma(k) = k u / (1 - k u)):

  * a sum of n products or terms accumulated in ANY order:  gamma(n + c) * sum_i |term_i|, c = the roundings of a term
    besides the adds (its multiplies, a trailing x (1 - x) factor, one more add for accumulate).  Padding with exact
    zeros (slot / lane / block partials of lanes that own no term) adds nothing: x + 0 is exact;
  * an elementwise chain of k roundings: gamma(k) * (sum of |intermediate terms|) where the chain subtracts;
  * a transcendental: its documented worst-case ulp count, propagated through the rest of the chain by the fp64
    derivative (or, where the function is monotone, by evaluating it at both ends of the allowed interval).

ULP allowances (the only non-derived numbers; none is measured): the kernels under test call expf, logf, sqrtf and
the IEEE `/` of the ROCm device library, which implements the OpenCL C precision contract (OpenCL C specification,
"Relative error as ULPs": exp <= 3 ulp, log <= 3 ulp, sqrt <= 3 ulp, x / y <= 2.5 ulp; the HIP math API page reports
1 ulp for expf and logf, and hipcc rounds fp32 `/` and sqrtf correctly by default, so the allowances are upper
bounds).  One ulp is at most 2 u relative.  None of these kernels calls sigmoid_fast (__expf + v_rcp_f32: the layer
activations of the row GEMMs and combine only), so the measured allowance the design notes mention is not needed here.

What the bars replace (the reference side of tests/test_gpu_kernels.py replayed in fp64, same seeds and shapes; its
helper allows tol (1 + max|ref|) on every element):
    distmult do (D = 32 / 256)   max|ref| 8.4e-8 / 1.3e-7   old limit 1.0e-4   (an all-zero do passed)
    distmult drel                max|ref| 3.2e-5 / 3.0e-5   old limit 1.0e-4   (an all-zero drel passed)
    distmult logits              [-4.2, 4.4]: the BCE clip branch never ran
    adam v                       max|ref| 1.0015e-6          old limit 1.0e-6   (an unchanged or zero v passed)
    adam m                       max|ref| 3.7e-3             old limit 1.0e-6
    adam var                     max|update| 2.1e-2          old limit 4.8e-6
Worst observed |err| / bound on an MI355X over all cases of each test (1 = at the bound):
    distmult_bce / _heads: s 0.048, p 0.22, ds 0.24, do 0.36, drel 0.077, loss 0.023, dXh 0.27; prediction seed: ds
    0.57, do 0.49, dXh 0.18, drel 0.018, loss 0.003; adam: m 0.97, v 0.62, var 0.97; tail_seg_reduce: dP 0.66, dsum
    0.66, dWedge 0.043; seg_gather_reduce 0.66; head_bwd_node: dz 0.036, dP 0.50, dsum 1.0 (one add: half an ulp);
    head_dz 0.30; head_wsum 0.57; reduce_slabs: plain 0.50, slabs4 0.33, split 0.074; alpha_fwd: S 0.14, W 0.17;
    spmm_csr 0.60; sddmm_csr 0.041; gemm_tn_narrow: dWa 0.49, dba 0.39.
The ratios far below 1 belong to the long sums (the loss over T = 7001 edges 0.003-0.02, drel, the narrow TN at
M = 9001: 1.2e-5 there, 0.49 at M = 1): the order-independent bound grows like n u while the rounding errors of a
sum of n terms of mixed rounding direction grow like sqrt(n) u, and the kernels sum in short chains (<= 16 rows
per block in the narrow TN).  The bound is kept order-independent on purpose: no slab, slot or butterfly order has
to be mirrored, and at the short lengths (where a dropped or doubled term is what goes wrong) it is within 2-3x.

The tests without the `gpu` mark evaluate each operation in fp32 torch on the CPU with the tests' own input builders
and assert (a) that this sits inside the bound and (b) that the reference with a deliberate error is rejected: one
element off by 1e-3 relative, one relation's rows scaled by (1 + 1e-4), and the last ragged group dropped.
"""
import ctypes
import math

import pytest
import torch

from bounds import NAN, U, assert_within, gam, guard_intact, guarded, rejects, worst_ratio  # noqa: F401
from iddgcn_amd import ops

gpu = pytest.mark.gpu
F64, F32, I32 = torch.float64, torch.float32, torch.int32
EXP_ULP, LOG_ULP, SQRT_ULP, DIV_ULP = 3.0, 3.0, 3.0, 2.5      # OpenCL C "Relative error as ULPs"
ULP = 2.0 * U                                                   # one ulp, relative, at most


def f32c(x):
    """The fp32 value a C float argument / constant holds, as a Python float."""
    return float(torch.tensor(x, dtype=F32))


EPS32 = f32c(1e-7)                                                          # EPS_BCE = 1e-7f
HI32 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(1e-7, dtype=F32))  # 1.0f - 1e-7f as the kernel forms it


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def check_all(got, refs, what, names=None):
    for k in (names or refs):
        assert_within(got[k], refs[k][0], refs[k][1], f"{what} {k}")


def segsum(vals, seg, n):
    return torch.zeros((n, *vals.shape[1:]), dtype=vals.dtype).index_add_(0, seg, vals)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- the self-check's perturbations -------------------------------------------------------------------------
def _pick_element(ref, bound):
    """The element a 1e-3 relative error is tried on: the one of MEDIAN conditioning (|ref| / bound) among the
    nonzero elements if the bar can resolve 1e-3 there, else the best-conditioned one."""
    r, b = ref.flatten().abs(), bound.expand_as(ref).flatten()
    nz = (r > 0).nonzero().flatten()
    if nz.numel() == 0:
        return None
    cond = r[nz] / b[nz].clamp_min(1e-300)
    order = cond.argsort()
    i = int(nz[order[order.numel() // 2]])
    if 1e-3 * float(r[i]) <= float(b[i]):
        i = int(nz[order[-1]])
    return i


def assert_perturbations_rejected(refs, rel_slices, dropped, what):
    """refs: name -> (ref, bound); rel_slices: name -> index expression of one relation's rows; dropped: name -> the
    reference with the last ragged group left out."""
    for name, (ref, bound) in refs.items():
        i = _pick_element(ref, bound)
        if i is None:
            continue
        cand = ref.clone(memory_format=torch.contiguous_format)
        cand.view(-1)[i] *= 1.0 + 1e-3
        assert rejects(cand, ref, bound), f"{what} {name}: one element off by 1e-3 relative passes the bar"
        cov = float(((1e-3 * ref.abs() > bound) & (ref != 0)).double().sum() / max(1, int((ref != 0).sum())))
        print(f"COVER {what} {name}: a 1e-3 relative error is rejected on {100 * cov:.1f}% of the nonzero elements")
    for name, sl in rel_slices.items():
        ref, bound = refs[name]
        cand = ref.clone()
        cand[sl] = cand[sl] * (1.0 + 1e-4)
        assert rejects(cand, ref, bound), f"{what} {name}: one relation's rows scaled by 1 + 1e-4 pass the bar"
    for name, cand in dropped.items():
        ref, bound = refs[name]
        assert rejects(cand, ref, bound), f"{what} {name}: dropping the last ragged group passes the bar"


# =============================================================================================================
# DistMult + BCE
# =============================================================================================================
class DmCase:
    pass


def dm_case(D, R, T, N=120, sat_only=False):
    """Heads skewed as in production's worst case: three hub heads hold half the edges, half the nodes have none.
    About 5% of the edges are SATURATED (fp64 |s| in [22, 32], both labels, both signs); every other fp64 logit has
    |s| <= 7.5; nothing lies in 8 < |s| < 20, so no edge's clip branch depends on the fp32 rounding of p (p leaves
    [1e-7, 1 - 2^-23] at |s| ~ 16.1).  Asserted on the reference in dm_ref."""
    g = _gen(1000 + 7 * D + 13 * R + T + (5 if sat_only else 0))
    c = DmCase()
    c.D, c.R, c.T, c.N = D, R, T, N
    c.Xh = torch.rand(N, D, generator=g) * 0.9 + 0.05
    Xt = torch.rand(T, D, generator=g) * 0.9 + 0.05
    # std of a logit = sqrt(D) sigma sqrt(E a^2 E b^2), E a^2 = 0.3175 for a ~ U(0.05, 0.95): sigma for std ~ 2.5
    c.rel = torch.randn(R, D, generator=g) * (7.9 / math.sqrt(D))
    hub = torch.rand(T, generator=g) < 0.5
    c.h = torch.where(hub, torch.randint(0, 3, (T,), generator=g), torch.randint(0, N // 2, (T,), generator=g))
    c.r = torch.randint(0, R, (T,), generator=g)
    y = (torch.rand(T, generator=g) < 0.5).float()
    s = (c.Xh.double()[c.h] * c.rel.double()[c.r] * Xt.double()).sum(1)
    want = (s.abs() > (1e-4 if sat_only else 0.25)) & ((torch.arange(T) % 20 == 7) | sat_only)
    k = torch.cumsum(want.long(), 0) - 1                      # saturated edge i: label i % 2, sign (i / 2) % 2
    y = torch.where(want, (k % 2).float(), y)
    sign = torch.where(want & ((k // 2) % 2 == 1), -torch.sign(s), torch.ones_like(s))
    target = torch.where(want, 22.0 + 10.0 * torch.rand(T, generator=g, dtype=F64), s.abs().clamp(max=7.5))
    fac = torch.where(want | (s.abs() > 7.5), target / s.abs().clamp_min(1e-30), torch.ones_like(s)) * sign
    c.Xt = (Xt.double() * fac[:, None]).float()
    c.y, c.want_sat = y, want
    c.scale = 1.0 / (T * N)
    hperm = torch.argsort(c.h, stable=True)
    c.hperm = hperm.to(I32)
    c.hptr = torch.searchsorted(c.h[hperm].contiguous(), torch.arange(N + 1), right=False).to(I32)
    return c


def dm_ref(c, train=True, omit=None):
    """fp64 DistMult + Keras BCE + seeds from the fp32 inputs: name -> (reference, bound).  `omit`: edges left out
    (their seeds zero), the self-check's dropped group."""
    D, R, T, N = c.D, c.R, c.T, c.N
    a, b, rho, y = c.Xh.double()[c.h], c.Xt.double(), c.rel.double()[c.r], c.y.double()
    scale = f32c(c.scale)
    omit = torch.zeros(T, dtype=torch.bool) if omit is None else omit
    # s = sum_c a rho b: D terms of two multiplies each, summed in any order (lane quads, then a butterfly)
    t = a * rho * b
    s, Ds = t.sum(1), gam(D + 2) * t.abs().sum(1)
    assert bool(((s.abs() <= 8.0) | (s.abs() >= 20.0)).all()), "a logit lies in the gap 8 < |s| < 20"
    assert bool((s.abs()[c.want_sat] >= 20.0).all()) and bool((s.abs()[~c.want_sat] <= 8.0).all())
    # p = 1 / (1 + expf(-s)): dp/ds = p q (q = 1 - p); p = 1 / (1 + E) has relative sensitivity q to E (EXP_ULP
    # ulps), then the add's rounding and the division's DIV_ULP ulps act on p directly
    p, q = torch.sigmoid(s), torch.sigmoid(-s)
    Dp = p * q * torch.expm1(Ds) + p * (q * EXP_ULP * ULP + U + DIV_ULP * ULP)
    out = {"s": (s, Ds), "p": (p, Dp)}
    sat = (p < EPS32) | (p > HI32)
    assert bool((sat == c.want_sat).all())
    if train:
        assert bool(((y == 0) | (y == 1)).all())        # one branch of g is then exactly zero: no cancellation

        def seed(pp, qq):        # ds(p) = scale (-y / (p + eps) + (1 - y) / (1 - p + eps)) p (1 - p)
            return scale * (-y / (pp + EPS32) + (1 - y) / (qq + EPS32)) * pp * qq
        ds = seed(p, q)
        # ds is monotone in p for y in {0, 1} (~ -scale (1 - p), ~ scale p): its range over p +- Dp is at the ends.
        # The chain's own roundings on the nonzero branch: p + eps (or 1 - p, then + eps), the division (2 DIV_ULP
        # u), x scale, x p, 1 - p, x (1 - p): at most 6 + 5 = 11 u, all multiplicative
        up, dn = seed((p + Dp).clamp_max(1), (q - Dp).clamp_min(0)), seed((p - Dp).clamp_min(0), (q + Dp).clamp_max(1))
        Dds = torch.maximum((up - ds).abs(), (dn - ds).abs()) + gam(11) * ds.abs()
        dead = sat | omit          # p clipped: g = 0 exactly, so ds, the do row and every contribution are exact zeros
        ds, Dds = torch.where(dead, 0.0, ds), torch.where(dead, 0.0, Dds)
        # loss term: Keras' -(y log(clip(p) + eps) + (1 - y) log(1 - clip(p) + eps)) with the fp32 constants; the
        # argument of each log carries Dp (unclipped p only), the rounding of + eps (and of 1 - p), then LOG_ULP ulps
        pc = p.clamp(EPS32, HI32)
        onem = torch.where(sat, 1 - pc, q)
        Dpc = torch.where(sat, 0.0, Dp)
        x1, x0 = pc + EPS32, onem + EPS32
        Lt = -(y * torch.log(x1) + (1 - y) * torch.log(x0))
        dx1, dx0 = Dpc + U * x1, Dpc + U * onem + U * x0
        DLt = y * (dx1 / (x1 - dx1)) + (1 - y) * (dx0 / (x0 - dx0)) + LOG_ULP * ULP * Lt.abs()
    else:
        # prediction seed: g = scale for every edge, ds = scale p (1 - p) (3 roundings), |d(pq)/dp| = |q - p|
        ds = scale * p * q
        Dds = scale * ((q - p).abs() * Dp + Dp * Dp) + gam(3) * ds
        ds, Dds = torch.where(omit, 0.0, ds), torch.where(omit, 0.0, Dds)
        Lt, DLt = p, Dp
    Lt, DLt = torch.where(omit, 0.0, Lt), torch.where(omit, 0.0, DLt)
    out["ds"] = (ds, Dds)
    # the slab sums: T terms in any order
    out["loss"] = (Lt.sum().reshape(1), (DLt.sum() + gam(T) * Lt.abs().sum()).reshape(1))
    out["loss_terms"] = (Lt, DLt)
    # do = ((ds rho) a) (b (1 - b)): 5 roundings on top of ds
    w = rho * a * b * (1 - b)
    do = ds[:, None] * w
    out["do"] = (do, w.abs() * Dds[:, None] + gam(5) * do.abs())
    # drel[r] = sum over the edges of r of ds (a b): 2 multiplies per term
    ab = a * b
    tt = ds[:, None] * ab
    nr = torch.bincount(c.r, minlength=R).double()
    out["drel"] = (segsum(tt, c.r, R), segsum(ab.abs() * Dds[:, None], c.r, R) + gam(nr + 2)[:, None] * segsum(tt.abs(), c.r, R))
    # dXh[n] = a (1 - a) sum_k fma(b ds, rho, acc): 1 multiply per term, then 1 - a, a (1 - a) and the final product
    th = b * ds[:, None] * rho
    aa = c.Xh.double() * (1 - c.Xh.double())
    ln = torch.bincount(c.h, minlength=N).double()
    out["dXh"] = (aa * segsum(th, c.h, N),
                  aa.abs() * (segsum((b * rho).abs() * Dds[:, None], c.h, N) + gam(ln + 4)[:, None] * segsum(th.abs(), c.h, N)))
    out["sat"] = sat
    return out


def dm_emul32(c, train=True):
    """The kernels' arithmetic in fp32 torch on the CPU (sums in torch's order)."""
    a, b, rho, y = c.Xh[c.h], c.Xt, c.rel[c.r], c.y
    s = (a * rho * b).sum(1)
    p = 1.0 / (1.0 + torch.exp(-s))
    if train:
        pc = p.clamp(EPS32, HI32)
        ok = (p >= EPS32) & (p <= HI32)
        g = torch.where(ok, c.scale * (-(y / (pc + EPS32)) + (1.0 - y) / (1.0 - pc + EPS32)), torch.zeros_like(p))
        Lt = -(y * torch.log(pc + EPS32) + (1.0 - y) * torch.log(1.0 - pc + EPS32))
    else:
        g, Lt = torch.full_like(p, c.scale), p
    ds = g * p * (1.0 - p)
    do = ((ds[:, None] * rho) * a) * (b * (1.0 - b))
    return {"s": s, "p": p, "ds": ds, "do": do, "loss": Lt.sum().reshape(1), "loss_terms": Lt,
            "drel": segsum(ds[:, None] * (a * b), c.r, c.R),
            "dXh": segsum((b * ds[:, None]) * rho, c.h, c.N) * (c.Xh * (1.0 - c.Xh))}


DM_NAMES = ("s", "p", "ds", "do", "loss", "drel", "dXh")


def _last_block(T, blk=256):
    m = torch.zeros(T, dtype=torch.bool)
    m[blk * ((T - 1) // blk):] = True
    return m


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("D,R,T", [(32, 3, 257), (256, 2, 255), (64, 8, 300)])
def test_selfcheck_distmult_bounds(D, R, T, train):
    c = dm_case(D, R, T)
    refs = dm_ref(c, train)
    em = dm_emul32(c, train)
    check_all(em, refs, f"cpu-fp32 distmult D{D} R{R} T{T} train{train}", DM_NAMES + ("loss_terms",))
    k = R - 1
    ek = c.r == k
    dropped = dm_ref(c, train, omit=_last_block(T))
    named = {n: refs[n] for n in DM_NAMES}
    sl = {"ds": ek, "do": ek, "drel": k, "p": ek, "s": ek}
    if not train:      # every term of the prediction seed's drel is positive and carries the logit's worst-case error
        del sl["drel"]     # gamma(D + 2) sum|t| (4e-4 at D = 256) with one sign: 1e-4 is below what that bar resolves
    assert_perturbations_rejected(named, sl,
                                  {n: dropped[n][0] for n in ("ds", "do", "drel", "loss", "dXh")},
                                  f"distmult D{D} R{R} T{T}")
    if train:        # an all-zero tail seed, relation gradient or head seed (what the old bars let through) is refused
        for n in ("ds", "do", "drel", "dXh"):
            assert rejects(torch.zeros_like(refs[n][0]), *refs[n]), n
        # a saturated edge given the unclipped seed is refused: its bound is zero
        sat = refs["sat"]
        cand = refs["ds"][0].clone()
        cand[sat] = 1e-12
        assert bool(sat.any()) and rejects(cand, *refs["ds"])


def _dm_dev(c, dev):
    d = DmCase()
    d.__dict__.update(c.__dict__)
    for k in ("Xh", "Xt", "rel", "y"):
        setattr(d, k, getattr(c, k).to(dev))
    for k in ("h", "r"):
        setattr(d, k, getattr(c, k).to(I32).to(dev))
    d.hperm, d.hptr = c.hperm.to(dev), c.hptr.to(dev)
    return d


def _dm_collect(c, nb, bufs, wholes, what):
    for k, w in wholes.items():
        guard_intact(w, f"{what} {k}")
    out = {k: v.detach().cpu().clone() for k, v in bufs.items()}
    if "drel_slab" in out:
        out["drel"] = out["drel_slab"].view(nb, c.R, c.D).double().sum(0)        # the partials summed exactly
        out["loss"] = out["loss_slab"].double().sum().reshape(1)
    return out


def run_dm_plain(c, d, dev, train=True, t_idx=None, Xt=None):
    """One distmult_bce launch into NaN-prefilled, guarded outputs; returns CPU copies (+ the slab sums in fp64)."""
    T, D, R = c.T, c.D, c.R
    nb = ops.distmult_blocks(T)
    wholes, bufs = {}, {}
    for k, shape in (("p", (T,)), ("s", (T,)), ("ds", (T,)), ("do", (T, D)), ("drel_slab", (nb * R * D,)),
                     ("loss_slab", (nb,))):
        if not train and k not in ("p", "s"):
            continue
        wholes[k], bufs[k] = guarded(dev, *shape)
    kw = dict(p_out=bufs["p"], s_out=bufs["s"])
    if train:
        kw.update(y=d.y, scale=c.scale, ds_out=bufs["ds"], do_out=bufs["do"], drel_slab=bufs["drel_slab"],
                  loss_slab=bufs["loss_slab"])
    ops.distmult_bce(d.Xh, d.h, d.Xt if Xt is None else Xt, d.r, d.rel, t_idx=t_idx, **kw)
    return _dm_collect(c, nb, bufs, wholes, "distmult_bce")


def run_dm_heads(c, d, dev, train=True, in_place=False):
    T, D, R, N = c.T, c.D, c.R, c.N
    nb = ops.distmult_blocks(T)
    wholes, bufs = {}, {}
    for k, shape in (("p", (T,)), ("s", (T,)), ("ds", (T,)), ("do", (T, D)), ("dXh", (N, D)),
                     ("drel_slab", (nb * R * D,)), ("loss_slab", (nb,))):
        wholes[k], bufs[k] = guarded(dev, *shape)
    Xt = d.Xt
    if in_place:                       # do_out aliases Xt: do^3 written over x^3
        bufs["do"].copy_(d.Xt)
        Xt = bufs["do"]
    ops.distmult_bce_heads(d.hptr, d.hperm, d.Xh, Xt, d.r, d.rel, d.y if train else None, bufs["do"], bufs["dXh"],
                           bufs["drel_slab"], bufs["loss_slab"], scale=c.scale, p_out=bufs["p"], s_out=bufs["s"],
                           ds_out=bufs["ds"])
    return _dm_collect(c, nb, bufs, wholes, "distmult_bce_heads")


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs bitwise"


DM_RAW = ("p", "s", "ds", "do", "drel_slab", "loss_slab")


@gpu
@pytest.mark.parametrize("T", [1, 255, 257, 7001])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_distmult_bce_training_vs_fp64(D, R, T, cuda):
    """distmult_bce and distmult_bce_heads (BCE seed, scale = 1 / (T N) as in production, so do ~ 1e-7) against fp64,
    every output per element: s, p, ds, do, drel, the loss and (heads) dXh.  T around one 256-thread block, the
    U = 2 pipelining and the grid-stride tail.  Saturated edges: ds and their do rows exactly zero (zero bound), no
    contribution to drel / dXh (the reference omits them), their loss terms the Keras clip form.  Both forms twice
    (deterministic), with t_idx, in place (do over Xt), and the bitwise relations between the two forms: p, s, ds,
    do; dXh at D = 256 bitwise the seg_gather_reduce of the plain form's ds."""
    c = dm_case(D, R, T)
    refs = dm_ref(c, True)
    d = _dm_dev(c, cuda)
    what = f"D{D} R{R} T{T}"
    plain = run_dm_plain(c, d, cuda)
    check_all(plain, refs, "distmult_bce " + what, ("s", "p", "ds", "do", "drel", "loss"))
    _same(plain, run_dm_plain(c, d, cuda), DM_RAW, "distmult_bce run twice")
    sat = refs["sat"]
    assert bool((plain["ds"][sat] == 0).all()) and bool((plain["do"][sat] == 0).all())
    # t_idx: the tail rows as a shuffled table
    perm = torch.randperm(T, generator=_gen(T))
    tab = torch.empty_like(c.Xt)
    tab[perm] = c.Xt
    _same(plain, run_dm_plain(c, d, cuda, t_idx=perm.to(I32).to(cuda), Xt=tab.to(cuda)), DM_RAW, "distmult_bce t_idx")
    heads = run_dm_heads(c, d, cuda)
    check_all(heads, refs, "distmult_bce_heads " + what, DM_NAMES)
    _same(heads, run_dm_heads(c, d, cuda), DM_RAW + ("dXh",), "distmult_bce_heads run twice")
    _same(heads, run_dm_heads(c, d, cuda, in_place=True), DM_RAW + ("dXh",), "distmult_bce_heads in place")
    _same(heads, plain, ("p", "s", "ds", "do"), "heads form vs plain form")
    empty = (c.hptr[1:] == c.hptr[:-1])
    assert bool((heads["dXh"][empty] == 0).all())
    # the head seed as the two-kernel path forms it
    w, o = guarded(cuda, c.N, D)
    ops.seg_gather_reduce(d.hptr, d.Xt, o, perm=d.hperm, coef=plain["ds"].to(cuda), r_idx=d.r, rel=d.rel, X=d.Xh)
    guard_intact(w, "seg_gather_reduce")
    assert_within(o, *refs["dXh"], "seg_gather_reduce(dXh) " + what)
    if D == 256:
        assert torch.equal(o.cpu(), heads["dXh"])


@gpu
@pytest.mark.parametrize("T", [257, 7001])
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_distmult_heads_prediction_seed_vs_fp64(D, R, T, cuda):
    """y = None: g = scale for every edge, saturated ones included (no clipping), and the loss slabs sum p."""
    c = dm_case(D, R, T)
    refs = dm_ref(c, False)
    d = _dm_dev(c, cuda)
    heads = run_dm_heads(c, d, cuda, train=False)
    check_all(heads, refs, f"distmult_bce_heads(pred) D{D} R{R} T{T}", DM_NAMES)
    _same(heads, run_dm_heads(c, d, cuda, train=False), DM_RAW + ("dXh",), "prediction seed run twice")
    pred = run_dm_plain(c, d, cuda, train=False)          # the plain form without y: p and s only
    _same(heads, pred, ("p", "s"), "plain predict vs heads")


@gpu
@pytest.mark.parametrize("D,R", [(32, 1), (128, 3), (256, 2), (256, 8)])
def test_distmult_all_saturated_batch(D, R, cuda):
    """Every edge saturated (|s| >= 20, both signs, both labels): the BCE clip branch alone.  p is 0 / 1 within the
    allowance, every seed output is EXACTLY zero and the loss is the sum of the Keras clip terms
    -log(clip(p) + eps) with the fp32 constants 1e-7f and 1.0f - 1e-7f."""
    c = dm_case(D, R, 300, sat_only=True)
    refs = dm_ref(c, True)
    assert bool(refs["sat"].all())
    lt, low, y1 = refs["loss_terms"][0], refs["p"][0] < 0.5, c.y == 1
    k = lambda x: torch.full_like(lt, -math.log(x))      # noqa: E731
    clip = torch.where(low, torch.where(y1, k(2 * EPS32), k(1.0)), torch.where(y1, k(HI32 + EPS32), k((1.0 - HI32) + EPS32)))
    assert bool(((lt - clip).abs() <= 1e-12).all())
    assert all(bool((low == a).logical_and(y1 == b).any()) for a in (True, False) for b in (True, False))
    d = _dm_dev(c, cuda)
    for out, names in ((run_dm_plain(c, d, cuda), ("s", "p", "ds", "do", "drel", "loss")),
                       (run_dm_heads(c, d, cuda), DM_NAMES)):
        check_all(out, refs, f"distmult saturated D{D} R{R}", names)
        for k in ("ds", "do", "drel_slab"):
            assert bool((out[k] == 0).all()), k
    assert bool((out["dXh"] == 0).all())
    assert bool(((out["p"] == 0) | (out["p"] == 1) | (out["p"] < EPS32)).all())


@gpu
def test_distmult_empty_batches(cuda):
    """The documented contract (include/iddgcn.h): iddgcn_distmult_bce_f32 with T = 0 launches nothing and leaves its
    slabs untouched (the engine trains through the heads form only); iddgcn_distmult_bce_heads_f32 always writes its
    n_blocks slab partials: zeros for n_nodes = 0, and for nodes without any edge also zero dXh rows."""
    lib, st = ops.L.lib(), ops._stream()
    D, R, N = 64, 3, 5
    buf = torch.rand(64, D, device=cuda)
    ib = torch.zeros(64, dtype=I32, device=cuda)
    wr, slab_r = guarded(cuda, R * D)
    wl, slab_l = guarded(cuda, 1)
    wo, do = guarded(cuda, 4, D)
    wx, dXh = guarded(cuda, N, D)
    wd, ds = guarded(cuda, 4)
    assert ops.distmult_blocks(0) == 1
    rc = lib.iddgcn_distmult_bce_f32(st, 0, D, R, _ptr(buf), _ptr(ib), _ptr(buf), None, _ptr(ib), _ptr(buf), _ptr(buf),
                                     1.0, None, None, _ptr(ds), _ptr(do), _ptr(slab_r), _ptr(slab_l), 1)
    torch.cuda.synchronize()
    assert rc == 0
    for w in (wr, wl, wo, wd):
        assert bool(torch.isnan(w).all())               # nothing written: the caller must not reduce these slabs
    rc = lib.iddgcn_distmult_bce_heads_f32(st, 0, D, R, _ptr(ib), _ptr(ib), _ptr(buf), _ptr(buf), _ptr(ib), _ptr(buf),
                                           _ptr(buf), 1.0, None, None, _ptr(ds), _ptr(do), _ptr(dXh), _ptr(slab_r),
                                           _ptr(slab_l), 1)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((slab_r == 0).all()) and bool((slab_l == 0).all())
    guard_intact(wr, "drel slab")
    guard_intact(wl, "loss slab")
    assert bool(torch.isnan(wx).all()) and bool(torch.isnan(wo).all()) and bool(torch.isnan(wd).all())
    slab_r.fill_(NAN)
    slab_l.fill_(NAN)
    rc = lib.iddgcn_distmult_bce_heads_f32(st, N, D, R, _ptr(ib), _ptr(ib), _ptr(buf), _ptr(buf), _ptr(ib), _ptr(buf),
                                           _ptr(buf), 1.0, None, None, _ptr(ds), _ptr(do), _ptr(dXh), _ptr(slab_r),
                                           _ptr(slab_l), 1)      # seg_ptr all zero: N heads, no edge
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((dXh == 0).all()) and bool((slab_r == 0).all()) and bool((slab_l == 0).all())
    guard_intact(wx, "dXh")
    assert bool(torch.isnan(wo).all()) and bool(torch.isnan(wd).all())


# =============================================================================================================
# Adam
# =============================================================================================================
B1, B2, ADAM_EPS, ALPHA = f32c(0.9), f32c(0.999), f32c(1e-7), f32c(3e-4)


def adam_case(n):
    """g over 8 decades with exact zeros; v with zeros and values ~1e-12 (sqrt(v) + eps dominated by eps); m of both
    signs."""
    g = _gen(77 + n)
    gr = torch.randn(n, generator=g) * 10.0 ** (-8.0 * torch.rand(n, generator=g))
    gr[torch.rand(n, generator=g) < 0.1] = 0.0
    v = torch.rand(n, generator=g) * 1e-6
    sel = torch.rand(n, generator=g)
    v = torch.where(sel < 0.1, torch.zeros(n), torch.where(sel < 0.3, v * 1e-6, v))
    m = torch.randn(n, generator=g) * 1e-3
    var = torch.randn(n, generator=g)
    return var, m, v, gr


def adam_ref(var, m, v, g, sparse, alpha=ALPHA, b1=B1, b2=B2, eps=ADAM_EPS, live=None):
    """fp64 Keras Adam with the fp32 constants the kernel holds (b1, b2, eps, alpha as C floats; 1.0f - b is exact for
    b in [0.5, 1], Sterbenz).  `live`: elements updated (the self-check's dropped group keeps its old values)."""
    var0, m0, v0 = var.double(), m.double(), v.double()
    g = g.double()
    c1, c2 = 1.0 - b1, 1.0 - b2
    assert f32c(c1) == c1 and f32c(c2) == c2
    if sparse:
        # m b1 + g c1: two products and one add: each term meets two roundings
        mr, Dm = m0 * b1 + g * c1, gam(2) * ((m0 * b1).abs() + (g * c1).abs())
        # v b2 + (g g) c2: the second term has two multiplies
        vr, Dv = v0 * b2 + g * g * c2, gam(3) * (v0 * b2 + g * g * c2)
    else:
        # m + (g - m) c1: the subtraction, the product, the add: 3 roundings on |m| + |(g - m) c1|
        mr, Dm = m0 + (g - m0) * c1, gam(3) * (m0.abs() + ((g - m0) * c1).abs())
        # v + (g g - v) c2: the square, the subtraction, the product, the add: 4 roundings on v + (g g + v) c2
        vr, Dv = v0 + (g * g - v0) * c2, gam(4) * (v0 + (g * g + v0) * c2)
    # var - (m alpha) / (sqrtf(v) + eps).  den = sqrt(v) + eps carries v's error through the square root (the full
    # width of sqrt over v +- Dv: no derivative, which is singular at v = 0), SQRT_ULP ulps, and the add's rounding
    sq = vr.clamp_min(0).sqrt()
    den = sq + eps
    Dden = ((vr + Dv).sqrt() - (vr - Dv).clamp_min(0).sqrt()) + SQRT_ULP * ULP * sq + U * den
    upd = mr * alpha / den
    # upd: m's error over den, den's error relative, the product m alpha (u) and the division (DIV_ULP ulps)
    Dupd = Dm * alpha / (den - Dden) + upd.abs() * (Dden / (den - Dden) + gam(1) + DIV_ULP * ULP)
    vn = var0 - upd
    Dvar = Dupd + U * (var0.abs() + upd.abs())                       # the final subtraction
    if live is not None:
        z = torch.zeros_like(Dm)
        mr, vr, vn = torch.where(live, mr, m0), torch.where(live, vr, v0), torch.where(live, vn, var0)
        Dm, Dv, Dvar = torch.where(live, Dm, z), torch.where(live, Dv, z), torch.where(live, Dvar, z)
    return {"m": (mr, Dm), "v": (vr, Dv), "var": (vn, Dvar)}


def adam_emul32(var, m, v, g, sparse):
    c1, c2 = 1.0 - B1, 1.0 - B2
    if sparse:
        mi, vi = m * B1 + g * c1, v * B2 + (g * g) * c2
    else:
        mi, vi = m + (g - m) * c1, v + (g * g - v) * c2
    return {"m": mi, "v": vi, "var": var - (mi * ALPHA) / (torch.sqrt(vi) + ADAM_EPS)}


@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("n", [257, 10001])
def test_selfcheck_adam_bounds(n, sparse):
    case = adam_case(n)
    refs = adam_ref(*case, sparse)
    check_all(adam_emul32(*case, sparse), refs, f"cpu-fp32 adam n{n} sparse{sparse}")
    live = torch.ones(n, dtype=torch.bool)
    live[-max(n % 256, 4):] = False        # the last ragged block left alone (at least 4 elements: one may have v = 0)
    dropped = adam_ref(*case, sparse, live=live)
    third = slice(0, n // 3)
    assert_perturbations_rejected(refs, {"m": third, "v": third}, {k: dropped[k][0] for k in refs},
                                  f"adam n{n} sparse{sparse}")
    # the update var - var0 scaled by 1 + 1e-4 on a third of the elements
    cand = refs["var"][0].clone()
    cand[third] = case[0].double()[third] + (cand[third] - case[0].double()[third]) * (1 + 1e-4)
    assert rejects(cand, *refs["var"])
    # non-vacuity: a v that is never updated and a b2 of 0.99 are refused.  (The two forms themselves are the same
    # real-number function, since 1.0f - b is exact: m + (g - m)(1 - b1) = b1 m + (1 - b1) g.  They differ only in
    # their roundings, which is why each is held to its own chain's bound.)
    assert rejects(case[2].double(), *refs["v"])
    assert rejects(adam_ref(*case, sparse, b2=f32c(0.99))["v"][0], *refs["v"])
    assert rejects(adam_ref(*case, sparse, b1=f32c(0.99))["m"][0], *refs["m"])
    assert rejects(torch.zeros(n, dtype=F64), *refs["v"]) and rejects(case[0].double(), *refs["var"])


def _adam_bufs(case, dev):
    wholes, bufs = [], []
    for t in case[:3]:
        w, b = guarded(dev, t.numel())
        b.copy_(t)
        wholes.append(w)
        bufs.append(b)
    return wholes, bufs, case[3].to(dev)


@gpu
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 10001])
def test_adam_vs_fp64(n, sparse, cuda):
    """adam: m, v and var per element against each form's OWN formula in fp64, with the fp32 constants the kernel
    holds; twice (deterministic); adam_table with alpha_table[k], step = [k] bitwise adam(alpha = table[k]) for
    k = 0 and a middle k, and it does not write step."""
    case = adam_case(n)
    refs = adam_ref(*case, sparse)
    runs = []
    for _ in range(2):
        wholes, (var, m, v), g = _adam_bufs(case, cuda)
        ops.adam(var, m, v, g, ALPHA, B1, B2, ADAM_EPS, sparse)
        for w in wholes:
            guard_intact(w, "adam")
        runs.append({"var": var.cpu(), "m": m.cpu(), "v": v.cpu()})
    check_all(runs[0], refs, f"adam n{n} sparse{sparse}")
    _same(runs[0], runs[1], ("var", "m", "v"), "adam run twice")
    table = torch.tensor([ALPHA, 1e-3, 2.5e-4, 7e-4, 1e-5], dtype=F32)
    for k in (0, 2):
        wholes, (var, m, v), g = _adam_bufs(case, cuda)
        ops.adam(var, m, v, g, float(table[k]), B1, B2, ADAM_EPS, sparse)
        wholes2, (var2, m2, v2), _ = _adam_bufs(case, cuda)
        step = torch.tensor([k], dtype=I32, device=cuda)
        ops.adam_table(var2, m2, v2, g, table.to(cuda), step, B1, B2, ADAM_EPS, sparse)
        assert torch.equal(var, var2) and torch.equal(m, m2) and torch.equal(v, v2)
        assert int(step.item()) == k
        for w in wholes2:
            guard_intact(w, "adam_table")


@gpu
def test_step_advance(cuda):
    """loss_history[step] = loss, step += 1, neighbours untouched; both NULL-argument forms; three calls."""
    hist = torch.full((8,), NAN, device=cuda)
    ctr = torch.tensor([2, -7], dtype=I32, device=cuda)            # [step, a neighbour that must survive]
    step = ctr[:1]
    losses = [0.75, -3.5, 1e-7]
    for i, lv in enumerate(losses):
        ops.step_advance(step, hist, torch.tensor([lv], dtype=F32, device=cuda))
        assert ctr.tolist() == [3 + i, -7]
    h = hist.cpu()
    assert h[2:5].tolist() == [f32c(x) for x in losses]
    assert bool(torch.isnan(h[:2]).all()) and bool(torch.isnan(h[5:]).all())
    ops.step_advance(step, None, torch.tensor([9.0], device=cuda))      # no history: counts only
    ops.step_advance(step, hist, None)                                  # no loss: counts only
    ops.step_advance(step)
    assert ctr.tolist() == [8, -7]
    assert torch.equal(hist.cpu()[2:5], h[2:5]) and bool(torch.isnan(hist.cpu()[5:]).all())


@gpu
@pytest.mark.parametrize("sparse", [0, 1])
def test_adam_table_three_replayed_iterations(sparse, cuda):
    """Three iterations of adam_table + step_advance on one stream (the graph-replayed fit's tail) are bitwise three
    adam calls with host-side alphas, and the history holds the three losses."""
    n = 1001
    case = adam_case(n)
    alphas = [f32c(1e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)) for t in (1, 2, 3)]
    grads = [case[3], case[3].flip(0) * 0.5, case[3] * -2.0]
    _, (var, m, v), _ = _adam_bufs(case, cuda)
    for a, g in zip(alphas, grads):
        ops.adam(var, m, v, g.to(cuda), a, B1, B2, ADAM_EPS, sparse)
    _, (var2, m2, v2), _ = _adam_bufs(case, cuda)
    table = torch.tensor(alphas, dtype=F32, device=cuda)
    step = torch.zeros(1, dtype=I32, device=cuda)
    hist = torch.full((4,), NAN, device=cuda)
    loss = torch.zeros(1, device=cuda)
    for i, g in enumerate(grads):
        loss.fill_(1.5 - i)
        ops.adam_table(var2, m2, v2, g.to(cuda), table, step, B1, B2, ADAM_EPS, sparse)
        ops.step_advance(step, hist, loss)
    assert torch.equal(var, var2) and torch.equal(m, m2) and torch.equal(v, v2)
    assert int(step.item()) == 3 and hist.cpu()[:3].tolist() == [1.5, 0.5, -0.5] and bool(torch.isnan(hist[3]))


# =============================================================================================================
# Segmented reductions and the head backward
# =============================================================================================================
GRAPHS = ["uniform", "hub", "sparse", "empty", "tiny"]


def seg_graph(case, seed):
    """Sorted segment ids of T edges over N nodes (N no multiple of the 4 nodes per block): runs of nodes without
    edges, a hub holding a third of the edges (many groups of U = 4 / 8), nodes with 0 and 1 edges, tiny graphs.
    "small" is the self-check's size: sums short enough for the bar to resolve a 1e-4 relative error."""
    g = _gen(seed)
    N = {"tiny": 5, "empty": 301, "small": 103}.get(case, 1003)
    T = {"tiny": 37, "empty": 3, "sparse": 60, "small": 600}.get(case, 3000)
    t = torch.randint(0, N, (T,), generator=g)
    if case in ("hub", "small"):
        t[: T // 3] = N // 2
    if case == "uniform":
        t[(t >= 100) & (t < 140)] = 99            # 40 consecutive nodes without edges
    t = torch.sort(t).values
    ptr = torch.searchsorted(t, torch.arange(N + 1), right=False).to(I32)
    return N, T, t, ptr


def last_group(ptr, T, U4=4):
    """The last (ragged) group of U edges of the longest segment."""
    ln = (ptr[1:] - ptr[:-1]).long()
    n = int(ln.argmax())
    L, end = int(ln[n]), int(ptr[n + 1])
    m = torch.zeros(T, dtype=torch.bool)
    m[end - (L % U4 or min(U4, L)):end] = True
    return m


def tail_ref(N, t, ptr, h, W, dO, P, drop=None):
    """dP[r][n] = sum_e W[h_e][r] dO[e] (len terms, one multiply: gamma(len + 1)); dsum[n] = sum_e dO[e]
    (gamma(len)); dWedge[e][r] = <dO[e], P[r][n]> (D terms, one multiply: gamma(D + 1)).  Nodes without edges: every
    term list is empty, the bound is zero, the rows must be exact zeros."""
    T, D = dO.shape
    R = P.shape[0]
    Wd = W.double()[h] if h is not None else W.double()
    d, Pd = dO.double(), P.double()
    keep = torch.ones(T, dtype=F64) if drop is None else (~drop).double()
    ln = (ptr[1:] - ptr[:-1]).double()
    dk = d * keep[:, None]
    dP, bP, dW, bW = [], [], [], []
    for r in range(R):
        wd = Wd[:, r:r + 1] * dk
        dP.append(segsum(wd, t, N))
        bP.append(gam(ln + 1)[:, None] * segsum(wd.abs(), t, N))
        q = dk * Pd[r][t]
        dW.append(q.sum(1))
        bW.append(gam(D + 1) * q.abs().sum(1))
    return {"dP": (torch.stack(dP), torch.stack(bP)), "dsum": (segsum(dk, t, N), gam(ln)[:, None] * segsum(dk.abs(), t, N)),
            "dWedge": (torch.stack(dW, 1), torch.stack(bW, 1))}


def tail_inputs(case, R, D, seed, split_w=False):
    N, T, t, ptr = seg_graph(case, seed)
    g = _gen(seed + 1)
    h = torch.randint(0, N, (T,), generator=g)
    W = torch.rand(N, R, generator=g)
    if split_w:                 # relation 0 ~ 1, relation 1 ~ 1e-3: a swap of relations cannot hide inside any bar
        W[:, 1] *= 1e-3
    return N, T, t, ptr, h, W, torch.randn(T, D, generator=g), torch.randn(R, N, D, generator=g)


def test_selfcheck_tail_seg_bounds():
    R, D = 3, 32
    N, T, t, ptr, h, W, dO, P = tail_inputs("small", R, D, 5)
    refs = tail_ref(N, t, ptr, h, W, dO, P)
    Wg = W[h]
    em = {"dP": torch.stack([segsum(Wg[:, r:r + 1] * dO, t, N) for r in range(R)]), "dsum": segsum(dO, t, N),
          "dWedge": torch.stack([(dO * P[r][t]).sum(1) for r in range(R)], 1)}
    check_all(em, refs, "cpu-fp32 tail_seg_reduce")
    dropped = tail_ref(N, t, ptr, h, W, dO, P, drop=last_group(ptr, T))
    assert_perturbations_rejected(refs, {"dP": 1, "dWedge": (slice(None), 1)}, {k: dropped[k][0] for k in refs},
                                  "tail_seg_reduce")
    swapped = refs["dP"][0].flip(0)
    assert rejects(swapped, *refs["dP"])


def run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=True):
    """tail_seg_reduce on row-range views [2, 2 + N) of (R, N + 3, D) tables (relation stride > N D), everything
    NaN-prefilled: returns CPU copies after checking that nothing outside the views was written."""
    R, _, D = P.shape
    Pb = torch.full((R, N + 3, D), NAN, device=cuda)
    Pb[:, 2:2 + N] = P.to(cuda)
    dPb = torch.full((R, N + 3, D), NAN, device=cuda)
    wW, dWe = guarded(cuda, T, R)
    wS, ds = guarded(cuda, N, D)
    ops.tail_seg_reduce(ptr.to(cuda), None if h is None else h.to(I32).to(cuda), W.to(cuda), dO.to(cuda),
                        Pb[:, 2:2 + N], dPb[:, 2:2 + N], dWe, dsum=ds if dsum else None)
    assert bool(torch.isnan(dPb[:, :2]).all()) and bool(torch.isnan(dPb[:, 2 + N:]).all()), "dP rows outside the view"
    guard_intact(wW, "dWedge")
    assert bool(torch.isnan(wS[-1] if dsum else wS).all())
    out = {"dP": dPb[:, 2:2 + N].cpu(), "dWedge": dWe.cpu()}
    if dsum:
        out["dsum"] = ds.cpu()
    return out


def _tail_check(cuda, case, R, D, split_w=False):
    N, T, t, ptr, h, W, dO, P = tail_inputs(case, R, D, 11 * R + D + len(case), split_w)
    refs = tail_ref(N, t, ptr, h, W, dO, P)
    what = f"tail_seg_reduce(h_idx) {case} R{R} D{D}"
    a = run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=True)
    check_all(a, refs, what)
    _same(a, run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=True), ("dP", "dsum", "dWedge"), what + " run twice")
    b = run_tail(cuda, N, T, ptr, h, W, dO, P, dsum=False)
    _same(a, b, ("dP", "dWedge"), what + " without dsum")
    # the engine's form: W gathered per edge once (gather_rows), h_idx = None: bitwise the h_idx form
    wg, We = guarded(cuda, T, R)
    ops.gather_rows(W.to(cuda), h.to(I32).to(cuda), We)
    guard_intact(wg, "gather_rows")
    assert torch.equal(We.cpu(), W[h])
    c = run_tail(cuda, N, T, ptr, None, We.cpu(), dO, P, dsum=True)
    check_all(c, refs, what.replace("h_idx", "per-edge W"))
    _same(a, c, ("dP", "dsum"), what + " vs per-edge W")


# every graph at D = 64, 256 x R = 1, 2, 4, 8; the other of the 32 tail_seg_reduce_kernel<D, R> instantiations on the
# smallest graph (R = 2 at D = 32, 128: test_tail_seg_reduce_h_idx_slot_partials)
TAIL_ARMS = [(R, D, case) for case in GRAPHS for D in (64, 256) for R in (1, 2, 4, 8)] + \
            [(R, D, "tiny") for D in (32, 64, 128, 256) for R in range(1, 9)
             if not (D in (64, 256) and R in (1, 2, 4, 8)) and not (D in (32, 128) and R == 2)]


@gpu
@pytest.mark.parametrize("R,D,case", TAIL_ARMS)
def test_tail_seg_reduce_h_idx_vs_fp64(R, D, case, cuda):
    """tail_seg_reduce with h_idx (the config-3 / config-4 form; <256, 2> is the headline's instantiation): dP, dsum
    and dWedge per element against fp64, with and without dsum, on row-range views of larger P / dP tables, twice,
    and bitwise the per-edge-W form fed by gather_rows.  Every (D, R) instantiation of the kernel is launched."""
    _tail_check(cuda, case, R, D)


@gpu
@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("D", [32, 128])
def test_tail_seg_reduce_h_idx_slot_partials(D, case, cuda):
    """D < 256 at R = 2: 64 / (D / 4) edge slots per node, partials summed by xor shuffles."""
    _tail_check(cuda, case, 2, D)


@gpu
def test_tail_seg_reduce_headline_instantiation_distinct_relations(cuda):
    """R = 2, D = 256 with h_idx and W[:, 0] ~ 1, W[:, 1] ~ 1e-3: pins the arithmetic of the instantiation that once
    carried the packed-fp32 hazard; a swap or a mix of the two relations is three decades outside the bar."""
    _tail_check(cuda, "hub", 2, 256, split_w=True)


def sgr_ref(N, node_k, ptr, perm, coef, r_idx, rel, rows, X, drop=None):
    """out[n] = (X ? x (1 - x) : 1) sum_k coef[e] rel[r_e] rows[e], e = perm[k]: len terms with one multiply for coef
    and one (fused) for rel, then 1 - x, x (1 - x) and the final product: gamma(len + c)."""
    T = node_k.numel()
    e = perm if perm is not None else torch.arange(T)
    term = rows.double()[e]
    if coef is not None:
        term = term * coef.double()[e][:, None]
    if rel is not None:
        term = term * rel.double()[r_idx[e]]
    if drop is not None:
        term = term * (~drop).double()[:, None]
    c = (coef is not None) + (rel is not None) + 3 * (X is not None)
    xx = X.double() * (1 - X.double()) if X is not None else torch.ones(N, 1, dtype=F64)
    ln = (ptr[1:] - ptr[:-1]).double()
    return {"out": (xx * segsum(term, node_k, N), xx.abs() * gam(ln + c)[:, None] * segsum(term.abs(), node_k, N))}


def sgr_inputs(case, D, seed):
    N, T, t, ptr = seg_graph(case, seed)
    g = _gen(seed + 2)
    return dict(N=N, T=T, t=t, ptr=ptr, perm=torch.randperm(T, generator=g), coef=torch.randn(T, generator=g),
                r_idx=torch.randint(0, 3, (T,), generator=g), rel=torch.randn(3, D, generator=g),
                rows=torch.randn(T, D, generator=g), X=torch.rand(N, D, generator=g))


def test_selfcheck_seg_gather_reduce_bounds():
    i = sgr_inputs("small", 64, 9)
    refs = sgr_ref(i["N"], i["t"], i["ptr"], i["perm"], i["coef"], i["r_idx"], i["rel"], i["rows"], i["X"])
    e = i["perm"]
    em = segsum((i["rows"][e] * i["coef"][e][:, None]) * i["rel"][i["r_idx"][e]], i["t"], i["N"]) * (i["X"] * (1 - i["X"]))
    check_all({"out": em}, refs, "cpu-fp32 seg_gather_reduce")
    dropped = sgr_ref(i["N"], i["t"], i["ptr"], i["perm"], i["coef"], i["r_idx"], i["rel"], i["rows"], i["X"],
                      drop=last_group(i["ptr"], i["T"]))
    rel2 = i["rel"].clone()
    rel2[1] *= 1 + 1e-4                       # one relation's rows scaled: the reference recomputed with it
    scaled = sgr_ref(i["N"], i["t"], i["ptr"], i["perm"], i["coef"], i["r_idx"], rel2.double(), i["rows"], i["X"])
    assert_perturbations_rejected(refs, {}, {"out": dropped["out"][0]}, "seg_gather_reduce")
    assert rejects(scaled["out"][0], *refs["out"])


@gpu
@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("D", [32, 256])
@pytest.mark.parametrize("opts", ["none", "perm", "coef", "rel", "X", "all"])
def test_seg_gather_reduce_vs_fp64(opts, D, case, cuda):
    """seg_gather_reduce with each optional argument on and off, per element against fp64; empty segments exact
    zeros; twice."""
    i = sgr_inputs(case, D, 3 * D + len(case))
    on = lambda k: i[k] if opts in (k, "all") else None      # noqa: E731
    perm, coef, rel, X = on("perm"), on("coef"), on("rel"), on("X")
    refs = sgr_ref(i["N"], i["t"], i["ptr"], perm, coef, i["r_idx"], rel, i["rows"], X)
    dev = lambda t, ty=None: None if t is None else (t.to(ty) if ty else t).to(cuda)      # noqa: E731
    outs = []
    for _ in range(2):
        w, o = guarded(cuda, i["N"], D)
        ops.seg_gather_reduce(i["ptr"].to(cuda), dev(i["rows"]), o, perm=dev(perm, I32), coef=dev(coef),
                              r_idx=dev(i["r_idx"], I32) if rel is not None else None, rel=dev(rel), X=dev(X))
        guard_intact(w, "seg_gather_reduce")
        outs.append(o.cpu())
    assert_within(outs[0], *refs["out"], f"seg_gather_reduce {opts} {case} D{D}")
    assert torch.equal(outs[0], outs[1])


def softsig_bwd(dW, DdW, S, Wn):
    """ds_r = dW_r w_r (1 - w_r) (3 roundings); dot = sum_r ds_r s_r (R terms, one multiply);
    dz_j = (ds_j - dot) s_j: the bound is taken on the TERMS of ds_j - sum_r ds_r s_r (the subtraction cancels), times
    |s_j|, plus the subtraction's and the product's roundings."""
    R = S.shape[1]
    s, w = S.double(), Wn.double()
    ww = w * (1 - w)
    ds, Dds = dW * ww, ww.abs() * DdW + gam(3) * (dW * ww).abs()
    dot, dotabs = (ds * s).sum(1, keepdim=True), (ds * s).abs().sum(1, keepdim=True)
    Ddot = (s.abs() * Dds).sum(1, keepdim=True) + gam(R + 1) * dotabs
    return (ds - dot) * s, s.abs() * (Dds + Ddot) + gam(2) * s.abs() * (ds.abs() + dotabs)


def head_inputs(n, T, R, D, seed):
    g = _gen(seed)
    h = torch.randint(0, n, (T,), generator=g)
    if T > 20:
        h[: T // 3] = n // 2                   # a hub head
    hperm = torch.argsort(h, stable=True)
    node_k = h[hperm].contiguous()
    hptr = torch.searchsorted(node_k, torch.arange(n + 1), right=False).to(I32)
    S = torch.softmax(torch.randn(n, R, generator=g), -1)
    return dict(n=n, T=T, R=R, D=D, hperm=hperm, node_k=node_k, hptr=hptr, S=S, Wn=torch.sigmoid(S),
                dWedge=torch.randn(max(T, 1), R, generator=g), dwh=torch.randn(n, R, generator=g),
                dO=torch.randn(n, D, generator=g), P=torch.randn(R, n, D, generator=g),
                dP0=torch.randn(R, n, D, generator=g), dsum0=torch.randn(n, D, generator=g))


def head_seg_sums(i, drop=None):
    c = i["dWedge"].double()[i["hperm"]]
    if drop is not None:
        c = c * (~drop).double()[:, None]
    ln = (i["hptr"][1:] - i["hptr"][:-1]).double()
    return segsum(c, i["node_k"], i["n"]), segsum(c.abs(), i["node_k"], i["n"]), ln


def head_dz_ref(i, drop=None):
    """dW = dwh + the head segment's dWedge rows: len + 1 terms, adds only."""
    sg, sa, ln = head_seg_sums(i, drop)
    dW, DdW = i["dwh"].double() + sg, gam(ln + 1)[:, None] * (i["dwh"].double().abs() + sa)
    return {"dz": softsig_bwd(dW, DdW, i["S"], i["Wn"])}


def head_bwd_ref(i, seg=True, ep=None, drop=None):
    """dW_r = <dO[n], P[r][n]> + the head segment's dWedge rows (+ ep): D products and len (+ 1) further terms in any
    order (lane-strided partials, then a butterfly): gamma(D + len + 2).  dP += w dO and dsum += dO: one product and
    one add on |dP0| + |w dO|, one add on |dsum0| + |dO|."""
    d, P = i["dO"].double(), i["P"].double()
    q = d[None] * P
    dW, A = q.sum(2).t(), q.abs().sum(2).t()
    ln = torch.zeros(i["n"], dtype=F64)
    if seg:
        sg, sa, ln = head_seg_sums(i, drop)
        dW, A = dW + sg, A + sa
    if ep is not None:
        dW, A = dW + ep.double(), A + ep.double().abs()
    DdW = gam(i["D"] + ln + 2)[:, None] * A
    wd = i["Wn"].double().t()[:, :, None] * d[None]
    return {"dz": softsig_bwd(dW, DdW, i["S"], i["Wn"]),
            "dP": (i["dP0"].double() + wd, gam(2) * (i["dP0"].double().abs() + wd.abs())),
            "dsum": (i["dsum0"].double() + d, gam(1) * (i["dsum0"].double().abs() + d.abs()))}


def test_selfcheck_head_backward_bounds():
    i = head_inputs(103, 600, 3, 32, 21)
    sg32 = segsum(i["dWedge"][i["hperm"]], i["node_k"], i["n"])

    def dz32(dW):
        ds = dW * i["Wn"] * (1 - i["Wn"])
        return (ds - (ds * i["S"]).sum(1, keepdim=True)) * i["S"]
    refs = head_bwd_ref(i)
    em = {"dz": dz32((i["dO"][None] * i["P"]).sum(2).t() + sg32), "dP": i["dP0"] + i["Wn"].t()[:, :, None] * i["dO"][None],
          "dsum": i["dsum0"] + i["dO"]}
    check_all(em, refs, "cpu-fp32 head_bwd_node")
    drop = last_group(i["hptr"], i["T"])
    assert_perturbations_rejected(refs, {"dz": (slice(None), 1), "dP": 1}, {"dz": head_bwd_ref(i, drop=drop)["dz"][0]},
                                  "head_bwd_node")
    refz = head_dz_ref(i)
    check_all({"dz": dz32(i["dwh"] + sg32)}, refz, "cpu-fp32 head_dz")
    assert_perturbations_rejected(refz, {"dz": (slice(None), 1)}, {"dz": head_dz_ref(i, drop=drop)["dz"][0]}, "head_dz")
    # head_wsum: len terms, adds only
    sg, sa, ln = head_seg_sums(i)
    refw = {"out": (sg, gam(ln)[:, None] * sa)}
    check_all({"out": sg32}, refw, "cpu-fp32 head_wsum")
    assert_perturbations_rejected(refw, {"out": (slice(None), 1)}, {"out": head_seg_sums(i, drop)[0]}, "head_wsum")


def run_head_bwd(cuda, i, seg=True, ep=None, with_dP=True, with_dsum=True):
    n, R, D = i["n"], i["R"], i["D"]
    dPb = torch.full((R, n + 2, D), NAN, device=cuda)
    dPb[:, 1:1 + n] = i["dP0"].to(cuda)
    Pb = torch.full((R, n + 2, D), NAN, device=cuda)
    Pb[:, 1:1 + n] = i["P"].to(cuda)
    wS, ds = guarded(cuda, n, D)
    ds.copy_(i["dsum0"])
    wz, dz = guarded(cuda, n, R)
    kw = {}
    if seg:
        kw = dict(hseg_ptr=i["hptr"].to(cuda), hperm=i["hperm"].to(I32).to(cuda), dWedge=i["dWedge"].to(cuda))
    ops.head_bwd_node(i["dO"].to(cuda), Pb[:, 1:1 + n], i["S"].to(cuda), i["Wn"].to(cuda),
                      dPb[:, 1:1 + n] if with_dP else None, dz, dsum=ds if with_dsum else None,
                      ep=None if ep is None else ep.to(cuda), **kw)
    guard_intact(wz, "dz")
    guard_intact(wS, "dsum")
    assert bool(torch.isnan(dPb[:, 0]).all()) and bool(torch.isnan(dPb[:, -1]).all())
    return {"dz": dz.cpu(), "dP": dPb[:, 1:1 + n].cpu(), "dsum": ds.cpu()}


@gpu
@pytest.mark.parametrize("n,T", [(1, 5), (257, 3000), (1003, 60)])
@pytest.mark.parametrize("D", [32, 256])
@pytest.mark.parametrize("R", [1, 2, 8])
def test_head_bwd_node_vs_fp64(R, D, n, T, cuda):
    """head_bwd_node: dz against the fp64 softmax-sigmoid backward, dP and dsum against their updates, per element;
    with head segments, with `ep` instead of them, with dP = None, with and without dsum; twice.
    The `ep` form with ep = head_wsum(dWedge) is NOT bitwise the segment form: head_wsum adds a segment in order,
    the segment form adds lane-strided partials (lane sub takes k = beg + sub, beg + sub + D / 4, ...) and reduces
    them with the dot-product parts in one butterfly.  Both associate the same terms, so both are held to the
    segment form's order-independent bound."""
    i = head_inputs(n, T, R, D, 100 * R + D + n)
    refs = head_bwd_ref(i)
    what = f"head_bwd_node R{R} D{D} n{n}"
    a = run_head_bwd(cuda, i)
    check_all(a, refs, what)
    _same(a, run_head_bwd(cuda, i), ("dz", "dP", "dsum"), what + " run twice")
    b = run_head_bwd(cuda, i, with_dP=False, with_dsum=False)
    assert torch.equal(a["dz"], b["dz"])
    assert torch.equal(b["dP"], i["dP0"]) and torch.equal(b["dsum"], i["dsum0"])        # left alone
    # ep = head_wsum(dWedge) in place of the segments
    we, ep = guarded(cuda, n, R)
    ops.head_wsum(i["hptr"].to(cuda), i["hperm"].to(I32).to(cuda), i["dWedge"].to(cuda), ep)
    guard_intact(we, "head_wsum")
    c = run_head_bwd(cuda, i, seg=False, ep=ep.cpu())
    check_all(c, refs, what + " (ep = head_wsum, segment-form reference)")
    check_all(c, head_bwd_ref(i, seg=False, ep=ep.cpu()), what + " (ep form)")
    rnd_ep = torch.randn(n, R, generator=_gen(n))
    check_all(run_head_bwd(cuda, i, seg=False, ep=rnd_ep), head_bwd_ref(i, seg=False, ep=rnd_ep), what + " (random ep)")
    check_all(run_head_bwd(cuda, i, seg=False), head_bwd_ref(i, seg=False), what + " (no segments, no ep)")


@gpu
@pytest.mark.parametrize("n", [1, 31, 33, 1000])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_head_dz_vs_fp64(R, n, cuda):
    """head_dz against fp64 directly (8 lanes per node, idle lanes for R < 8; n around one 32-node block); twice."""
    i = head_inputs(n, 3 * n + 2, R, 32, 7 * R + n)
    refs = head_dz_ref(i)
    outs = []
    for _ in range(2):
        w, dz = guarded(cuda, n, R)
        ops.head_dz(i["S"].to(cuda), i["Wn"].to(cuda), i["hptr"].to(cuda), i["hperm"].to(I32).to(cuda),
                    i["dWedge"].to(cuda), i["dwh"].to(cuda), dz)
        guard_intact(w, "head_dz")
        outs.append(dz.cpu())
    assert_within(outs[0], *refs["dz"], f"head_dz R{R} n{n}")
    assert torch.equal(outs[0], outs[1])


def seq_segsum32(w, hperm, hptr):
    """The fp32 sum of each segment in segment order (adds only: exact to emulate, no FMA can form)."""
    n = hptr.numel() - 1
    beg, ln = hptr[:-1].long(), (hptr[1:] - hptr[:-1]).long()
    acc = torch.zeros(n, w.shape[1], dtype=F32)
    for j in range(int(ln.max()) if n else 0):
        m = ln > j
        acc[m] = acc[m] + w[hperm[beg[m] + j]]
    return acc


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, 5003])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 8])
def test_head_wsum_exact_and_vs_fp64(R, n, cuda):
    """head_wsum: bitwise the sequential fp32 sum in segment order (what the header promises), within the bound of
    fp64, zero rows for nodes without edges; duplicate-free but out-of-order hperm; twice."""
    i = head_inputs(n, 2 * n + 3, R, 32, 13 * R + n)
    sg, sa, ln = head_seg_sums(i)
    outs = []
    for _ in range(2):
        w, o = guarded(cuda, n, R)
        ops.head_wsum(i["hptr"].to(cuda), i["hperm"].to(I32).to(cuda), i["dWedge"].to(cuda), o)
        guard_intact(w, "head_wsum")
        outs.append(o.cpu())
    assert_within(outs[0], sg, gam(ln)[:, None] * sa, f"head_wsum R{R} n{n}")
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], seq_segsum32(i["dWedge"], i["hperm"], i["hptr"]))
    assert bool((outs[0][ln == 0] == 0).all())


@gpu
@pytest.mark.parametrize("M", [0, 1, 255, 257, 5003])
@pytest.mark.parametrize("width", [1, 2, 3, 4, 8, 16])
def test_gather_rows_exact(width, M, cuda):
    """gather_rows: widths 4 and 8 take the 16-byte vector kernel, the others the narrow one; duplicate and
    out-of-order indices; exact.  A src (or dst) whose base is only 4-byte aligned (a view starting at element 1)
    must give the same rows: the launcher sends it to the narrow kernel (it tests both pointers for 16-byte
    alignment), which this asserts through the result."""
    g = _gen(width + 17 * M)
    N = 97
    src = torch.randn(N, width, generator=g)
    idx = torch.randint(0, N, (max(M, 1),), generator=g)
    idx[: max(M, 1) // 2] = idx[0]                         # duplicates
    idx = idx[:M] if M else idx
    want = src[idx[:M]] if M else torch.empty(0, width)
    flat = torch.full((N * width + 5,), NAN, device=cuda)
    srcs = {"aligned": src.to(cuda)}
    flat[1:1 + N * width] = src.flatten().to(cuda)
    srcs["offset"] = flat[1:1 + N * width].view(N, width)
    assert srcs["offset"].data_ptr() % 16 == 4
    idx_d = idx.to(I32).to(cuda)
    for name, s in srcs.items():
        for dst_off in (0, 1):
            whole = torch.full((M * width + width + 1,), NAN, device=cuda)
            dst = whole[dst_off:dst_off + M * width].view(M, width)
            if M:
                ops.gather_rows(s, idx_d, dst)
            else:      # an empty tensor has no device pointer to pass: the C entry directly, valid pointers, M = 0
                assert ops.L.lib().iddgcn_gather_rows_f32(ops._stream(), 0, width, _ptr(s), _ptr(idx_d), _ptr(whole)) == 0
            assert torch.equal(dst.cpu(), want), f"{name} src, dst offset {dst_off}"
            assert bool(torch.isnan(whole[:dst_off]).all()) and bool(torch.isnan(whole[dst_off + M * width:]).all())


# =============================================================================================================
# Slab reduction
# =============================================================================================================
def slabs_ref(slab, n_slabs, n, out0, accumulate, scale, drop_last=False):
    """out = (accumulate ? out : 0) + scale sum_b slab[b]: n_slabs terms in any order (one chain, or 4 / 16 wave
    chains combined through LDS), + 1 for the scale, + 1 for the accumulate."""
    s = slab.double().view(n_slabs, n)
    if drop_last:
        s = s[:-1]
    sc = f32c(scale)
    ref, mag = sc * s.sum(0), abs(sc) * s.abs().sum(0)
    if accumulate:
        ref, mag = ref + out0.double(), mag + out0.double().abs()
    return {"out": (ref, gam(n_slabs + (sc != 1.0) + bool(accumulate)) * mag)}


def slabs_inputs(n, n_slabs, seed):
    """Slabs spanning 6 decades with mixed signs."""
    g = _gen(seed)
    slab = torch.randn(n_slabs * n, generator=g) * 10.0 ** (-6.0 * torch.rand(n_slabs * n, generator=g))
    return slab, torch.randn(n, generator=g)


def slabs_kernel(n, n_slabs, ptr):
    """The launcher's predicate (launch_reduce_slabs), re-derived."""
    few_blocks = n // 4 < 64 * 64 and n_slabs >= 64
    if n % 4 == 0 and n_slabs >= 8 and not few_blocks and ptr % 16 == 0:
        return "slabs4"
    return "split" if n_slabs >= 64 else "plain"


@pytest.mark.parametrize("accumulate,scale", [(0, 1.0), (1, 1.0 / 7)])
def test_selfcheck_reduce_slabs_bounds(accumulate, scale):
    n, ns = 300, 9
    slab, out0 = slabs_inputs(n, ns, 3)
    refs = slabs_ref(slab, ns, n, out0, accumulate, scale)
    s32 = slab.view(ns, n).sum(0) * f32c(scale)
    check_all({"out": out0 + s32 if accumulate else s32}, refs, "cpu-fp32 reduce_slabs")
    assert_perturbations_rejected(refs, {"out": slice(0, n // 3)},
                                  {"out": slabs_ref(slab, ns, n, out0, accumulate, scale, drop_last=True)["out"][0]},
                                  "reduce_slabs")
    assert rejects(slabs_ref(slab, ns, n, out0, accumulate, 1.0 if scale != 1.0 else 0.5)["out"][0], *refs["out"])
    assert rejects(slabs_ref(slab, ns, n, out0, 1 - accumulate, scale)["out"][0], *refs["out"])


SLAB_CASES = [("slabs4", 4 * 64 * 64, 64, 0), ("split", 4 * 64 * 64 - 4, 64, 0), ("plain", 1, 7, 0),
              ("split", 4 * 64 * 64, 64, 1), ("plain", 4 * 64 * 64, 9, 1), ("slabs4", 4 * 64 * 64, 9, 0),
              ("plain", 4 * 64 * 64 - 4, 9, 1), ("split", 1, 64, 0)]


@gpu
@pytest.mark.parametrize("accumulate,scale", [(0, 1.0), (1, 1.0), (0, 1.0 / 7), (1, 1.0 / 7)])
@pytest.mark.parametrize("kernel,n,n_slabs,offset", SLAB_CASES,
                         ids=[f"{k}-n{n}-s{s}-off{o}" for k, n, s, o in SLAB_CASES])
def test_reduce_slabs_vs_fp64(kernel, n, n_slabs, offset, accumulate, scale, cuda):
    """reduce_slabs through each of its three kernels (the intended one named in the id and asserted by re-deriving
    the launcher's predicate from n, n_slabs and the slab's address; a view offset by one float defeats the 16-byte
    path), with accumulate and scale, per element against fp64; twice."""
    slab, out0 = slabs_inputs(n, n_slabs, n + n_slabs)
    refs = slabs_ref(slab, n_slabs, n, out0, accumulate, scale)
    base = torch.empty(n_slabs * n + 8, device=cuda)
    sv = base[offset:offset + n_slabs * n]
    sv.copy_(slab)
    assert slabs_kernel(n, n_slabs, sv.data_ptr()) == kernel
    outs = []
    for _ in range(2):
        w, o = guarded(cuda, n)
        o.copy_(out0) if accumulate else None
        ops.reduce_slabs(sv, n_slabs, o, accumulate=bool(accumulate), scale=scale)
        guard_intact(w, "reduce_slabs")
        outs.append(o.cpu())
    assert_within(outs[0], *refs["out"], f"reduce_slabs[{kernel}] n{n} slabs{n_slabs} acc{accumulate} scale{scale:.3g}")
    assert torch.equal(outs[0], outs[1])


# =============================================================================================================
# alpha, SpMM, SDDMM, narrow TN
# =============================================================================================================
def alpha_inputs(M, D, R, seed, Nx=None):
    """Logits with a spread of about +-60: a softmax without the max subtraction overflows expf."""
    g = _gen(seed)
    Nx = Nx or max(M // 2, 1)
    X = torch.rand(Nx, D, generator=g)
    Wa = torch.randn(D, R, generator=g) * (45.0 / (0.577 * math.sqrt(D)))       # std of a logit ~ 45 for x ~ U(0, 1)
    ba = torch.randn(R, generator=g) * 2.0
    idx = torch.randint(0, Nx, (M,), generator=g)         # duplicates
    return X, Wa, ba, idx


def alpha_ref(X, Wa, ba, idx, live=None):
    """z = x Wa + ba: D fused products and the bias add: gamma(D + 1) (sum|x wa| + |ba|).  e_r = expf(z_r - max):
    the exponent carries z_r's and the max's error and the subtraction's rounding, expf EXP_ULP ulps; the sum of
    R terms gamma(R - 1); the division DIV_ULP ulps.  With every e_q off by a factor exp(d_q), |d_q| <= E (the row's
    largest exponent error), S_r is off by exp(d_r) / sum_q S_q exp(d_q), at most 1 / (S_r + (1 - S_r) exp(-2 E)): the
    errors of a dominant S_r ~ 1 cancel.  Then the sum's and the division's roundings, plus one smallest normal of
    absolute slack where expf underflows.  W = 1 / (1 + expf(-S)) as the DistMult p."""
    x = X.double() if idx is None else X.double()[idx]
    D, R = Wa.shape
    z = x @ Wa.double() + ba.double()
    Dz = gam(D + 1) * (x.abs() @ Wa.double().abs() + ba.double().abs())
    mx, imx = z.max(1, keepdim=True)
    zs = z - mx
    eps = Dz + Dz.gather(1, imx) + U * zs.abs() + EXP_ULP * ULP
    S = torch.softmax(z, 1)
    E = eps.max(1, keepdim=True).values
    rest = S.sum(1, keepdim=True) - S                     # 1 - S_r without cancellation
    rel = (1.0 / (S + rest * torch.exp(-2 * E))) * (1 + gam(R) + DIV_ULP * ULP) - 1.0
    DS = S * rel + 2.0 ** -126
    W, q = torch.sigmoid(S), torch.sigmoid(-S)
    DW = W * q * DS + W * (q * EXP_ULP * ULP + U + DIV_ULP * ULP)
    if live is not None:
        S, W = S * live[:, None], W * live[:, None]
    return {"S": (S, DS), "W": (W, DW)}


def test_selfcheck_alpha_bounds():
    X, Wa, ba, idx = alpha_inputs(200, 64, 3, 4)
    refs = alpha_ref(X, Wa, ba, idx)
    z = X[idx] @ Wa + ba
    e = torch.exp(z - z.max(1, keepdim=True).values)
    S = e / e.sum(1, keepdim=True)
    check_all({"S": S, "W": 1.0 / (1.0 + torch.exp(-S))}, refs, "cpu-fp32 alpha_fwd")
    assert float(z.max()) > 88.8 and float((z.max(1).values - z.min(1).values).max()) > 60.0    # expf(z) overflows
    live = torch.ones(200, dtype=F64)
    live[-(200 % 16 or 16):] = 0                          # the last row group of a block never written (zeros)
    dropped = alpha_ref(X, Wa, ba, idx, live)
    assert_perturbations_rejected(refs, {"S": (slice(None), 1), "W": (slice(None), 1)},
                                  {k: dropped[k][0] for k in refs}, "alpha_fwd")


@gpu
@pytest.mark.parametrize("M", [1, 63, 65, 999, "stride"])
@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_alpha_fwd_vs_fp64(D, R, M, cuda):
    """alpha_fwd: S and W per element against fp64 at logits spread over +-60, every row of S summing to 1 within
    R u, x_idx with duplicates and without x_idx; M around a block and one M past the persistent grid (2048 blocks of
    256 / (D / 4) rows) so that its stride loop iterates; twice."""
    if M == "stride":
        M = 2048 * (256 // (D // 4)) + 5
    X, Wa, ba, idx = alpha_inputs(M, D, R, D + R + M, Nx=min(max(M // 2, 1), 4000))
    for use_idx in (True, False):
        if not use_idx:
            X, idx = X[idx].contiguous(), None
        refs = alpha_ref(X, Wa, ba, idx)
        outs = []
        for _ in range(2):
            wS, S = guarded(cuda, M, R)
            wW, W = guarded(cuda, M, R)
            ops.alpha_fwd(X.to(cuda), Wa.to(cuda), ba.to(cuda), S, W, x_idx=None if idx is None else idx.to(I32).to(cuda))
            guard_intact(wS, "S")
            guard_intact(wW, "W")
            outs.append({"S": S.cpu(), "W": W.cpu()})
        check_all(outs[0], refs, f"alpha_fwd D{D} R{R} M{M} idx{use_idx}")
        _same(outs[0], outs[1], ("S", "W"), "alpha_fwd run twice")
        assert float((outs[0]["S"].double().sum(1) - 1).abs().max()) <= R * U


def csr_case(n_seg, D, seed, n_rows=37, Nx=300):
    """Rows of length 0, 1, 2, 3 and ~1000 (even and odd: the two-in-flight loop's tail), n_seg * n_rows no multiple
    of the rows per block (the last row group partially live)."""
    g = _gen(seed)
    base = [0, 1, 2, 3, 5, 8, 0, 1000, 3, 999, 1, 2]
    ln = torch.tensor([base[(i + s) % len(base)] for s in range(n_seg) for i in range(n_rows)])
    starts = torch.cat([torch.zeros(1, dtype=torch.long), ln.cumsum(0)])
    ptr = torch.cat([starts[s * n_rows:(s + 1) * n_rows + 1] for s in range(n_seg)]).to(I32)
    nnz = int(ln.sum())
    row = torch.repeat_interleave(torch.arange(n_seg * n_rows), ln)
    return dict(n_seg=n_seg, n_rows=n_rows, D=D, ln=ln, beg=starts[:-1], ptr=ptr, nnz=nnz, row=row,
                col=torch.randint(0, Nx, (nnz,), generator=g), vals=torch.randn(nnz, generator=g),
                X=torch.randn(Nx, D, generator=g), Y0=torch.randn(n_seg * n_rows, D, generator=g),
                G=torch.randn(n_seg * n_rows, D, generator=g))


def spmm_ref(c, vals, accumulate, drop=None):
    """Y[row] = (accumulate ? Y0 : 0) + sum_k (vals ? v_k : 1) X[col_k]: len terms, + 1 multiply with vals, + 1 add
    with accumulate."""
    t = c["X"].double()[c["col"]]
    if vals:
        t = t * c["vals"].double()[:, None]
    if drop is not None:
        t = t * (~drop).double()[:, None]
    rows = c["n_seg"] * c["n_rows"]
    ref, mag = segsum(t, c["row"], rows), segsum(t.abs(), c["row"], rows)
    if accumulate:
        ref, mag = ref + c["Y0"].double(), mag + c["Y0"].double().abs()
    return {"Y": (ref, gam(c["ln"].double() + bool(vals) + bool(accumulate))[:, None] * mag)}


def spmm_seq32(c, accumulate):
    """The fp32 sums in CSR order, then the accumulate add: the order the header promises.  Without vals the kernel
    only adds, so no FMA can form and this is exact to emulate."""
    acc = torch.zeros(c["n_seg"] * c["n_rows"], c["D"], dtype=F32)
    for j in range(int(c["ln"].max())):
        m = c["ln"] > j
        acc[m] = acc[m] + c["X"][c["col"][c["beg"][m] + j]]
    return acc + c["Y0"] if accumulate else acc


def sddmm_ref(c, drop=None):
    """out[k] = <G[row_k], X[col_k]>: D terms, one multiply each."""
    q = c["G"].double()[c["row"]] * c["X"].double()[c["col"]]
    if drop is not None:
        q = q * (~drop).double()[:, None]
    return {"out": (q.sum(1), gam(c["D"] + 1) * q.abs().sum(1))}


def odd_tails(c):
    """The stored entries the two-in-flight loops handle last: the final entry of every row of odd length."""
    m = torch.zeros(c["nnz"], dtype=torch.bool)
    odd = (c["ln"] % 2 == 1)
    m[(c["beg"] + c["ln"] - 1)[odd]] = True
    return m


def test_selfcheck_spmm_sddmm_bounds():
    c = csr_case(3, 32, 8, n_rows=13)
    for vals, acc in ((False, False), (True, True)):
        refs = spmm_ref(c, vals, acc)
        t = c["X"][c["col"]] * (c["vals"][:, None] if vals else 1.0)
        y = segsum(t, c["row"], 39)
        check_all({"Y": y + c["Y0"] if acc else y}, refs, "cpu-fp32 spmm")
        if not vals:
            check_all({"Y": spmm_seq32(c, acc)}, refs, "cpu-fp32 sequential spmm")
        assert_perturbations_rejected(refs, {"Y": slice(13, 26)}, {"Y": spmm_ref(c, vals, acc, odd_tails(c))["Y"][0]}, "spmm")
    refs = sddmm_ref(c)
    check_all({"out": (c["G"][c["row"]] * c["X"][c["col"]]).sum(1)}, refs, "cpu-fp32 sddmm")
    seg1 = (c["row"] >= 13) & (c["row"] < 26)
    assert_perturbations_rejected(refs, {"out": seg1}, {"out": sddmm_ref(c, odd_tails(c))["out"][0]}, "sddmm")


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("vals", [False, True])
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_spmm_csr_vs_fp64(D, n_seg, vals, accumulate, cuda):
    """spmm_csr per element against fp64 on rows of length 0, 1, 2, 3, 999 and 1000, with and without vals and
    accumulate, guard row, twice.  Without vals it is also BITWISE the sequential fp32 sum in CSR order (adds only).
    With vals the product x v may be contracted with the add into an FMA, so only the bound applies there."""
    c = csr_case(n_seg, D, D + n_seg)
    refs = spmm_ref(c, vals, accumulate)
    rows = n_seg * c["n_rows"]
    outs = []
    for _ in range(2):
        w, Y = guarded(cuda, rows, D)
        Y.copy_(c["Y0"]) if accumulate else None
        ops.spmm_csr(c["ptr"].to(cuda), c["col"].to(I32).to(cuda), c["vals"].to(cuda) if vals else None, c["X"].to(cuda),
                     Y.view(n_seg, c["n_rows"], D), n_seg, c["n_rows"], accumulate=accumulate)
        guard_intact(w, "spmm_csr")
        outs.append(Y.cpu())
    assert_within(outs[0], *refs["Y"], f"spmm_csr D{D} seg{n_seg} vals{vals} acc{accumulate}")
    assert torch.equal(outs[0], outs[1])
    if not vals:
        assert torch.equal(outs[0], spmm_seq32(c, accumulate))
    if not accumulate:
        assert bool((outs[0][c["ln"] == 0] == 0).all())


@gpu
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_sddmm_csr_vs_fp64(D, n_seg, cuda):
    """sddmm_csr per element against fp64 (the per-element bound replaces 1e-5 sqrt(D) (1 + max)); same rows; twice."""
    c = csr_case(n_seg, D, 2 * D + n_seg)
    refs = sddmm_ref(c)
    outs = []
    for _ in range(2):
        w, o = guarded(cuda, c["nnz"])
        ops.sddmm_csr(c["ptr"].to(cuda), c["col"].to(I32).to(cuda), c["G"].to(cuda).view(n_seg, c["n_rows"], D),
                      c["X"].to(cuda), o, n_seg, c["n_rows"])
        guard_intact(w, "sddmm_csr")
        outs.append(o.cpu())
    assert_within(outs[0], *refs["out"], f"sddmm_csr D{D} seg{n_seg}")
    assert torch.equal(outs[0], outs[1])


def narrow_ref(A, dz, dWa0, dba0, accumulate, M=None):
    """dWa[d][r] = sum_e A[e][d] dz[e][r]: M terms, one multiply, summed over blocks of <= 16 rows and then slabs:
    gamma(M + 1 (+ 1 with accumulate)); dba[r] = sum_e dz[e][r]: gamma(M (+ 1))."""
    M = A.shape[0] if M is None else M
    a, z = A.double()[:M], dz.double()[:M]
    w, wa = a.t() @ z, a.abs().t() @ z.abs()
    b, ba = z.sum(0), z.abs().sum(0)
    if accumulate:
        w, wa, b, ba = w + dWa0.double(), wa + dWa0.double().abs(), b + dba0.double(), ba + dba0.double().abs()
    n = A.shape[0]
    return {"dWa": (w, gam(n + 1 + bool(accumulate)) * wa), "dba": (b, gam(n + bool(accumulate)) * ba)}


def narrow_inputs(M, D, R, seed):
    g = _gen(seed)
    return (torch.rand(max(M, 1), D, generator=g)[:M], torch.randn(max(M, 1), R, generator=g)[:M],
            torch.randn(D, R, generator=g), torch.randn(R, generator=g))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_selfcheck_gemm_tn_narrow_bounds(accumulate):
    M, D, R = 100, 32, 3
    A, dz, w0, b0 = narrow_inputs(M, D, R, 6)
    w0, b0 = w0 * 0.1, b0 * 0.1
    refs = narrow_ref(A, dz, w0, b0, accumulate)
    w, b = A.t() @ dz, dz.sum(0)
    check_all({"dWa": w0 + w if accumulate else w, "dba": b0 + b if accumulate else b}, refs, "cpu-fp32 gemm_tn_narrow")
    dropped = narrow_ref(A, dz, w0, b0, accumulate, M=M - (M % 16 or 16))         # the last block of <= 16 rows
    assert_perturbations_rejected(refs, {"dWa": (slice(None), 1), "dba": 1}, {k: dropped[k][0] for k in refs},
                                  "gemm_tn_narrow")
    assert rejects(narrow_ref(A, dz, w0, b0, 1 - accumulate)["dWa"][0], *refs["dWa"])


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M", [0, 1, 1000, 9001])
@pytest.mark.parametrize("D", [32, 256])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_gemm_tn_narrow_vs_fp64(R, D, M, accumulate, cuda):
    """gemm_tn_narrow: dWa and dba per element against fp64, each with its own bound, with and without accumulate,
    M = 0 (zeros, or the accumulated values unchanged) to M past 1024 blocks' worth of 16-row chains; twice."""
    A, dz, w0, b0 = narrow_inputs(M, D, R, R + D + M)
    refs = narrow_ref(A, dz, w0, b0, accumulate)
    nb = ops.tn_narrow_blocks(M)
    outs = []
    for _ in range(2):
        wW, dWa = guarded(cuda, D, R)
        wB, dba = guarded(cuda, R)
        if accumulate:
            dWa.copy_(w0)
            dba.copy_(b0)
        slab = torch.full(((nb + 1) * (D + 1) * R,), NAN, device=cuda)
        if M:
            ops.gemm_tn_narrow(A.to(cuda), dz.to(cuda), dWa, dba, slab, accumulate=accumulate)
        else:       # an empty tensor has no device pointer to pass: the C entry directly, valid pointers, M = 0
            assert ops.L.lib().iddgcn_gemm_tn_narrow_f32(ops._stream(), 0, D, R, _ptr(slab), _ptr(slab), _ptr(slab), nb,
                                                         _ptr(dWa), _ptr(dba), int(accumulate)) == 0
        guard_intact(wW, "dWa")
        guard_intact(wB, "dba")
        outs.append({"dWa": dWa.cpu(), "dba": dba.cpu()})
    check_all(outs[0], refs, f"gemm_tn_narrow R{R} D{D} M{M} acc{accumulate}")
    _same(outs[0], outs[1], ("dWa", "dba"), "gemm_tn_narrow run twice")
