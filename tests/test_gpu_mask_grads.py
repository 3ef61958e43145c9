"""The gradient mask_explain_kernel computes (ops.mask_explain), read bit for bit from its Adam moments, against the
float64 autograd of tests/ref_mask_grads.py.

The handle: with m = v = 0, one epoch and b1 = b2 = 0.5 the kernel leaves m = g / 2 and v = fl(g g) / 2 (both halvings
exact), so 2 m is its fp32 gradient with respect to the mask logit, and init_e puts the mask anywhere.  The moments are
per entry of the full adjacency and the triples share entries, so every query is measured alone (qids = [j]) on freshly
zeroed state.

Bar, per query: |2 m - g64| <= max(4 max|g32 - g64|, 1e-5 max|g64|) (bounds.query_bar), g64 and g32 the float64 and
float32 autograd of the same formulation: the kernel's output never enters a bar.  tests/test_mask_grads_host.py shows
what this bar rejects (a cut softmax path, a layer's missing AE gradient, a gradient scaled by 1.001) and that the 1e-5
bar on final masked values (tests/test_gpu_mask_batched.py) does not.  Every test prints its worst error / bar."""
import numpy as np
import pytest
import torch

from iddgcn_amd import explain as X
from iddgcn_amd import ops
from tests import ref_mask_grads as RM
from tests.bounds import guard_intact, guarded, query_bar
from tests.test_mask_batched_host import EMPTY, N_ENT, N_REL, fold4_case
from tests.test_mask_grads_host import (check_input_conditions, host_candidates, large_degree_case, ratios_of,
                                        synthetic)

pytestmark = pytest.mark.gpu
KINDS = ("gnnexplainer", "iddgcn")
SENTINEL = -12345
CH = 512                                           # the kernel's staging pass
ES_ROWS = {64: 448, 32: 896}                       # candidates whose E rows it keeps in LDS
F32_MIN_NORMAL = 2.0 ** -126


class Case:
    """One (graph, weights, queries, kind) on the device, its candidate lists and its reference gradients."""

    def __init__(self, N, R, D, tri, q, init, params, ratios, dev):
        self.N, self.R, self.D, self.tri, self.q, self.params, self.ratios, self.dev = N, R, D, tri, q, params, ratios, dev
        self.kind = "gnnexplainer" if ratios is None else "iddgcn"
        self.init = np.asarray(init, np.float32)
        dadj, self.qptr, self.entry, self.crel, self.ccol, self.crole = host_candidates(tri, q, N, R)
        self.row, self.col, self.rel, _ = X._entry_table(dadj, real=False)
        self.total = dadj.total_nnz
        self.init_e = self.init[self.row, self.col]
        g = lambda a, dt=np.int32: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)  # noqa: E731
        self.g = g
        w = lambda k: g(params[k], np.float32)  # noqa: E731
        self.layers = tuple(tuple(w(f"{nm}{l}") for l in (1, 2, 3)) for nm in ("K", "S", "Wa", "ba"))
        self.E, self.relw = w("E"), w("rel")
        self.lists = (g(q[:, 0]), g(q[:, 1]), g(q[:, 2]), g(self.qptr, np.int64), g(self.entry), g(self.crel),
                      g(self.ccol), g(self.crole))
        self.d_ratios = None if ratios is None else g(ratios, np.float32)
        self._ref = None

    def cand(self, j):
        return slice(int(self.qptr[j]), int(self.qptr[j + 1]))

    def ref(self):
        """(g64, g32) per query at the initial mask, once."""
        if self._ref is None:
            a = (self.params, self.tri, self.q, self.N, self.R, self.init, self.ratios)
            self._ref = tuple([x for x, _ in RM.mask_grads(*a, dt)] for dt in (torch.float64, torch.float32))
            check_input_conditions(self.q, self.qptr, self.crole, self._ref[0], self.kind)
        return self._ref

    def mask_of(self, init_e):
        """An (R, N, N) mask for the reference from one logit per stored entry."""
        mask = np.zeros((self.R, self.N, self.N))
        mask[self.rel, self.row, self.col] = init_e
        return mask

    def alpha_table(self, epochs, epochs_base):
        n = epochs_base + len(self.q) * epochs
        return (np.float32(1e-3) * (1 + np.arange(n) % 7)).astype(np.float32)     # a step that depends on its index

    def run(self, j, init_e=None, m0=0.0, v0=0.0, steps0=0, epochs=1, epochs_base=0, b1=0.5, b2=0.5, eps=1e-7,
            alpha=None):
        """Query j alone.  m, v, steps hold the given values at its candidates, NaN / a sentinel everywhere else and
        in one slot past the end; out is NaN with one slot past its end.  Checks that nothing but the query's own
        entries was written and returns (m, v, steps, out, alpha) of its candidates (numpy)."""
        dev, sl = self.dev, self.cand(j)
        e = torch.as_tensor(self.entry[sl].astype(np.int64), device=dev)
        init_e = self.init_e if init_e is None else init_e
        alpha = self.alpha_table(epochs, epochs_base) if alpha is None else alpha
        mw, m = guarded(dev, self.total)
        vw, v = guarded(dev, self.total)
        sw, steps = guarded(dev, self.total, fill=SENTINEL, dtype=torch.int32)
        ow, out = guarded(dev, len(self.entry))
        for t, x, dt in ((m, m0, np.float32), (v, v0, np.float32), (steps, steps0, np.int32)):
            t[e] = self.g(np.full(len(self.entry[sl]), x, dt) if np.isscalar(x) else x, dt)
        K, S, Wa, ba = self.layers
        ops.mask_explain(self.E, K, S, Wa, ba, self.relw, *self.lists, self.g(init_e, np.float32), m, v, steps,
                         self.g(alpha, np.float32), out, self.g([j]), [0, 1], epochs, epochs_base, b1, b2, eps,
                         self.d_ratios)
        torch.cuda.synchronize()
        other = torch.ones(self.total + 1, dtype=torch.bool, device=dev)
        other[e] = False
        what = f"query {j}"
        assert bool(torch.isnan(mw[other]).all()) and bool(torch.isnan(vw[other]).all()), what
        assert bool((sw[other] == SENTINEL).all()), what
        guard_intact(mw, what), guard_intact(vw, what), guard_intact(ow, what)
        written = ~torch.isnan(ow)
        assert int(written.sum()) == sl.stop - sl.start and bool(written[sl].all()), what
        return (m[e].cpu().numpy(), v[e].cpu().numpy(), steps[e].cpu().numpy(), out[sl].cpu().numpy(),
                np.asarray(alpha, np.float32))

    def check_gradient(self, j, m, g64, g32):
        """2 m within the bar of g64; m exactly +0 where the reference gradient is exactly 0.  Returns error / bar."""
        bar = query_bar(g64, g32)
        err = float(np.abs(2.0 * m.astype(np.float64) - g64).max())
        assert err <= bar, (j, tuple(self.q[j]), err, bar)
        zero = g64 == 0
        assert not m.view(np.int32)[zero].any(), j
        return err / bar


def check_first_step(c, j, m, v, steps, out, alpha, init_e, step0, eps=1e-7):
    """What one epoch from zero moments must leave besides the gradient."""
    f = np.float32
    g = f(2) * m
    want_v = (g * g).astype(f) * f(0.5)
    exact = (want_v >= F32_MIN_NORMAL) | (g == 0)
    assert np.array_equal(v.view(np.int32)[exact], want_v.view(np.int32)[exact]), j
    assert exact.any(), j
    assert np.array_equal(steps, np.full(len(steps), step0 + 1, np.int32)), j
    d = np.float64
    x = init_e.astype(d) - d(alpha[step0]) * m.astype(d) / (np.sqrt(v.astype(d)) + d(f(eps)))
    want = 1.0 / (1.0 + np.exp(-x))
    ulp = np.spacing(want.astype(f)).astype(d)
    off = float((np.abs(out.astype(d) - want) / ulp).max())
    assert off <= 4.0, (j, off)
    return off


def one_epoch_everywhere(c, init_e=None, g64=None, g32=None, first_step=True):
    """Every query of the case alone, one epoch from zero moments: (worst error / bar, worst out distance in ulp,
    the bitwise gradients)."""
    if g64 is None:
        g64, g32 = c.ref()
    init = c.init_e if init_e is None else init_e
    worst, off, grads = 0.0, 0.0, []
    for j in range(len(c.q)):
        sl = c.cand(j)
        m, v, steps, out, alpha = c.run(j, init_e=init_e)
        assert len(m) == len(g64[j])
        if len(m):
            worst = max(worst, c.check_gradient(j, m, g64[j], g32[j]))
            if first_step:
                off = max(off, check_first_step(c, j, m, v, steps, out, alpha, init[c.entry[sl]], j))
        grads.append(np.float32(2) * m)
    return worst, off, grads


# -- the cases, built once -------------------------------------------------------------------------------------------
_CASES = {}


def synthetic_on(dev, D, R, kind, variant="plain"):
    key = (D, R, kind, variant)
    if key not in _CASES:
        tri, q, init, params, ratios = synthetic(D, R, kind, wa_scale=8.0 if variant == "wa8" else 1.0,
                                                 saturate=variant == "saturate")
        _CASES[key] = Case(40, R, D, tri, q, init, params, ratios, dev)
    return _CASES[key]


SHAPES = [(32, 1), (32, 3), (32, 8), (64, 1), (64, 4), (64, 5), (64, 8)]
FIRST = ([(D, R, kind, "plain") for D, R in SHAPES for kind in KINDS] +
         [(64, 8, "iddgcn", "wa8"), (32, 3, "gnnexplainer", "wa8"), (64, 4, "iddgcn", "saturate"),
          (64, 5, "gnnexplainer", "saturate")])


# -- 1. the gradient at the initial mask -----------------------------------------------------------------------------
@pytest.mark.parametrize("D,R,kind,variant", FIRST)
def test_gradient_at_the_initial_mask(D, R, kind, variant, cuda):
    """Every kernel width, R = 1 (no softmax gradient), R = 5 and 8 at D = 64 (the second relation of a lane group),
    softmax weights x 8 and saturated sigmoids.  Per query: 2 m within the bar, v = fl(g g) / 2 bitwise, m = +0 on the
    column-only candidates under GNNExplainer, steps, the stepped mask within 4 fp32 ulp, nothing else written; the
    triple without a candidate (GNNExplainer only) writes nothing at all."""
    c = synthetic_on(cuda, D, R, kind, variant)
    worst, off, _ = one_epoch_everywhere(c)
    print(f"gradient at init D={D} R={R} {kind} {variant}: worst error / bar {worst:.3f}, "
          f"stepped mask within {off:.2f} ulp")
    if kind == "gnnexplainer":
        assert c.qptr[EMPTY] == c.qptr[EMPTY + 1]        # run() has checked that every buffer is untouched


# -- 2. away from the initial mask -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,R", [(32, 3), (64, 8), (64, 4)])
def test_gradient_away_from_the_initial_mask(D, R, kind, cuda):
    """init_e = init + U(-3, 3) per stored entry (different per relation at one (row, col)): masked values between
    about 0.05 and 0.95."""
    c = synthetic_on(cuda, D, R, kind)
    init_e = (c.init_e + np.random.default_rng(11).uniform(-3, 3, c.total)).astype(np.float32)
    a = (c.params, c.tri, c.q, c.N, c.R, c.mask_of(init_e), c.ratios)
    g64, g32 = ([x for x, _ in RM.mask_grads(*a, dt)] for dt in (torch.float64, torch.float32))
    moved = max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(g64, c.ref()[0]) if y.size)
    assert moved > 0.1                                   # the reference gradient is another one here
    worst, _, _ = one_epoch_everywhere(c, init_e, g64, g32, first_step=False)
    print(f"gradient away from init D={D} R={R} {kind}: worst error / bar {worst:.3f}")


# -- 3. staging boundaries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 32])
def test_gradient_across_staging_boundaries(D, kind, cuda):
    """The large-degree graph: more than 1024 candidates (three staging passes of 512), past the E rows kept in LDS
    (448 at D = 64, 896 at D = 32: the others come from global memory, skipped where both multipliers are 0), with
    relation segments that straddle every one of these boundaries.  At D = 32 every candidate past 896 is a
    column-only one (all skipped); at D = 64 both kinds occur past 448.  All of this is asserted from the lists."""
    N, R, tri, q, init, params = large_degree_case(D)
    c = Case(N, R, D, tri, q, init, params, ratios_of(kind, R), cuda)
    inside = crosses_pass = crosses_es = skipped = from_global = False
    for j in range(len(q)):
        sl = c.cand(j)
        n, crel = sl.stop - sl.start, c.crel[sl]
        start = np.searchsorted(crel, np.arange(R + 1))              # the kernel's rstart
        for r in range(R):
            a, b = start[r], start[r + 1]
            inside |= bool(0 < a < n and a % CH != 0 and b > a)     # a relation boundary strictly inside a pass
            crosses_pass |= bool(a // CH != (b - 1) // CH and b > a)
            crosses_es |= bool(a < ES_ROWS[D] < b)
        skipped |= bool((c.crole[sl][ES_ROWS[D]:] == 0).any())
        from_global |= bool((c.crole[sl][ES_ROWS[D]:] != 0).any())
    assert max(np.diff(c.qptr)) > 2 * CH and inside and crosses_pass and crosses_es and skipped
    assert from_global == (D == 64)      # past 896 this graph has column-only candidates alone: every read is skipped
    worst, off, _ = one_epoch_everywhere(c, first_step=False)
    print(f"gradient across staging boundaries D={D} {kind}: candidates {np.diff(c.qptr).tolist()}, "
          f"worst error / bar {worst:.3f}")


# -- 4. fold 4, trained weights --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_fold4(kind, golden, cuda):
    """The bundled fold-4 weights (D = 64, R = 4), the first 6 test triples."""
    adjacency, test = fold4_case(golden)
    w = golden("weights_fold4.npz")
    init = np.random.default_rng(123).standard_normal((N_ENT, N_ENT)).astype(np.float32)
    ratios = None if kind == "gnnexplainer" else (0.4, 0.4, 0.1, 0.1)
    c = Case(N_ENT, N_REL, 64, adjacency, test[:6], init, w, ratios, cuda)
    g64, g32 = c.ref()
    rel_bar = [query_bar(a, b) / np.abs(a).max() for a, b in zip(g64, g32)]
    worst, _, _ = one_epoch_everywhere(c, first_step=False)
    print(f"gradient fold 4 {kind}: bars {min(rel_bar):.1e} .. {max(rel_bar):.1e} of max|g|, "
          f"worst error / bar {worst:.3f}")


# -- 5. lazy decay and the moment update -----------------------------------------------------------------------------
def test_lazy_decay_and_moment_update(cuda):
    """epochs_base = 5 and query index 2: step0 = 7.  Preset moments and last-step counters giving gaps of 0, 1 and 3:
    m = m0 0.5^gap + (g - m0 0.5^gap) / 2 and the same for v with g g, g the bitwise gradient of the query (it does
    not depend on the moments).  Bounds 8 u (|m0| 0.5^gap + |g|) and 8 u (v0 0.5^gap + g g): at most four roundings
    and powf's error; a gap off by one is a factor 2."""
    c = synthetic_on(cuda, 64, 8, "iddgcn")
    j, base = 2, 5
    m, _, _, _, _ = c.run(j)
    g = (np.float32(2) * m).astype(np.float64)
    n = len(g)
    assert n >= 6 and np.all(g != 0)
    rng = np.random.default_rng(7)
    scale = np.abs(g).max()
    m0 = (rng.standard_normal(n) * scale).astype(np.float32)
    v0 = (rng.uniform(0.1, 1.0, n) * scale * scale).astype(np.float32)
    gap = np.array([0, 1, 3])[np.arange(n) % 3]
    step0 = base + j * 1
    assert step0 == 7
    m1, v1, steps, _, _ = c.run(j, m0=m0, v0=v0, steps0=(step0 - gap).astype(np.int32), epochs_base=base)
    dm, dv = m0.astype(np.float64) * 0.5 ** gap, v0.astype(np.float64) * 0.5 ** gap
    want_m, want_v = dm + (g - dm) * 0.5, dv + (g * g - dv) * 0.5
    u8 = 8 * 2.0 ** -24
    rm = np.abs(m1 - want_m) / (u8 * (np.abs(dm) + np.abs(g)))
    rv = np.abs(v1 - want_v) / (u8 * (dv + g * g))
    print(f"lazy decay: worst error / bound m {rm.max():.3f}, v {rv.max():.3f}")
    assert rm.max() <= 1 and rv.max() <= 1
    assert np.array_equal(steps, np.full(n, step0 + 1, np.int32))
    # a gap off by one would be far outside: from the expected values alone
    for wrong in (gap + 1, np.maximum(gap - 1, 0)):
        moved = wrong != gap
        dmw = m0.astype(np.float64) * 0.5 ** wrong
        assert np.all(np.abs(dmw + (g - dmw) * 0.5 - want_m)[moved] > 100 * (u8 * (np.abs(dm) + np.abs(g)))[moved])


# -- 6. several epochs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,R", [(32, 3), (64, 8)])
def test_three_epochs_with_a_smooth_step(D, R, cuda):
    """b1 = b2 = 0, eps = 1e-2, alpha = 1, three epochs: m is the last epoch's gradient and the step
    alpha g / (|g| + eps) is smooth in g, so the fp32 and float64 trajectories cannot part on a sign.  The masks move
    by up to 1.5; the third gradient is more than 100 bars from the first (from the reference alone), so a kernel that
    never re-read its mask would fail."""
    c = synthetic_on(cuda, D, R, "iddgcn")
    g1 = c.ref()[0]
    hyper = dict(epochs=3, alphas=np.ones(3), b1=0.0, b2=0.0, eps=1e-2)
    worst = worst_out = 0.0
    for j in range(len(c.q)):
        a = (c.params, c.tri, c.q[j:j + 1], c.N, c.R, c.init, c.ratios)
        (g64, f64), = RM.trajectory(*a, dtype=torch.float64, **hyper)
        (g32, _), = RM.trajectory(*a, dtype=torch.float32, **hyper)
        bar = query_bar(g64, g32)
        assert np.abs(g64 - g1[j]).max() > 100 * bar, j
        m, _, steps, out, _ = c.run(j, epochs=3, b1=0.0, b2=0.0, eps=1e-2,
                                    alpha=np.ones(3 * len(c.q), np.float32))
        err = float(np.abs(m.astype(np.float64) - g64).max())
        assert err <= bar, (j, err, bar)
        worst = max(worst, err / bar)
        worst_out = max(worst_out, float(np.abs(out - f64).max()))
        assert np.array_equal(steps, np.full(len(steps), 3 * j + 3, np.int32))
    print(f"three epochs D={D} R={R}: worst error / bar {worst:.3f}, max |masked value - reference| {worst_out:.2e}")
    assert worst_out <= 1e-5
