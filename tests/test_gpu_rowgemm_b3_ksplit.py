"""The bf16x3 gathered-combine forward (rowgemm256_b3_kernel, NV = R in {1, 2}: kernel ids 510 / 520), whose k
dimension is split over wave pairs: C = sigmoid(A S + sum_r coef[e, r] P_r[t_e]) at D = 256 against an fp64 torch
reference, at the project's bar for the bf16x3 mode (max relative error <= max(1.25 x the exact-f32 mode's error on
the same inputs, 1e-6 of max|ref|)), plus the properties the k split could break: the order of the two k halves'
hand-off, determinism, independence of M and of the tiling, and that exactly the rows [0, M) are written."""
import functools

import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import ops

pytestmark = pytest.mark.gpu
D, N = 256, 700
SENTINEL = 7.0            # a sigmoid never returns it
M_RANGES = 32 * 8 * 3 + 17    # several row ranges, ragged last tile
M_BIG = 20_017


def _v_idx(kind, M, g):
    if kind == "none":        # node-aligned: row e combines V row e, 32 distinct rows in every tile
        return None
    if kind == "random":      # up to 32 distinct rows per tile: two DMA rounds
        return torch.randint(0, N, (M,), generator=g)
    t = torch.randint(0, N, (M,), generator=g).sort().values      # tail-sorted edges: 1-3 distinct rows per tile
    if kind == "long_run" and M > 64:                                # one run covering many tiles, ragged at both ends
        a, b = min(45, M // 3), min(45 + 32 * 37 + 5, M - 7)
        t[a:b] = t[a]
    return t


@functools.lru_cache(maxsize=None)
def _case(M, R, kind, a_kind="uniform"):
    """Inputs (fp64 on the GPU), the fp64 reference, and the exact-f32 mode's error against it.  Computed once per
    case and shared; nothing here is modified afterwards."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1000 * R + M + sum(map(ord, kind + a_kind)))
    A = torch.rand(M, D, generator=g, dtype=torch.float64)
    if a_kind == "row_decades":
        A = torch.randn(M, D, generator=g, dtype=torch.float64) * 10 ** (
            12 * torch.rand(M, 1, generator=g, dtype=torch.float64) - 6)
    elif a_kind == "zero_rows":
        A[::3] = 0
    S = torch.randn(D, D, generator=g, dtype=torch.float64)
    nv = M if kind == "none" else N
    W = torch.rand(N, R, generator=g, dtype=torch.float64)
    P = torch.randn(R, nv, D, generator=g, dtype=torch.float64) * 4
    coef = W[torch.randint(0, N, (M,), generator=g)]
    t = _v_idx(kind, M, g)
    A, S, P, coef = A.to(dev), S.to(dev), P.to(dev), coef.to(dev)
    t = None if t is None else t.to(dev)
    rows = P if t is None else P[:, t]
    ref = torch.sigmoid(A @ S + sum(coef[:, r:r + 1] * rows[r] for r in range(R)))
    c = dict(M=M, R=R, A=A.float(), S=S.float(), P=P.float(), coef=coef.float().contiguous(),
             t=None if t is None else t.int(), nv=nv, ref=ref)
    c["exact_err"] = _maxrel(_run(c, "exact")[:M], ref)
    return c


def _maxrel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _kw(c):
    return dict(coef=c["coef"], V=c["P"], v_idx=c["t"], v_rel_stride=c["nv"] * D, act=c.get("act", L.ACT_SIGMOID))


def _run(c, precision="bf16x3", A=None, S=None):
    """One launch into a sentinel-filled C with a guard row; returns the whole buffer (M + 1 rows)."""
    M = c["M"]
    buf = torch.full((M + 1, D), SENTINEL, device=c["A"].device)
    ops.rowgemm(c["A"] if A is None else A, c["S"] if S is None else S, buf[:M], precision=precision, **_kw(c))
    return buf


def _check(c, per_row=None, sentinel=SENTINEL):
    M, R = c["M"], c["R"]
    buf = _run(c)
    out = buf[:M]
    print(f"M={M} R={R}: bf16x3 err {_maxrel(out, c['ref']):.3e}, exact err {c['exact_err']:.3e}")
    assert ops.rowgemm_kernel_id(c["A"], c["S"], out, precision="bf16x3", **_kw(c)) == 500 + 10 * R
    if sentinel is not None:
        assert not (out == sentinel).any(), "an element of C[0:M) was not written"
    assert (buf[M] == SENTINEL).all(), "written past row M"
    assert torch.equal(_run(c), buf), "two launches differ"
    if per_row is not None:
        rel = ((out.double() - c["ref"]).abs().amax(1) / c["ref"].abs().amax(1)).max().item()
        print(f"  per-row err {rel:.3e}")
        assert rel <= per_row, rel
    assert _maxrel(out, c["ref"]) <= max(1.25 * c["exact_err"], 1e-6), (_maxrel(out, c["ref"]), c["exact_err"])
    return out


@pytest.mark.parametrize("kind", ["sorted", "random", "none", "long_run"])
@pytest.mark.parametrize("M", [5, 33, M_RANGES, M_BIG])
@pytest.mark.parametrize("R", [1, 2])
def test_ksplit_forward_vs_fp64(R, M, kind, cuda):
    """R = 1, 2; M below one tile, one row past a tile, several ranges with a ragged last tile, 20,017; v_idx
    sorted (1-3 distinct rows per tile), unsorted (up to 32, two DMA rounds), absent (node-aligned, 32 in every
    tile), with one run over many tiles.  Every element of C[0:M) written, nothing past row M, two launches equal."""
    _check(_case(M, R, kind))


@pytest.mark.parametrize("R", [1, 2])
def test_ksplit_rows_spanning_decades(R, cuda):
    """A's rows span 12 decades.  The sigmoid output meets the bar of the mode; the per-row bar of 1e-5 of the row's
    own largest reference value is set, as in test_rowgemm_bf16x3_vs_fp64, on the linear output (the same launch
    with no activation: A S + combine): a sigmoid of a row scaled by 1e6 turns the fp32 accumulation's rounding
    where the sum cancels (about 1e-7 of the row's scale, in any fp32 kernel) into an error of order 1e-2."""
    c = _case(M_BIG, R, "sorted", "row_decades")
    _check(c)
    rows = c["P"].double()[:, c["t"].long()]
    lin = dict(c, act=L.ACT_NONE, ref=c["A"].double() @ c["S"].double() +
               sum(c["coef"].double()[:, r:r + 1] * rows[r] for r in range(R)))
    lin["exact_err"] = _maxrel(_run(lin, "exact")[:M_BIG], lin["ref"])
    _check(lin, per_row=1e-5, sentinel=None)


@pytest.mark.parametrize("R", [1, 2])
def test_ksplit_zero_rows_give_the_combine_alone(R, cuda):
    """Every third row of A zero: those outputs are bitwise the same call's with A = 0 (sigmoid_fast of the combine
    term alone: both k halves contribute exact zeros)."""
    c = _case(M_BIG, R, "sorted", "zero_rows")
    out = _check(c)
    alone = _run(c, A=torch.zeros_like(c["A"]))[:c["M"]]
    assert torch.equal(out[::3], alone[::3])


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("live", ["low", "high"])
def test_ksplit_handoff_order(live, R, cuda):
    """The k halves' hand-off: with A zero in columns 128..255 (or 0..127) one wave of every pair contributes an
    exact zero partial, which must not change a bit.  The same product with the live half moved to the other
    k half (A's column halves and S's row halves swapped: the same k order inside the half, the other wave of the
    pair computing it) is bitwise equal, and the result meets the bar of the full kernel on that A."""
    c = dict(_case(M_RANGES, R, "sorted"))
    A = c["A"].clone()
    if live == "low":
        A[:, 128:] = 0
    else:
        A[:, :128] = 0
    c["A"] = A
    rows = c["P"].double() if c["t"] is None else c["P"].double()[:, c["t"].long()]
    c["ref"] = torch.sigmoid(A.double() @ c["S"].double() +
                             sum(c["coef"].double()[:, r:r + 1] * rows[r] for r in range(R)))
    c["exact_err"] = _maxrel(_run(c, "exact")[:c["M"]], c["ref"])
    out = _check(c)
    swapped = _run(c, A=torch.cat([A[:, 128:], A[:, :128]], 1).contiguous(),
                   S=torch.cat([c["S"][128:], c["S"][:128]], 0).contiguous())[:c["M"]]
    assert torch.equal(out, swapped)


@pytest.mark.parametrize("kind", ["sorted", "random", "none"])
@pytest.mark.parametrize("R", [1, 2])
def test_ksplit_independent_of_M_and_tiling(R, kind, cuda):
    """A row's result depends on that row only: the first M1 rows of the M2 = 20,017 call (other tiles per range,
    other ranges) are bitwise the M1 call's, for M1 inside a tile, one past a tile, and over several ranges."""
    c = _case(M_BIG, R, kind)
    big = _run(c)[:M_BIG]
    for M1 in (5, 33, M_RANGES):
        s = dict(c, M=M1, A=c["A"][:M1], coef=c["coef"][:M1].contiguous())
        if c["t"] is None:
            s.update(P=c["P"][:, :M1].contiguous(), nv=M1)
        else:
            s["t"] = c["t"][:M1].contiguous()
        assert torch.equal(_run(s)[:M1], big[:M1]), M1
