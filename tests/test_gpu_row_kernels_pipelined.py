"""The node-level row kernels that keep several rows in flight, at the edges of their new loops, against the references
of test_gpu_step_kernels.py (same bounds):

  * alpha_fwd: a lane group walks rows g, g + stride, ...; the persistent grid is 2048 blocks of 256 / (D / 4)
    groups, so `stride` rows give every group exactly one row.  Rows per group of 1, 3, 4, 5 and ragged counts (some
    groups one row more than others).  A form with ALPHA_NF = 4 rows loaded ahead did not gain and is not in the
    library; these are the sizes at which such a loop changes path, kept for the next attempt;
  * gemm_tn_narrow: a block sums its rows in groups of TNN_G = 8 loaded together, then a serial rest.  Rows per block
    of 1, G - 1, G, G + 1, 2 G, a ragged last block, and past 1024 blocks' 16 rows (several groups per block).  Beside
    the fp64 bar, small-integer inputs whose sums are exact in fp32 in any order: every row enters once;
  * gather_rows at width 2 with src and dst at every offset of 0, 1, 2 floats from a 16-byte aligned base: exact.  (An
    8-byte vector form for 8-byte aligned pointers was measured and not kept; these are the
    alignments at which such a form switches kernels.)
"""
import pytest
import torch

from bounds import NAN, U, guard_intact, guarded
from iddgcn_amd import ops
from test_gpu_step_kernels import _gen, _ptr, _same, alpha_inputs, alpha_ref, check_all, narrow_inputs, narrow_ref

gpu = pytest.mark.gpu
I32 = torch.int32
ALPHA_NF, TNN_G = 4, 8                     # rows ahead tried for alpha; iddgcn_hip.hip TNN_G


def alpha_stride(D):
    return 2048 * (256 // (D // 4))


ALPHA_M = {"one": lambda s: 1, "nf-1": lambda s: (ALPHA_NF - 1) * s, "nf": lambda s: ALPHA_NF * s,
           "nf+1": lambda s: (ALPHA_NF + 1) * s, "ragged": lambda s: ALPHA_NF * s + 5,
           "ragged-short": lambda s: (ALPHA_NF - 2) * s + s // 2 + 3}


@gpu
@pytest.mark.parametrize("M", list(ALPHA_M))
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("D", [64, 256])
def test_alpha_fwd_rows_per_group(D, R, M, cuda):
    M = ALPHA_M[M](alpha_stride(D))
    X, Wa, ba, idx = alpha_inputs(M, D, R, D + R + M, Nx=min(max(M // 2, 1), 3000))
    Xd, Wad, bad = X.to(cuda), Wa.to(cuda), ba.to(cuda)
    refs = alpha_ref(X, Wa, ba, idx)
    outs = []
    for _ in range(2):
        wS, S = guarded(cuda, M, R)
        wW, W = guarded(cuda, M, R)
        ops.alpha_fwd(Xd, Wad, bad, S, W, x_idx=idx.to(I32).to(cuda))
        guard_intact(wS, "S")
        guard_intact(wW, "W")
        outs.append({"S": S.cpu(), "W": W.cpu()})
    check_all(outs[0], refs, f"alpha_fwd D{D} R{R} M{M}")
    _same(outs[0], outs[1], ("S", "W"), "alpha_fwd run twice")
    assert float((outs[0]["S"].double().sum(1) - 1).abs().max()) <= R * U
    # without x_idx on the gathered rows: the same rows, bitwise
    wS, S = guarded(cuda, M, R)
    wW, W = guarded(cuda, M, R)
    ops.alpha_fwd(Xd[idx.to(cuda)].contiguous(), Wad, bad, S, W)
    guard_intact(wS, "S")
    guard_intact(wW, "W")
    _same(outs[0], {"S": S.cpu(), "W": W.cpu()}, ("S", "W"), "alpha_fwd with and without x_idx")


@gpu
def test_alpha_fwd_no_rows(cuda):
    buf = torch.full((64,), NAN, device=cuda)
    assert ops.L.lib().iddgcn_alpha_fwd_f32(ops._stream(), 0, 256, 2, _ptr(buf), None, _ptr(buf), _ptr(buf), _ptr(buf),
                                            _ptr(buf)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# rows per block: 1, G - 1, G, G + 1, 2 G; 17 rows: two blocks of 9 and 8; 1000: 16 per block, the last 8; past
# 16 x 1024 rows: 26 per block (three groups and a rest of 2), the last block ragged
NARROW_M = [1, TNN_G - 1, TNN_G, TNN_G + 1, 2 * TNN_G, 17, 1000, 1024 * 25 + 3]


def run_narrow(cuda, A, dz, w0, b0, accumulate):
    M, D = A.shape
    R = dz.shape[1]
    nb = ops.tn_narrow_blocks(M)
    wW, dWa = guarded(cuda, D, R)
    wB, dba = guarded(cuda, R)
    if accumulate:
        dWa.copy_(w0)
        dba.copy_(b0)
    slab = torch.full(((nb + 1) * (D + 1) * R,), NAN, device=cuda)
    ops.gemm_tn_narrow(A.to(cuda), dz.to(cuda), dWa, dba, slab, accumulate=accumulate)
    guard_intact(wW, "dWa")
    guard_intact(wB, "dba")
    return {"dWa": dWa.cpu(), "dba": dba.cpu()}


@gpu
@pytest.mark.parametrize("M", NARROW_M)
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("D", [64, 256])
def test_gemm_tn_narrow_row_groups(D, R, M, cuda):
    A, dz, w0, b0 = narrow_inputs(M, D, R, R + D + M)
    for accumulate in (False, True):
        refs = narrow_ref(A, dz, w0, b0, accumulate)
        a = run_narrow(cuda, A, dz, w0, b0, accumulate)
        check_all(a, refs, f"gemm_tn_narrow R{R} D{D} M{M} acc{accumulate}")
        _same(a, run_narrow(cuda, A, dz, w0, b0, accumulate), ("dWa", "dba"), "gemm_tn_narrow run twice")
    # small integers: every partial sum is an integer below 2^24, exact in fp32 whatever the order
    g = _gen(M + D)
    Ai = torch.randint(0, 8, (M, D), generator=g).float()
    zi = torch.randint(-8, 9, (M, R), generator=g).float()
    e = run_narrow(cuda, Ai, zi, w0, b0, False)
    assert torch.equal(e["dWa"].double(), Ai.double().t() @ zi.double()), "dWa: a row dropped or entered twice"
    assert torch.equal(e["dba"].double(), zi.double().sum(0)), "dba: a row dropped or entered twice"


@gpu
@pytest.mark.parametrize("M", [0, 1, 255, 257, 5003])
def test_gather_rows_width2(M, cuda):
    """Offsets in floats of src and dst from a 16-byte aligned base (16-, 4- and 8-byte aligned pointers): all exact,
    nothing written outside dst."""
    g = _gen(31 * M + 2)
    N, width = 97, 2
    src = torch.randn(N, width, generator=g)
    idx = torch.randint(0, N, (max(M, 1),), generator=g)
    idx[: max(M, 1) // 2] = idx[0]                         # duplicates
    want = src[idx[:M]]
    idx_d = idx.to(I32).to(cuda)
    for s_off in (0, 1, 2):
        flat = torch.full((N * width + 8,), NAN, device=cuda)
        flat[s_off:s_off + N * width] = src.flatten().to(cuda)
        s = flat[s_off:s_off + N * width].view(N, width)
        assert s.data_ptr() % 16 == 4 * s_off
        for d_off in (0, 1, 2):
            whole = torch.full((M * width + 8,), NAN, device=cuda)
            dst = whole[d_off:d_off + M * width].view(M, width)
            if M:
                assert dst.data_ptr() % 16 == 4 * d_off
                ops.gather_rows(s, idx_d, dst)
            else:      # an empty tensor has no device pointer to pass: the C entry directly, valid pointers, M = 0
                assert ops.L.lib().iddgcn_gather_rows_f32(ops._stream(), 0, width, _ptr(s), _ptr(idx_d), _ptr(whole)) == 0
            assert torch.equal(dst.cpu(), want), f"src offset {s_off}, dst offset {d_off}"
            assert bool(torch.isnan(whole[:d_off]).all()) and bool(torch.isnan(whole[d_off + M * width:]).all())
