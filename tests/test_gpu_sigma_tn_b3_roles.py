"""The fused sigma' + dS pass over fp32 tables (iddgcn_sigma_tn_f32, sigma_tn_b3_kernel) in its role-split form: twelve
waves per workgroup, waves 0-7 the sigma' column groups (they stage, convert and store), waves 8-11 the dS TN alone,
32 of the half's 128 16x16 tiles each.

What can go wrong in that form and is asked here:
  * a dS tile dropped, written twice or written by the wrong wave: the owner map test puts exactly one 1 into each of
    the 256 tiles at a position of its own;
  * a buffer reused under the twelve-wave barrier before every wave is done with it: M = 4097, 8193 and 12289 give two,
    three and four tiles per range (iddgcn_sigma_tn_ranges) with a ragged or short last range, so each of the two LDS
    buffers is refilled while the other is read; M = 1, 32, 33 are one ragged tile, one full tile and a full plus a
    ragged one, M = 4096 is 128 ranges of one tile;
  * a sum in another order or a product missing: on integer-valued data (dO and S integers in [-4, 4], X in
    {1/4, 1/2, 3/4}: every product and partial sum exact in fp32, test_gpu_mfma_gemms.py's family A) dS and dX are
    bitwise the fp64 result;
  * a value that depends on what the slab or dS held before, or on the run: three launches on NaN-filled outputs give
    identical bits and no NaN.
"""
import pytest
import torch

from iddgcn_amd import ops
from test_gpu_mfma_gemms import LIM, assert_bitwise, run_stn, stn_case, stn_ref

pytestmark = pytest.mark.gpu
D = 256
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("M", [1, 32, 33, 4096, 4097, 8193, 12289])
def test_roles_exact_integers_bitwise(M, cuda):
    c = stn_case(M, "int")
    refs = stn_ref(c)
    # every sum of moduli below 2^24 (dX's also after the 1/16 grid of x (1 - x)): fp32 holds each partial sum exactly
    assert float(refs["dS"][1].max()) * 4 < LIM and float(refs["dX"][1].max()) * 16 < LIM
    out, nr = run_stn(c, cuda, f"sigma_tn roles int M{M}")
    assert nr == int(ops.sigma_tn_slab_floats(M)) // (D * D)
    for k in ("dS", "dX"):
        assert_bitwise(out[k], refs[k][0], f"sigma_tn[bf16x3] roles int M{M} {k}")


def test_roles_every_ds_tile_has_one_owner(cuda):
    """256 rows (eight 32-row tiles, one per range: the smallest table with a row for each of the 16 x 16 tiles of dS).
    Row r carries one 1 in X (column i) and one 1 in dO (column j), so it adds exactly 1 at dS[i, j]; (i, j) lies in tile
    (37 r + 11) mod 256 at the in-tile position (r mod 16, (r / 16 + 5 r) mod 16): every tile is hit once, no two at the
    same in-tile position, and rows that share a 32-row tile feed tiles of different owner waves.  X in {0, 1} makes
    x (1 - x) = 0, so dX is 0 everywhere."""
    M = 256
    r = torch.arange(M)
    tile = (37 * r + 11) % 256
    pi, pj = r % 16, (r // 16 + 5 * (r % 16)) % 16
    assert len(set(tile.tolist())) == 256 and len(set((16 * pi + pj).tolist())) == 256
    i, j = 16 * (tile // 16) + pi, 16 * (tile % 16) + pj
    X, dO = torch.zeros(M, D), torch.zeros(M, D)
    X[r, i] = 1.0
    dO[r, j] = 1.0
    want = torch.zeros(D, D)
    want[i, j] = 1.0
    assert int(want.sum()) == 256 and all(int(want[16 * a:16 * a + 16, 16 * b:16 * b + 16].sum()) == 1
                                          for a in range(16) for b in range(16))
    S = torch.randint(-4, 5, (D, D), generator=torch.Generator().manual_seed(5)).float()
    slab = torch.full((ops.sigma_tn_slab_floats(M),), NAN, device=cuda)
    dS = torch.full((D, D), NAN, device=cuda)
    Xd = X.to(cuda)
    ops.sigma_tn(dO.to(cuda), Xd, S.to(cuda), dS, slab, precision="bf16x3")
    got = dS.cpu()
    bad = (_bits(got) != _bits(want)).nonzero()
    assert len(bad) == 0, f"{len(bad)} elements of dS differ from the owner map, first at {tuple(bad[0].tolist())}: " \
                          f"got {got[tuple(bad[0].tolist())].item()!r}"
    assert bool((Xd == 0).all()), "dX: x (1 - x) = 0 on a 0/1 table"


@pytest.mark.parametrize("M", [33, 8193])
def test_roles_three_launches_same_bits_on_nan_outputs(M, cuda):
    g = torch.Generator().manual_seed(M)
    X = torch.rand(M, D, generator=g).to(cuda)
    dO = (torch.randn(M, D, generator=g) * 1e-3).to(cuda)
    S = (torch.randn(D, D, generator=g) / 16).to(cuda)
    runs = []
    for _ in range(3):
        slab = torch.full((ops.sigma_tn_slab_floats(M),), NAN, device=cuda)
        dS = torch.full((D, D), NAN, device=cuda)
        Xi = X.clone()
        ops.sigma_tn(dO, Xi, S, dS, slab, precision="bf16x3")
        runs.append((_bits(dS).cpu(), _bits(Xi).cpu(), bool(torch.isfinite(dS).all()), bool(torch.isfinite(Xi).all())))
    for n, (s, x, fs, fx) in enumerate(runs):
        assert fs and fx, f"launch {n}: a NaN of the prefilled slab / dS came through"
        assert torch.equal(s, runs[0][0]), f"launch {n}: dS bits differ from launch 0"
        assert torch.equal(x, runs[0][1]), f"launch {n}: dX bits differ from launch 0"
