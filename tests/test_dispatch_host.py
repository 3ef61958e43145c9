"""The C-ABI layer's host-side dispatch, pinned to the library it was refactored from.

tests/golden/dispatch/*.txt were recorded by tools/record_dispatch_golden.py from a library built at the commit before
the dispatch helpers and the row-GEMM plan were introduced; the tests recompute
the same tables from this tree's library.  Nothing here launches a kernel or needs a GPU."""
import os

from iddgcn_amd import _lib
from tests.conftest import GOLDEN, ROOT
from tools import record_dispatch_golden as rec

DISPATCH = os.path.join(GOLDEN, "dispatch")


def _read(name):
    with open(os.path.join(DISPATCH, name)) as f:
        return f.read()


def test_rowgemm_kernel_selection_is_the_parents():
    """iddgcn_rowgemm_kernel_id over the full product of D, precision, R, v_row_stride, v_idx / coef_idx / a_idx
    null or set, act, accumulate, planes and b_trans (record_dispatch_golden.ID_AXES: 115,200 cases) equals the
    recorded table; the first differing case is reported by its arguments.  The id is RowGemmPlan::id() of the plan
    the launching entries launch from, so this pins what runs, not a copy of the selection."""
    want = rec.decode_ids(_read("rowgemm_kernel_id.txt").rstrip("\n"))
    cases = list(rec.id_cases())
    assert len(want) == len(cases) == 115200
    assert len(set(want)) >= 30          # generic, v3 (exact / split / planes / 4-chain) and b3 forms all occur
    got = rec.kernel_ids(_lib.lib())
    for c, w, g in zip(cases, want, got):
        assert g == w, f"iddgcn_rowgemm_kernel_id{c}: {g}, recorded {w}"


def test_refusals_and_check_order_are_the_parents():
    """The return code of every launching entry point of iddgcn_hip.hip over D in {16, 32, 64, 128, 256} x
    R in {-1, 0, 1, 2, 8, 9} x precision in {0..5} (arguments an entry does not have are not passed) equals the
    recorded one: BAD_DIM before BAD_REL before BAD_ARG, per entry.  Every call returns before the entry's first
    launch, in one of two ways (record_dispatch_golden.refusal_entries, read against each entry's code):

    zero size, stand-in data pointers (the entry returns 0 at its size check when nothing else is wrong):
      spmm_csr, sddmm_csr (n_seg = 0), rowgemm_f32, rowgemm_bf16 (M = 0), gemm_tn_batched (n = 0), alpha_fwd,
      combine_f32, combine_bf16, combine_planes (M = 0), distmult_bce_f32, distmult_bce_bf16 (T = 0),
      seg_gather_reduce, tail_seg_reduce_f32 / _bf16 / _head_bf16 / _head_f32, head_bwd_node, head_wsum, head_dz
      (n_nodes = 0), gather_rows (M = 0), reduce_slabs, adam, adam_table (n = 0);
    null data pointers (the entry has no return at size 0 before a launch, so BAD_ARG is the latest it gets):
      rowgemm_batched (n = 1, M = 1: an all-empty D = 256 batch reads the runtime's launch status), gemm_tn_f32,
      gemm_tn_planes, gemm_tn_narrow, gemm_tn_bf16, sigma_tn_bf16, sigma_tn_f32, distmult_bce_heads_f32 / _bf16,
      step_advance."""
    want = {}
    for line in _read("refusals.txt").splitlines():
        name, mode, chars = line.split()
        want[name] = (mode, chars)
    got = rec.refusals(_lib.lib())
    assert sorted(got) == sorted(want)
    launching = [s for s in _lib.SIGNATURES if _is_hot_launcher(s)]
    assert sorted(launching) == sorted(want), "an entry point of iddgcn_hip.hip is not covered"
    cases = rec.refusal_cases()
    for name, (mode, chars) in want.items():
        assert got[name][0] == mode and len(chars) == len(cases) == 180
        assert "?" not in chars          # only 0 and the three refusals: nothing reached the runtime
        for (D, R, P), w, g in zip(cases, chars, got[name][1]):
            assert g == w, f"{name} (D={D}, R={R}, precision={P}, {mode}): returned {g}, recorded {w}"


def _is_hot_launcher(symbol):
    """The symbols of include/iddgcn.h that launch (its pure host queries and the digest excluded)."""
    import re
    header = open(os.path.join(ROOT, "include", "iddgcn.h")).read()
    if not re.search(r"\b%s\s*\(" % symbol, header):
        return False
    return symbol not in ("iddgcn_abi_version", "iddgcn_rowgemm_kernel_id", "iddgcn_gemm_tn_blocks",
                          "iddgcn_gemm_tn_narrow_blocks", "iddgcn_distmult_blocks", "iddgcn_sigma_tn_ranges",
                          "iddgcn_source_sha256")


def test_geometry_functions_are_the_parents():
    """iddgcn_gemm_tn_blocks (all four widths), iddgcn_gemm_tn_narrow_blocks, iddgcn_distmult_blocks and
    iddgcn_sigma_tn_ranges at the tile, cap and int-range boundaries (record_dispatch_golden.GEOM_ARGS)."""
    want = _read("geometry.txt").splitlines()
    got = rec.geometry_text(rec.geometry(_lib.lib())).splitlines()
    assert len(want) == len(got) == 21 * 7
    for w, g in zip(want, got):
        assert g == w, f"{g} (recorded: {w})"
