"""Thin torch-facing wrappers over the C-ABI (one call = one library entry point).

torch is used only as the device-memory / stream provider: every wrapper takes
CUDA(HIP) tensors, validates shapes/dtypes on the host (so a bad shape never
reaches a kernel), and passes raw pointers plus torch's current stream.
Index VALUES (entity / relation ids) are validated where they enter the
product path — graph.get_adj_mats / DeviceAdjacency / ScoredEdges (host or
device build, error flag) and the layer-level calls in model.py; direct callers
of these wrappers can turn on per-call range checks with IDDGCN_CHECK_INDICES=1.
"""
import ctypes
import os

import torch

from . import _lib as L

_F32 = torch.float32
_BF16 = torch.bfloat16
_I32 = torch.int32
_I64 = torch.int64
_U8 = torch.uint8
_F64 = torch.float64


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_PRECISION = {"exact": L.GEMM_EXACT_F32, "split": L.GEMM_SPLIT_F16, "exact4": L.GEMM_F32_4CHAIN,
              "bf16x3": L.GEMM_BF16X3, "bf16": L.GEMM_BF16,
              L.GEMM_EXACT_F32: L.GEMM_EXACT_F32, L.GEMM_SPLIT_F16: L.GEMM_SPLIT_F16,
              L.GEMM_F32_4CHAIN: L.GEMM_F32_4CHAIN, L.GEMM_BF16X3: L.GEMM_BF16X3, L.GEMM_BF16: L.GEMM_BF16}


def _prec(precision):
    """GEMM operand precision of one call (include/iddgcn.h IDDGCN_GEMM_*): "exact" / "split" / "exact4" (f32
    MFMA with four interleaved accumulation chains: row GEMMs, plain form at D = 256) / "bf16x3" (every fp32
    operand split exactly into three bf16 pieces, six bf16 MFMA products, fp32 accumulation) / "bf16" (bf16 edge
    tables only: every MFMA operand rounded to bf16, one product per term) or the constant."""
    if precision not in _PRECISION:
        raise L.IddgcnError(f"precision must be 'exact', 'split', 'exact4', 'bf16x3' or 'bf16', got {precision!r}")
    return _PRECISION[precision]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, dtype, shape=None, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise L.IddgcnError(f"{name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise L.IddgcnError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.IddgcnError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.IddgcnError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


# Index RANGES are checked here only when IDDGCN_CHECK_INDICES=1 (one device reduction + host sync per
# index array, a debug mode): the product path's indices come from graph.ScoredEdges / DeviceAdjacency,
# whose builders validate every entity / relation id on the host or in the device build (error flag).
CHECK_INDEX_RANGES = os.environ.get("IDDGCN_CHECK_INDICES", "0") == "1"


def _idx_ok(idx, n_rows, bound, name):
    """dtype / shape / contiguity of an int32 index array; with CHECK_INDEX_RANGES (or always for a
    CPU-resident check-free size-0 array) also 0 <= idx < bound."""
    if idx is None:
        return
    _req(idx, _I32, (n_rows,), name)
    if CHECK_INDEX_RANGES and bound is not None and idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= int(bound):
            raise L.IddgcnError(f"{name}: index out of range [0, {int(bound)}): min {lo}, max {hi}")


def _req_rows(t, shape, name, optional=False):
    """An fp32 GPU view of the given shape whose rows are contiguous (unit inner stride, row stride = the last dim;
    the outer strides are free: a node-row range of an (R, N, D) table keeps its relation stride, the engine's
    ws.P / ws.W / ws.X their layer stride).  Returns the outer strides (elements), zeros for an optional None."""
    if t is None and optional:
        return (0,) * (len(shape) - 2)
    if t is None or not t.is_cuda or t.dtype != _F32:
        raise L.IddgcnError(f"{name} must be an fp32 GPU tensor (no CPU fallback)")
    if tuple(t.shape) != tuple(shape) or t.stride(-1) != 1 or t.stride(-2) != shape[-1]:
        raise L.IddgcnError(f"{name} must be {tuple(shape)} with contiguous rows")
    return t.stride()[:-2]


def _ptr_ascends(p, limit, name, exact=False):
    """With CHECK_INDEX_RANGES (one host copy): the CSR pointer p ascends within [0, limit], or, ``exact``, from 0
    to exactly limit."""
    if not CHECK_INDEX_RANGES or p.numel() < 2:
        return
    q = p.cpu()
    lo, hi = int(q[0]), int(q[-1])
    if bool((q[1:] < q[:-1]).any()) or ((lo != 0 or hi != limit) if exact else (lo < 0 or hi > limit)):
        raise L.IddgcnError(f"{name} must ascend " + (f"from 0 to {limit}" if exact else f"within [0, {limit}]"))


def _req_layers(K, S, Wa, ba, R, D, who):
    """The three layers' K (R, D, D), S (D, D), Wa (D, R), ba (R,): fp32 GPU tensors, none missing."""
    if not (len(K) == len(S) == len(Wa) == len(ba) == 3):
        raise L.IddgcnError(f"{who}: K, S, Wa, ba must hold the three layers")
    for l in range(3):
        for x, shape, nm in ((K[l], (R, D, D), "K"), (S[l], (D, D), "S"), (Wa[l], (D, R), "Wa"), (ba[l], (R,), "ba")):
            if x is None:
                raise L.IddgcnError(f"{who}: every layer's K, S, Wa, ba is required ({nm}{l + 1} is None)")
            _req(x, _F32, shape, f"{nm}{l + 1}")


def _req_queries(h, r, t, qptr, crel, ccol, crole, N, R):
    """The queries (h, r, t) (Q,) of a per-triple kernel and their candidate lists: qptr (Q + 1,) int64 into crel /
    ccol / crole (C,).  Returns (Q, C)."""
    Q, C = h.shape[0], crel.shape[0]
    for idx, n, bound, nm in ((h, Q, N, "h"), (r, Q, R, "r"), (t, Q, N, "t"), (crel, C, R, "crel"), (ccol, C, N, "ccol"),
                              (crole, C, 4, "crole")):
        _idx_ok(idx, n, bound, nm)
    _req(qptr, _I64, (Q + 1,), "qptr")
    return Q, C


def _set_ptrs(a, **fields):
    """Device pointers into the fields of a MaskExplainArgs / ExplainCurvesArgs: a tensor, None, or the three layers'
    tensors (the K / S / Wa / ba arrays) per field."""
    for nm, t in fields.items():
        if isinstance(t, (list, tuple)):
            for l in range(3):
                getattr(a, nm)[l] = t[l].data_ptr()
        else:
            setattr(a, nm, None if t is None else t.data_ptr())


def _triples3(t, name):
    _req(t, _I64, None, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise L.IddgcnError(f"{name} must be (n, 3), got {tuple(t.shape)}")


def _by_dtype(t, f32, bf16):
    """The library entry of a pair by the element type of t: ``bf16`` for a bf16 tensor, else ``f32``."""
    return getattr(L.lib(), bf16 if t.dtype == _BF16 else f32)


def _same_size(n, who, **tensors):
    for nm, t in tensors.items():
        if t.numel() != n:
            raise L.IddgcnError(f"{who}: {nm} size mismatch")


def _out(t, shape, dtype, device, name):
    """An output of the given shape and dtype: allocated unless given, a given one checked."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(t, dtype, shape, name)
    return t


def spmm_csr(row_ptr, col, vals, X, Y, n_seg, n_rows, accumulate=False):
    D = X.shape[1]
    _req(row_ptr, _I32, (n_seg * (n_rows + 1),), "row_ptr")
    _req(col, _I32, None, "col")
    _req(vals, _F32, None, "vals")
    _req(X, _F32, None, "X")
    _req(Y, _F32, (n_seg, n_rows, D), "Y")
    L.check(L.lib().iddgcn_spmm_csr_f32(_stream(), n_seg, n_rows, D, _ptr(row_ptr), _ptr(col), _ptr(vals),
                                        _ptr(X), _ptr(Y), int(accumulate)), "spmm_csr")


def sddmm_csr(row_ptr, col, G, X, out, n_seg, n_rows):
    """out[k] = <G[s][row(k)], X[col[k]]> over the batched CSR (gradient w.r.t. adjacency values)."""
    D = X.shape[1]
    _req(row_ptr, _I32, (n_seg * (n_rows + 1),), "row_ptr")
    _req(col, _I32, None, "col")
    _req(G, _F32, (n_seg, n_rows, D), "G")
    _req(X, _F32, None, "X")
    _req(out, _F32, (col.shape[0],), "out")
    L.check(L.lib().iddgcn_sddmm_csr_f32(_stream(), n_seg, n_rows, D, _ptr(row_ptr), _ptr(col), _ptr(G), _ptr(X),
                                         _ptr(out)), "sddmm_csr")


def rowgemm(A, B, C, **kw):
    """C = epilogue(A[a_idx] · B^(T)) (include/iddgcn.h, iddgcn_rowgemm_f32); see _rowgemm_args.  bf16 A
    (the bf16-feature mode's edge tables) selects iddgcn_rowgemm_bf16: A, aux and C are then bf16."""
    args = _rowgemm_args(A, B, C, **kw)
    L.check(_by_dtype(A, "iddgcn_rowgemm_f32", "iddgcn_rowgemm_bf16")(_stream(), ctypes.byref(args)), "rowgemm")


def rowgemm_kernel_id(A, B, C, **kw):
    """Which kernel rowgemm(A, B, C, **kw) runs (iddgcn_rowgemm_kernel_id): 300 + 10*NV + ... (+2000 split
    operands) for the D=256 v3 pipeline, 100 the register-staged one."""
    args = _rowgemm_args(A, B, C, **kw)
    return int(L.lib().iddgcn_rowgemm_kernel_id(ctypes.byref(args)))


def rowgemm_batched(calls):
    """Independent row GEMMs of one width in one launch (iddgcn_rowgemm_batched_f32).  calls: list of
    (A, B, C, kwargs) as for rowgemm; at most L.ROWGEMM_BATCH (25)."""
    if not calls:
        return
    arr = (L.RowGemmArgs * len(calls))(*[_rowgemm_args(A, B, C, **kw) for A, B, C, kw in calls])
    L.check(L.lib().iddgcn_rowgemm_batched_f32(_stream(), arr, len(calls)), "rowgemm_batched")


def _rowgemm_args(A, B, C, *, a_idx=None, b_trans=False, accumulate=False, coef=None, coef_idx=None, V=None,
                  v_idx=None, v_rel_stride=0, v_row_stride=None, act=L.ACT_NONE, aux=None, M=None, planes=0,
                  precision="exact"):
    """C = epilogue(A[a_idx] · B^(T)) (include/iddgcn.h, iddgcn_rowgemm_f32).  planes: L.PLANES_* flags,
    which of A / C / aux are pre-split planes tables (fp32-shaped tensors holding [hi | lo] fp16 rows;
    D = 256, split GEMM mode).  precision, per call: "exact" (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain),
    "exact4" (the same MFMA, four interleaved accumulation chains: the node-level projections), "bf16x3" (fp32
    operands split exactly into three bf16 pieces, six bf16 MFMA products, fp32 accumulation) or "split"
    (split-fp16 operands, 22 significant bits); D < 256 runs exact f32 in every mode."""
    D = B.shape[0]
    M = C.shape[0] if M is None else M
    R = 0 if coef is None else coef.shape[-1]
    et = A.dtype if A.dtype == _BF16 else _F32         # edge-table element type (A, C, aux)
    _req(A, et, None, "A")
    _req(B, _F32, (D, D), "B")
    _req(C, et, (M, D), "C")
    if A.dim() != 2 or A.shape[1] != D:
        raise L.IddgcnError(f"A must be (rows, {D})")
    if a_idx is None and A.shape[0] < M:
        raise L.IddgcnError("A has fewer rows than C")
    _idx_ok(a_idx, M, A.shape[0], "a_idx")
    if R:
        _req(coef, _F32, None, "coef")
        _req(V, _F32, None, "V")
        _idx_ok(coef_idx, M, coef.shape[0], "coef_idx")
        vrows = (int(v_rel_stride) // int(D if v_row_stride is None else v_row_stride)
                 if (v_row_stride is None or v_row_stride) and v_rel_stride else None)
        _idx_ok(v_idx, M, vrows, "v_idx")
    if act == L.ACT_DSIGMOID:
        _req(aux, et, (M, D), "aux")
    return L.RowGemmArgs(
        M=M, D=D, A=_ptr(A), a_idx=_ptr(a_idx), B=_ptr(B), b_trans=int(b_trans), C=_ptr(C),
        accumulate=int(accumulate), R=R, coef=_ptr(coef), coef_idx=_ptr(coef_idx), V=_ptr(V),
        v_idx=_ptr(v_idx), v_rel_stride=int(v_rel_stride),
        v_row_stride=int(D if v_row_stride is None else v_row_stride), act=int(act), aux=_ptr(aux),
        planes=int(planes), precision=_prec(precision))


def tn_blocks(M, D):
    return int(L.lib().iddgcn_gemm_tn_blocks(int(M), int(D)))


def _tn_prec(precision):
    """Operand precision of a TN GEMM: "exact", "bf16x3" or "split" (include/iddgcn.h; the TN kernels take no
    four-chain form, so "exact4" is refused here rather than by the C side's IDDGCN_E_BAD_ARG)."""
    if precision in ("exact4", "bf16", L.GEMM_F32_4CHAIN, L.GEMM_BF16):
        raise L.IddgcnError(f"gemm_tn: precision {precision!r} is a row-GEMM form; use 'exact', 'bf16x3' or 'split'")
    return _prec(precision)


def gemm_tn(A, B, C, slab, accumulate=False, a_planes=False, precision="exact"):
    """C (+)= A^T B; bf16 A and B (the bf16-feature mode) select iddgcn_gemm_tn_bf16; a_planes: A is a
    pre-split planes table (iddgcn_gemm_tn_planes_f32, D = 256, split GEMM mode); precision: the fp32 form's
    operand precision ("exact", "bf16x3" or "split" at D = 256; other widths exact f32)."""
    prec = _tn_prec(precision)
    M, D = A.shape
    et = _BF16 if A.dtype == _BF16 else _F32
    _req(A, et, (M, D), "A")
    _req(B, et, (M, D), "B")
    _req(C, _F32, (D, D), "C")
    nb = tn_blocks(M, D)
    if slab.numel() < nb * D * D:
        raise L.IddgcnError("gemm_tn slab too small")
    args = (_stream(), M, D, _ptr(A), _ptr(B), _ptr(slab), nb, _ptr(C), int(accumulate))
    if a_planes:
        if et != _F32 or prec != L.GEMM_SPLIT_F16:
            raise L.IddgcnError("gemm_tn: planes A takes an fp32-shaped table in the split mode")
        rc = L.lib().iddgcn_gemm_tn_planes_f32(*args)
    elif et == _BF16:
        rc = L.lib().iddgcn_gemm_tn_bf16(*args)
    else:
        rc = L.lib().iddgcn_gemm_tn_f32(*args, prec)
    L.check(rc, "gemm_tn")


def sigma_tn(dO, X, S, dS, slab, precision="exact"):
    """A layer's edge backward GEMM pair in one pass (the autodiff of IDDGCN.py:62-63,79): dS = X^T dO (overwritten)
    and X = (dO S^T) * X (1 - X) in place.
      * bf16 tables (iddgcn_sigma_tn_bf16, ABI 11): the weights as a bf16 hi + lo pair ("exact", "split", "bf16x3"),
        or rounded to bf16 ("bf16", as rowgemm's bf16 form);
      * fp32 tables (iddgcn_sigma_tn_f32, ABI 12): precision "bf16x3" only (every operand split exactly into three
        bf16 pieces; X bitwise the bf16x3 row GEMM's sigma' output)."""
    M, D = X.shape
    prec = _prec(precision)
    et = _BF16 if X.dtype == _BF16 else _F32
    _req(X, et, (M, D), "X")
    _req(dO, et, (M, D), "dO")
    _req(S, _F32, (D, D), "S")
    _req(dS, _F32, (D, D), "dS")
    _req(slab, _F32, None, "slab")
    if et == _BF16 and prec not in (L.GEMM_EXACT_F32, L.GEMM_SPLIT_F16, L.GEMM_BF16X3, L.GEMM_BF16):
        raise L.IddgcnError(f"sigma_tn: precision {precision!r} is not a form of the bf16 pass")
    if et == _F32 and prec != L.GEMM_BF16X3:
        raise L.IddgcnError(f"sigma_tn: fp32 tables take precision 'bf16x3' only, got {precision!r}")
    fn = _by_dtype(X, "iddgcn_sigma_tn_f32", "iddgcn_sigma_tn_bf16")
    L.check(fn(_stream(), M, D, _ptr(dO), _ptr(X), _ptr(S), _ptr(slab), slab.numel(), _ptr(dS), prec), "sigma_tn")


def sigma_tn_slab_floats(M, D=256):
    return int(L.lib().iddgcn_sigma_tn_ranges(M)) * D * D


def gemm_tn_batched(entries, slab, precision="exact"):
    """Up to L.TN_BATCH independent C (+)= A^T B, entries = [(A, B, C, accumulate), ...] (fp32, same D), in one
    launch (iddgcn_gemm_tn_batched_f32, ABI 5; one launch at D = 256 in the split and bf16x3 modes); slab holds
    the partials of all entries.  precision: as gemm_tn."""
    prec = _tn_prec(precision)
    if not entries:
        return
    if len(entries) > L.TN_BATCH:
        raise L.IddgcnError(f"gemm_tn_batched: at most {L.TN_BATCH} entries")
    D = entries[0][0].shape[1]
    arr = (L.TnArgs * len(entries))()
    for k, (A, B, C, acc) in enumerate(entries):
        M = A.shape[0]
        _req(A, _F32, (M, D), "A")
        _req(B, _F32, (M, D), "B")
        _req(C, _F32, (D, D), "C")
        arr[k] = L.TnArgs(M, _ptr(A), _ptr(B), _ptr(C), int(bool(acc)))
    _req(slab, _F32, None, "slab")
    L.check(L.lib().iddgcn_gemm_tn_batched_f32(_stream(), D, arr, len(entries), _ptr(slab), slab.numel(), prec),
            "gemm_tn_batched")


def tn_narrow_blocks(M):
    return int(L.lib().iddgcn_gemm_tn_narrow_blocks(int(M)))


def gemm_tn_narrow(A, dz, dWa, dba, slab, accumulate=False):
    M, D = A.shape
    R = dz.shape[1]
    _req(dz, _F32, (M, R), "dz")
    _req(dWa, _F32, (D, R), "dWa")
    _req(dba, _F32, (R,), "dba")
    nb = tn_narrow_blocks(M)
    if slab.numel() < (nb + 1) * (D + 1) * R:
        raise L.IddgcnError("gemm_tn_narrow slab too small")
    L.check(L.lib().iddgcn_gemm_tn_narrow_f32(_stream(), M, D, R, _ptr(A), _ptr(dz), _ptr(slab), nb, _ptr(dWa),
                                              _ptr(dba), int(accumulate)), "gemm_tn_narrow")


def alpha_fwd(X, Wa, ba, S_out, W_out, x_idx=None, M=None):
    D, R = Wa.shape
    M = S_out.shape[0] if M is None else M
    _req(X, _F32, None, "X")
    _req(Wa, _F32, (D, R), "W_alpha")
    _req(ba, _F32, (R,), "b_alpha")
    _req(S_out, _F32, (M, R), "S_out")
    _req(W_out, _F32, (M, R), "W_out")
    _idx_ok(x_idx, M, X.shape[0], "x_idx")
    L.check(L.lib().iddgcn_alpha_fwd_f32(_stream(), M, D, R, _ptr(X), _ptr(x_idx), _ptr(Wa), _ptr(ba),
                                         _ptr(S_out), _ptr(W_out)), "alpha_fwd")


def combine(Y, coef, V, out, *, y_idx=None, coef_idx=None, v_idx=None, v_rel_stride=None, planes_out=False):
    """out = sigmoid(Y[y_idx] + sum_r coef[coef_idx, r] V_r[v_idx]) (iddgcn_combine_f32).  A bf16 out (the
    bf16-feature mode) or planes_out (out a pre-split planes table, D = 256) take the run form:
    y_idx and v_idx the same array, per-row coefficients."""
    M, D = out.shape
    R = coef.shape[-1]
    if out.dtype == _BF16 or planes_out:
        if y_idx is None or v_idx is not y_idx or coef_idx is not None:
            raise L.IddgcnError("combine into bf16 / planes: y_idx and v_idx must be the same array, no coef_idx")
        _req(out, _BF16 if out.dtype == _BF16 else _F32, (M, D), "out")
        _req(Y, _F32, None, "Y")
        _req(coef, _F32, (M, R), "coef")
        _idx_ok(y_idx, M, Y.shape[0], "y_idx")
        vrs = V.shape[1] * D if v_rel_stride is None else v_rel_stride
        fn = _by_dtype(out, "iddgcn_combine_planes_f32", "iddgcn_combine_bf16")
        L.check(fn(_stream(), M, D, R, _ptr(Y), _ptr(y_idx), _ptr(coef), _ptr(V), int(vrs), _ptr(out)), "combine_run")
        return
    _req(Y, _F32, None, "Y")
    _req(coef, _F32, None, "coef")
    _req(V, _F32, None, "V")
    _req(out, _F32, (M, D), "out")
    vrs = V.shape[1] * D if v_rel_stride is None else v_rel_stride
    for n, ix, bound in (("y_idx", y_idx, Y.shape[0]), ("coef_idx", coef_idx, coef.shape[0]),
                         ("v_idx", v_idx, int(vrs) // D)):
        _idx_ok(ix, M, bound, n)
    L.check(L.lib().iddgcn_combine_f32(_stream(), M, D, R, _ptr(Y), _ptr(y_idx), _ptr(coef), _ptr(coef_idx),
                                       _ptr(V), _ptr(v_idx), int(vrs), _ptr(out)), "combine")


def distmult_blocks(T):
    return int(L.lib().iddgcn_distmult_blocks(int(T)))


def distmult_bce(Xh, h_idx, Xt, r_idx, rel, *, t_idx=None, y=None, scale=1.0, p_out=None, s_out=None, ds_out=None,
                 do_out=None, drel_slab=None, loss_slab=None):
    """DistMult score (IDDGCN.py:103-109): p_out = sigmoid(s), s_out = s (the pre-sigmoid logit); with y the
    Keras BCE and both backward seeds."""
    T = h_idx.shape[0]
    R, D = rel.shape
    _req(h_idx, _I32, (T,), "h_idx")
    _req(r_idx, _I32, (T,), "r_idx")
    _req(Xh, _F32, None, "Xh")
    _req(Xt, _BF16 if Xt.dtype == _BF16 else _F32, None, "Xt")
    _req(rel, _F32, (R, D), "rel")
    _req(y, _F32, (T,), "y")
    _req(p_out, _F32, (T,), "p_out")
    _req(s_out, _F32, (T,), "s_out")
    _idx_ok(h_idx, T, Xh.shape[0], "h_idx")
    _idx_ok(t_idx, T, Xt.shape[0], "t_idx")
    _idx_ok(r_idx, T, R, "r_idx")
    if t_idx is None and Xt.shape[0] < T:
        raise L.IddgcnError("distmult: Xt has fewer rows than scored edges")
    nb = distmult_blocks(T)
    if y is not None:
        _req(ds_out, _F32, (T,), "ds_out")
        _req(do_out, Xt.dtype, (T, D), "do_out")
        if drel_slab.numel() < nb * R * D or loss_slab.numel() < nb:
            raise L.IddgcnError("distmult slabs too small")
    fn = _by_dtype(Xt, "iddgcn_distmult_bce_f32", "iddgcn_distmult_bce_bf16")
    L.check(fn(_stream(), T, D, R, _ptr(Xh), _ptr(h_idx), _ptr(Xt), _ptr(t_idx), _ptr(r_idx), _ptr(rel), _ptr(y),
               float(scale), _ptr(p_out), _ptr(s_out), _ptr(ds_out), _ptr(do_out), _ptr(drel_slab), _ptr(loss_slab),
               nb), "distmult_bce")
    return nb


def distmult_bce_heads(seg_ptr, perm, Xh, Xt, r_idx, rel, y, do_out, dXh, drel_slab, loss_slab, *, scale=1.0,
                      p_out=None, s_out=None, ds_out=None):
    """Training DistMult + BCE + tail seed (do_out) + head seed (dXh) in one pass over head segments.
    y=None selects the prediction seed (gradient of scale * sum_e p_e; loss slabs sum p_e)."""
    T = r_idx.shape[0]
    n_nodes, D = dXh.shape
    R = rel.shape[0]
    _req(seg_ptr, _I32, (n_nodes + 1,), "seg_ptr")
    _req(perm, _I32, (T,), "perm")
    _req(r_idx, _I32, (T,), "r_idx")
    et = _BF16 if Xt.dtype == _BF16 else _F32
    _req(Xh, _F32, (n_nodes, D), "Xh")
    _req(Xt, et, (T, D), "Xt")
    _req(rel, _F32, (R, D), "rel")
    _req(y, _F32, (T,), "y")
    _req(do_out, et, (T, D), "do_out")
    _req(dXh, _F32, (n_nodes, D), "dXh")
    _req(p_out, _F32, (T,), "p_out")
    _req(s_out, _F32, (T,), "s_out")
    _req(ds_out, _F32, (T,), "ds_out")
    nb = distmult_blocks(T)
    if drel_slab.numel() < nb * R * D or loss_slab.numel() < nb:
        raise L.IddgcnError("distmult slabs too small")
    fn = _by_dtype(Xt, "iddgcn_distmult_bce_heads_f32", "iddgcn_distmult_bce_heads_bf16")
    L.check(fn(_stream(), n_nodes, D, R, _ptr(seg_ptr), _ptr(perm), _ptr(Xh), _ptr(Xt), _ptr(r_idx), _ptr(rel),
               _ptr(y), float(scale), _ptr(p_out), _ptr(s_out), _ptr(ds_out), _ptr(do_out), _ptr(dXh),
               _ptr(drel_slab), _ptr(loss_slab), nb), "distmult_bce_heads")
    return nb


def seg_gather_reduce(seg_ptr, rows, out, *, perm=None, coef=None, r_idx=None, rel=None, X=None):
    n_nodes, D = out.shape
    _req(seg_ptr, _I32, (n_nodes + 1,), "seg_ptr")
    _req(out, _F32, (n_nodes, D), "out")
    L.check(L.lib().iddgcn_seg_gather_reduce_f32(_stream(), n_nodes, D, _ptr(seg_ptr), _ptr(perm), _ptr(coef),
                                                 _ptr(r_idx), _ptr(rel), _ptr(rows), _ptr(X), _ptr(out)),
            "seg_gather_reduce")


def tail_seg_reduce_head(seg_ptr, W, dO, P, dP, dWedge, head_dO, Wn, dwh, dsum=None):
    """tail_seg_reduce with per-edge W fused with the head chain's node terms of the same layer: dP[r][n] = tail sum
    + Wn[n][r] head_dO[n], dsum[n] = tail sum + head_dO[n], dwh[n][r] = <head_dO[n], P_r[n]>; the head backward is
    then head_dz.  bf16 rows at R = 8, D = 256 (iddgcn_tail_seg_reduce_head_bf16, ABI 9) or fp32 rows at R <= 2,
    D = 256 (iddgcn_tail_seg_reduce_head_f32, round 12: dP, dsum bitwise tail_seg_reduce + head_bwd_node), by the dtype
    of dO; other shapes are refused.  P, dP: (R, n, D) views with contiguous rows (a node-row range: seg_ptr the
    matching slice of the tail pointers, absolute edge offsets)."""
    R, n_nodes, D = P.shape
    _req(seg_ptr, _I32, (n_nodes + 1,), "seg_ptr")
    ps, = _req_rows(P, (R, n_nodes, D), "P")
    dps, = _req_rows(dP, (R, n_nodes, D), "dP", optional=True)
    _req(dsum, _F32, (n_nodes, D), "dsum")
    _req(head_dO, _F32, (n_nodes, D), "head_dO")
    _req(Wn, _F32, (n_nodes, R), "Wn")
    _req(dwh, _F32, (n_nodes, R), "dwh")
    _req(dO, _BF16 if dO.dtype == _BF16 else _F32, None, "dO")
    _req(W, _F32, None, "W")
    _req(dWedge, _F32, None, "dWedge")
    if W.shape[0] != dO.shape[0]:
        raise L.IddgcnError("tail_seg_reduce_head: per-edge W must have one row per edge")
    fn = _by_dtype(dO, "iddgcn_tail_seg_reduce_head_f32", "iddgcn_tail_seg_reduce_head_bf16")
    L.check(fn(_stream(), n_nodes, D, R, _ptr(seg_ptr), _ptr(W), _ptr(dO), _ptr(P), ps, _ptr(dP), dps, _ptr(dsum),
               _ptr(dWedge), _ptr(head_dO), _ptr(Wn), _ptr(dwh)), "tail_seg_reduce_head")


def head_dz(Ssm, W, hseg_ptr, hperm, dWedge, dwh, dz):
    """The head backward after tail_seg_reduce_head (iddgcn_head_dz_f32, ABI 9): dW_r = dwh[n][r] + the head
    segment's dWedge rows, then the softmax-sigmoid backward into dz (n, R)."""
    n_nodes, R = dz.shape
    for t, nm in ((Ssm, "Ssm"), (W, "W"), (dwh, "dwh"), (dz, "dz")):
        _req(t, _F32, (n_nodes, R), nm)
    _req(hseg_ptr, _I32, (n_nodes + 1,), "hseg_ptr")
    _req(hperm, _I32, None, "hperm")
    _req(dWedge, _F32, None, "dWedge")
    L.check(L.lib().iddgcn_head_dz_f32(_stream(), n_nodes, R, _ptr(Ssm), _ptr(W), _ptr(hseg_ptr), _ptr(hperm),
                                       _ptr(dWedge), _ptr(dwh), _ptr(dz)), "head_dz")


def tail_seg_reduce(seg_ptr, h_idx, W, dO, P, dP, dWedge, dsum=None):
    """Tail segment sums of a layer's backward (include/iddgcn.h iddgcn_tail_seg_reduce_*): dP[r][n] = sum over the
    tail segment of n of W[e][r] dO[e], dWedge[e][r] = <dO[e], P_r[t_e]> (and dsum[n] = sum of dO[e]).  P, dP: (R, n,
    D) views with contiguous rows (a node-row range: seg_ptr the matching slice of the tail pointers)."""
    R, n_nodes, D = P.shape
    _req(seg_ptr, _I32, (n_nodes + 1,), "seg_ptr")
    ps, = _req_rows(P, (R, n_nodes, D), "P")
    dps, = _req_rows(dP, (R, n_nodes, D), "dP", optional=True)
    _req(dsum, _F32, (n_nodes, D), "dsum")
    if h_idx is None and W.shape[0] != dO.shape[0]:
        raise L.IddgcnError("tail_seg_reduce: per-edge W must have one row per edge")
    _req(dO, _BF16 if dO.dtype == _BF16 else _F32, None, "dO")
    fn = _by_dtype(dO, "iddgcn_tail_seg_reduce_f32", "iddgcn_tail_seg_reduce_bf16")
    L.check(fn(_stream(), n_nodes, D, R, _ptr(seg_ptr), _ptr(h_idx), _ptr(W), _ptr(dO), _ptr(P), ps, _ptr(dP), dps,
               _ptr(dsum), _ptr(dWedge)), "tail_seg_reduce")


def head_bwd_node(dO, P, Ssm, W, dP, dz, *, hseg_ptr=None, hperm=None, dWedge=None, dsum=None, ep=None):
    """Head-chain backward of one layer over the rows of dO (include/iddgcn.h iddgcn_head_bwd_node_f32).  P and dP
    are (R, n, D) views whose rows are contiguous (a row range of the (R, N, D) node tables keeps their relation
    stride); ``ep``: (n, R) head sums of dWedge computed elsewhere (node-partitioned steps)."""
    R, n_nodes, D = P.shape
    _req(dO, _F32, (n_nodes, D), "dO")
    _req(Ssm, _F32, (n_nodes, R), "Ssm")
    _req(W, _F32, (n_nodes, R), "W")
    _req(dz, _F32, (n_nodes, R), "dz")
    _req(dsum, _F32, (n_nodes, D), "dsum")
    _req(ep, _F32, (n_nodes, R), "ep")
    ps, = _req_rows(P, (R, n_nodes, D), "P")
    # dP None (ABI 9): its head term was added by tail_seg_reduce_head
    dps, = _req_rows(dP, (R, n_nodes, D), "dP", optional=True)
    L.check(L.lib().iddgcn_head_bwd_node_f32(_stream(), n_nodes, D, R, _ptr(dO), _ptr(P), ps, _ptr(Ssm), _ptr(W),
                                             _ptr(hseg_ptr), _ptr(hperm), _ptr(dWedge), _ptr(ep), _ptr(dP), dps,
                                             _ptr(dsum), _ptr(dz)), "head_bwd_node")


def head_wsum(hptr, hperm, w, out):
    """out[n] = sum of w[hperm[k]] over the head segment k in [hptr[n], hptr[n+1]) (iddgcn_head_wsum_f32)."""
    n_nodes, R = out.shape
    _req(out, _F32, (n_nodes, R), "out")
    _req(w, _F32, None, "w")
    if hptr.numel() != n_nodes + 1:
        raise L.IddgcnError("head_wsum: hptr must have n + 1 entries")
    L.check(L.lib().iddgcn_head_wsum_f32(_stream(), n_nodes, R, _ptr(hptr), _ptr(hperm), _ptr(w), _ptr(out)),
            "head_wsum")


def gather_rows(src, idx, dst):
    """dst[e] = src[idx[e]] for narrow rows (src: (N, w), idx: (M,) int32, dst: (M, w))."""
    M, w = dst.shape
    _req(src, _F32, None, "src")
    _req(idx, _I32, (M,), "idx")
    _req(dst, _F32, (M, w), "dst")
    if src.dim() != 2 or src.shape[1] != w:
        raise L.IddgcnError("gather_rows: width mismatch")
    L.check(L.lib().iddgcn_gather_rows_f32(_stream(), M, w, _ptr(src), _ptr(idx), _ptr(dst)), "gather_rows")


def reduce_slabs(slab, n_slabs, out, accumulate=False, scale=1.0):
    n = out.numel()
    L.check(L.lib().iddgcn_reduce_slabs_f32(_stream(), n_slabs, n, _ptr(slab), _ptr(out), int(accumulate),
                                            float(scale)), "reduce_slabs")


def adam(var, m, v, g, alpha, b1, b2, eps, sparse_form):
    n = var.numel()
    _same_size(n, "adam", m=m, v=v, g=g)
    L.check(L.lib().iddgcn_adam_f32(_stream(), n, _ptr(var), _ptr(m), _ptr(v), _ptr(g), float(alpha), float(b1),
                                    float(b2), float(eps), int(sparse_form)), "adam")


def adam_table(var, m, v, g, alpha_table, step, b1, b2, eps, sparse_form):
    """iddgcn_adam_f32 with alpha = alpha_table[step[0]] read on the device (graph-replayable)."""
    n = var.numel()
    _same_size(n, "adam", m=m, v=v, g=g)
    _req(alpha_table, _F32, None, "alpha_table")
    _req(step, _I32, (1,), "step")
    L.check(L.lib().iddgcn_adam_table_f32(_stream(), n, _ptr(var), _ptr(m), _ptr(v), _ptr(g), _ptr(alpha_table),
                                          _ptr(step), float(b1), float(b2), float(eps), int(sparse_form)),
            "adam_table")


def step_advance(step, loss_history=None, loss=None):
    """loss_history[step] = loss; step += 1 (one device thread)."""
    _req(step, _I32, (1,), "step")
    L.check(L.lib().iddgcn_step_advance(_stream(), _ptr(step), _ptr(loss_history), _ptr(loss)), "step_advance")


# -- device graph build (include/iddgcn_graph.h) ------------------------------------------------
def _workspace(nbytes, device):
    if nbytes < 0:
        raise L.IddgcnError("graph build: sizes out of range")
    return torch.empty(max(int(nbytes), 1), dtype=_U8, device=device)


def radix_sort(keys, vals=None, *, end_bit=None, argsort=False):
    """Stable LSD radix sort of int32/int64 keys (non-negative; bits [0, end_bit)).  Returns
    (sorted keys, sorted vals) where vals is `vals` permuted, the stable argsort if argsort=True,
    or None."""
    if keys.dtype not in (_I32, _I64):
        raise L.IddgcnError("radix_sort: keys must be int32 or int64")
    _req(keys, keys.dtype, None, "keys")
    _req(vals, _I32, (keys.shape[0],), "vals")
    kb = keys.element_size()
    n = keys.shape[0]
    end_bit = 8 * kb if end_bit is None else int(end_bit)
    ko = torch.empty_like(keys)
    vo = torch.empty(n, dtype=_I32, device=keys.device) if (vals is not None or argsort) else None
    ws = _workspace(L.lib().iddgcn_radix_sort_workspace(n, kb), keys.device)
    L.check(L.lib().iddgcn_radix_sort_pairs(_stream(), n, kb, end_bit, _ptr(keys), _ptr(vals), _ptr(ko), _ptr(vo),
                                            _ptr(ws), ws.numel()), "radix_sort")
    return ko, vo


def build_adjacency(triples, N, R):
    """utils1.get_adj_mats + DeviceAdjacency's CSR layouts on the GPU.  triples: (M, 3) int64 GPU
    tensor.  Returns a dict of GPU tensors (capacity M + R) and the host counts
    (nnz, placeholders, error)."""
    _triples3(triples, "triples")
    M = triples.shape[0]
    dev = triples.device
    need = L.lib().iddgcn_adjacency_workspace(M, N, R)
    ws = _workspace(need, dev)
    C = M + R
    out = {"fwd_ptr": torch.empty(R * (N + 1), dtype=_I32, device=dev),
           "fwd_col": torch.empty(C, dtype=_I32, device=dev), "fwd_val": torch.empty(C, dtype=_F32, device=dev),
           "bwd_ptr": torch.empty(N + 1, dtype=_I32, device=dev),
           "bwd_col": torch.empty(C, dtype=_I32, device=dev), "bwd_src": torch.empty(C, dtype=_I32, device=dev),
           "bwd_val": torch.empty(C, dtype=_F32, device=dev)}
    counts = torch.empty(3, dtype=_I32, device=dev)
    o = out
    L.check(L.lib().iddgcn_build_adjacency(_stream(), M, N, R, _ptr(triples), _ptr(o["fwd_ptr"]), _ptr(o["fwd_col"]),
                                           _ptr(o["fwd_val"]), _ptr(o["bwd_ptr"]), _ptr(o["bwd_col"]),
                                           _ptr(o["bwd_src"]), _ptr(o["bwd_val"]), _ptr(counts), _ptr(ws),
                                           ws.numel()), "build_adjacency")
    nnz, nph, err = (int(x) for x in counts.cpu())     # the one host synchronisation of the build
    return out, nnz, nph, err


def build_scored_edges(triples, labels, N, R):
    """graph.ScoredEdges on the GPU: tail-sorted (stable) h/r/t, gathered labels, tptr, hperm, hptr,
    inv.  Returns (dict of GPU tensors, error flag)."""
    _triples3(triples, "triples")
    T = triples.shape[0]
    dev = triples.device
    _req(labels, _F32, (T,), "labels")
    ws = _workspace(L.lib().iddgcn_scored_edges_workspace(T, N), dev)
    o = {k: torch.empty(T, dtype=_I32, device=dev) for k in ("h", "r", "t", "hperm")}
    o["y"] = torch.empty(T, dtype=_F32, device=dev) if labels is not None else None
    o["tptr"] = torch.empty(N + 1, dtype=_I32, device=dev)
    o["hptr"] = torch.empty(N + 1, dtype=_I32, device=dev)
    o["inv"] = torch.empty(T, dtype=_I64, device=dev)
    err = torch.empty(1, dtype=_I32, device=dev)
    L.check(L.lib().iddgcn_build_scored_edges(_stream(), T, N, R, _ptr(triples), _ptr(labels), _ptr(o["h"]),
                                              _ptr(o["r"]), _ptr(o["t"]), _ptr(o["y"]), _ptr(o["tptr"]),
                                              _ptr(o["hperm"]), _ptr(o["hptr"]), _ptr(o["inv"]), _ptr(err), _ptr(ws),
                                              ws.numel()), "build_scored_edges")
    return o, int(err.item())


# -- similarity graph (include/iddgcn_similarity.h) ---------------------------------------------
def similarity_pairs(X, threshold, capacity=None, band_capacity=None):
    """Keys i*N + j (unordered, int64 GPU tensor) of every i < j with cosine(X_i, X_j) > threshold.
    X: (N, F) float64 GPU tensor.  Reruns once with exact buffer sizes if a capacity was short."""
    _req(X, _F64, None, "X")
    if X.dim() != 2:
        raise L.IddgcnError("X must be (N, F)")
    N, F = X.shape
    dev = X.device
    ws = _workspace(L.lib().iddgcn_similarity_workspace(N, F), dev)
    cap = int(capacity) if capacity is not None else max(1 << 16, 64 * N)
    bcap = int(band_capacity) if band_capacity is not None else max(1 << 14, 4 * N)
    counts = torch.empty(2, dtype=_I64, device=dev)
    for _ in range(2):
        keys = torch.empty(max(cap, 1), dtype=_I64, device=dev)
        band = torch.empty(max(bcap, 1), dtype=_I64, device=dev)
        L.check(L.lib().iddgcn_similarity_pairs(_stream(), N, F, _ptr(X), float(threshold), _ptr(keys), cap,
                                                _ptr(band), bcap, _ptr(counts), _ptr(ws), ws.numel()),
                "similarity_pairs")
        n_acc, n_band = (int(v) for v in counts.cpu())
        if n_acc <= cap and n_band <= bcap:
            return keys[:n_acc]
        cap, bcap = max(cap, n_acc), max(bcap, n_band)
    raise L.IddgcnError("similarity_pairs: capacity retry failed")


def similarity_triples(sorted_keys, N, relation, start):
    _req(sorted_keys, _I64, None, "sorted_keys")
    n = sorted_keys.shape[0]
    out = torch.empty((n, 3), dtype=_I64, device=sorted_keys.device)
    L.check(L.lib().iddgcn_similarity_triples(_stream(), n, N, int(relation), int(start), _ptr(sorted_keys),
                                              _ptr(out)), "similarity_triples")
    return out


# -- negative sampling (include/iddgcn_sampling.h) -----------------------------------------------
def mt19937_words(seed, n, device):
    """The first n words of np.random.seed(seed)'s MT19937 stream (tempered uint32, as int32 bits)."""
    state = torch.empty(625, dtype=_I32, device=device)
    L.check(L.lib().iddgcn_mt19937_seed(_stream(), int(seed), _ptr(state)), "mt19937_seed")
    out = torch.empty(max(int(n), 1), dtype=_I32, device=device)
    L.check(L.lib().iddgcn_mt19937_generate(_stream(), _ptr(state), int(n), _ptr(out)), "mt19937_generate")
    return out[:int(n)]


def negative_samples(triples, num_entities, seed):
    """utils1.generate_negative_samples_np (utils1.py:646-655) on the GPU, bit-exact: triples (M, 3)
    int64 GPU tensor -> (M, 3) int64 negatives.  Host synchronisations: one per round of entity words
    (normally one)."""
    _triples3(triples, "triples")
    N = int(num_entities)
    if not 1 <= N <= 2 ** 31 - 1:
        raise L.IddgcnError("num_entities must be in [1, 2^31)")
    if not 0 <= int(seed) <= 2 ** 32 - 1:
        raise L.IddgcnError("seed must be between 0 and 2**32 - 1 (np.random.seed)")
    lib, dev, M = L.lib(), triples.device, triples.shape[0]
    out = torch.empty(M, 3, dtype=_I64, device=dev)
    if M == 0:
        return out
    state = torch.empty(625, dtype=_I32, device=dev)
    L.check(lib.iddgcn_mt19937_seed(_stream(), int(seed), _ptr(state)), "mt19937_seed")
    cond = torch.empty(M, dtype=_I32, device=dev)
    L.check(lib.iddgcn_mt19937_generate(_stream(), _ptr(state), M, _ptr(cond)), "mt19937_generate")
    ent = None
    if N > 1:
        rng = N - 1
        accept = (rng + 1) / (int(lib.iddgcn_randint_mask(rng)) + 1)       # > 1/2
        words = torch.empty(0, dtype=_I32, device=dev)
        ent = torch.empty(M, dtype=_I32, device=dev)
        need = M
        while True:
            more = int(need / accept * 1.01) + 4096
            new = torch.empty(more, dtype=_I32, device=dev)
            L.check(lib.iddgcn_mt19937_generate(_stream(), _ptr(state), more, _ptr(new)), "mt19937_generate")
            words = torch.cat([words, new]) if words.numel() else new
            nc = int(lib.iddgcn_accept_chunks(words.numel()))
            counts = torch.empty(nc, dtype=_I32, device=dev)
            offs = torch.empty(nc + 1, dtype=_I64, device=dev)
            L.check(lib.iddgcn_masked_accept(_stream(), _ptr(words), words.numel(), rng, M, _ptr(counts), _ptr(offs),
                                             _ptr(ent)), "masked_accept")
            got = int(offs[nc].item())
            if got >= M:
                break
            need = M - got
    L.check(lib.iddgcn_assemble_negatives(_stream(), M, _ptr(triples), _ptr(cond), _ptr(ent), _ptr(out)),
            "assemble_negatives")
    return out


PLANE_INV = 2.0 ** -15


def planes_to_f32(t):
    """Decode a pre-split planes table (include/iddgcn.h, IDDGCN_PLANES_*): rows of D = 256 in an
    fp32-shaped (rows, 256) tensor, 8 column blocks of [hi f16[32] | lo f16[32]], x = (hi + lo) * 2^-15."""
    h = t.contiguous().view(torch.float16).view(t.shape[0], t.shape[1] // 32, 2, 32)
    return ((h[:, :, 0].float() + h[:, :, 1].float()) * PLANE_INV).reshape(t.shape[0], t.shape[1])


# -- all-candidate ranking (include/iddgcn_screen.h) ---------------------------------------------
_SIDES = {"tail": L.SCREEN_TAIL, "head": L.SCREEN_HEAD, L.SCREEN_TAIL: L.SCREEN_TAIL, L.SCREEN_HEAD: L.SCREEN_HEAD}


def _side(side):
    if side not in _SIDES:
        raise L.IddgcnError(f"side must be 'tail' or 'head', got {side!r}")
    return _SIDES[side]


def screen_chain(q_node, q_rel, ES1, P, W, X3, S2, S3, rel, s, side="tail"):
    """s[q, c] = the pre-sigmoid DistMult logit of query q against every candidate c in [0, N): the three-layer
    tail chain and DistMult in one kernel (iddgcn_screen_chain_f32; D in {32, 64}, fp32 tables).  side "tail":
    (q_node[q], q_rel[q], c); "head": (c, q_rel[q], q_node[q]).  P: (3, R, N, D) and W: (3, N, R) views with
    contiguous rows (the engine's ws.P / ws.W), ES1, X3 (N, D), S2, S3 (D, D), rel (R, D), s (Q, N)."""
    Q, N = s.shape
    R, D = rel.shape
    _req(s, _F32, (Q, N), "s")
    _idx_ok(q_node, Q, N, "q_node")
    _idx_ok(q_rel, Q, R, "q_rel")
    for t, shape, nm in ((ES1, (N, D), "ES1"), (X3, (N, D), "X3"), (S2, (D, D), "S2"), (S3, (D, D), "S3"),
                         (rel, (R, D), "rel")):
        _req(t, _F32, shape, nm)
    ps0, ps1 = _req_rows(P, (3, R, N, D), "P")
    ws0, = _req_rows(W, (3, N, R), "W")
    if ps1 < N * D:
        raise L.IddgcnError("screen_chain: the relations of P overlap")
    # rows of ES1 and P are read as 16-byte vectors
    if (ES1.data_ptr() | P.data_ptr()) & 15 or ps0 % 4 or ps1 % 4:
        raise L.IddgcnError("screen_chain: ES1 / P must be 16-byte aligned, P's layer and relation strides "
                            "multiples of 4 floats")
    L.check(L.lib().iddgcn_screen_chain_f32(_stream(), Q, N, D, R, _side(side), _ptr(q_node), _ptr(q_rel), _ptr(ES1),
                                            _ptr(P), ps0, ps1, _ptr(W), ws0, _ptr(X3),
                                            _ptr(S2), _ptr(S3), _ptr(rel), _ptr(s)), "screen_chain")


def rank_topk(s, target, k, fptr=None, fidx=None, greater=None, equal=None, topk_idx=None, topk_val=None):
    """Per-query selection over s (Q, N) (iddgcn_rank_topk_f32): greater / equal = the non-filtered candidates
    c != target[q] scoring above / exactly s[q, target[q]] (0 where target is -1), and the k best non-filtered
    candidates, descending by value, ties by ascending id, padded with -1 / -inf.  fptr (Q + 1), fidx: the
    filter as CSR, candidate ids ascending and unique per query; the target is exempt.  s is not modified.
    Returns (greater, equal, topk_idx, topk_val), allocated when not given."""
    if s.dim() != 2:
        raise L.IddgcnError("rank_topk: s must be (Q, N)")
    Q, N = s.shape
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX:
        raise L.IddgcnError(f"rank_topk: k must be in [1, {L.TOPK_MAX}]")
    dev = s.device
    _req(s, _F32, (Q, N), "s")
    _req(target, _I32, (Q,), "target")
    if CHECK_INDEX_RANGES and Q:
        lo, hi = int(target.min()), int(target.max())
        if lo < -1 or hi >= N:
            raise L.IddgcnError(f"target: index out of range [-1, {N}): min {lo}, max {hi}")
    if (fptr is None) != (fidx is None):
        raise L.IddgcnError("rank_topk: fptr and fidx go together")
    if fptr is not None:
        _req(fptr, _I32, (Q + 1,), "fptr")
        _req(fidx, _I32, None, "fidx")
        _ptr_ascends(fptr, fidx.numel(), "rank_topk: fptr")
        if fidx.numel() == 0:
            fptr = fidx = None
    greater = _out(greater, (Q,), _I32, dev, "greater")
    equal = _out(equal, (Q,), _I32, dev, "equal")
    topk_idx = _out(topk_idx, (Q, k), _I32, dev, "topk_idx")
    topk_val = _out(topk_val, (Q, k), _F32, dev, "topk_val")
    L.check(L.lib().iddgcn_rank_topk_f32(_stream(), Q, N, k, _ptr(s), _ptr(target), _ptr(fptr), _ptr(fidx),
                                         _ptr(greater), _ptr(equal), _ptr(topk_idx), _ptr(topk_val)), "rank_topk")
    return greater, equal, topk_idx, topk_val


# -- batched explaiNE (include/iddgcn_explain.h) ---------------------------------------------------
def explain_seeds(h, r, t, ES1, P, W, Ssm, X, K, S2, S3, Wa2, Wa3, rel, scale=1.0, G=None, p=None):
    """dAE rows of Q predictions (iddgcn_explain_seeds_f32; D in {32, 64}, fp32 tables): for query q = (h[q], r[q],
    t[q]) the tail chain is recomputed from the node tables and the backward of ``scale * p_q`` gives
    G[q, 0] = dAE[:, h[q]] and G[q, 1] = dAE[:, t[q]] ((R, D) each, the query's own contributions: at h == t the
    row's gradient is their sum) and p[q].  P (3, R, N, D), W, Ssm (3, N, R), X (3, N, D): the engine's ws.P / ws.W /
    ws.Ssm / ws.X; ES1 (N, D); K = (K1, K2, K3), (R, D, D) each; S2, S3 (D, D); Wa2, Wa3 (D, R); rel (R, D).
    Returns (G (Q, 2, R, D), p (Q,)), allocated when not given."""
    R, D = rel.shape
    N = ES1.shape[0]
    Q = h.shape[0]
    _idx_ok(h, Q, N, "h")
    _idx_ok(r, Q, R, "r")
    _idx_ok(t, Q, N, "t")
    if len(K) != 3:
        raise L.IddgcnError("explain_seeds: K must be (K1, K2, K3)")
    for x, shape, nm in ((ES1, (N, D), "ES1"), (S2, (D, D), "S2"), (S3, (D, D), "S3"), (Wa2, (D, R), "Wa2"),
                         (Wa3, (D, R), "Wa3"), (rel, (R, D), "rel"), (K[0], (R, D, D), "K1"), (K[1], (R, D, D), "K2"),
                         (K[2], (R, D, D), "K3")):
        if x is None:
            raise L.IddgcnError(f"explain_seeds: {nm} is required")
        _req(x, _F32, shape, nm)
    ps0, ps1 = _req_rows(P, (3, R, N, D), "P")
    ws0, = _req_rows(W, (3, N, R), "W")
    ss0, = _req_rows(Ssm, (3, N, R), "Ssm")
    xs0, = _req_rows(X, (3, N, D), "X")
    if ps1 < N * D:
        raise L.IddgcnError("explain_seeds: the relations of P overlap")
    if ws0 != ss0:
        raise L.IddgcnError("explain_seeds: W and Ssm must share their layer stride")
    G = _out(G, (Q, 2, R, D), _F32, ES1.device, "G")
    p = _out(p, (Q,), _F32, ES1.device, "p")
    if (ES1.data_ptr() | P.data_ptr() | G.data_ptr()) & 15 or ps0 % 4 or ps1 % 4:
        raise L.IddgcnError("explain_seeds: ES1 / P / G must be 16-byte aligned, P's layer and relation strides "
                            "multiples of 4 floats")
    L.check(L.lib().iddgcn_explain_seeds_f32(
        _stream(), Q, N, D, R, _ptr(h), _ptr(r), _ptr(t), float(scale), _ptr(ES1), _ptr(P), ps0, ps1,
        _ptr(W), _ptr(Ssm), ws0, _ptr(X), xs0, _ptr(K[0]), _ptr(K[1]), _ptr(K[2]), _ptr(S2), _ptr(S3),
        _ptr(Wa2), _ptr(Wa3), _ptr(rel), _ptr(G), _ptr(p)), "explain_seeds")
    return G, p


def explain_row_grads(h, t, row_ptr, col, G, E, qptr, entry, grad, entry_of_csr=None):
    """The ragged SDDMM of batched explaiNE (iddgcn_explain_row_grads_f32): query q's candidates — the stored entries
    of row h[q] of every relation, then (h[q] != t[q]) of row t[q] — written at qptr[q] + j: ``entry`` = the CSR
    position mapped through ``entry_of_csr`` (int64, e.g. DeviceAdjacency.fwd_src; None = the position), ``grad`` =
    <G[q, side, rel], E[col]>.  row_ptr (R (N + 1)), col: the batched forward CSR; qptr (Q + 1) int64 with
    qptr[q + 1] - qptr[q] the sum of the query's row degrees; entry int32 / grad fp32 of at least qptr[-1] elements."""
    Q, two, R, D = G.shape
    N = E.shape[0]
    _req(G, _F32, (Q, 2, R, D), "G")
    _req(E, _F32, (N, D), "E")
    _idx_ok(h, Q, N, "h")
    _idx_ok(t, Q, N, "t")
    _req(row_ptr, _I32, (R * (N + 1),), "row_ptr")
    _req(col, _I32, None, "col")
    _req(qptr, _I64, (Q + 1,), "qptr")
    _req(entry, _I32, None, "entry")
    _req(grad, _F32, None, "grad")
    if entry.dim() != 1 or grad.shape != entry.shape:
        raise L.IddgcnError("explain_row_grads: entry and grad must be 1-d and of one length")
    if entry_of_csr is not None:
        _req(entry_of_csr, _I64, (col.shape[0],), "entry_of_csr")
    if (E.data_ptr() | G.data_ptr()) & 15:
        raise L.IddgcnError("explain_row_grads: E / G must be 16-byte aligned")
    _ptr_ascends(qptr, entry.numel(), "explain_row_grads: qptr")
    L.check(L.lib().iddgcn_explain_row_grads_f32(
        _stream(), Q, N, D, R, _ptr(h), _ptr(t), _ptr(row_ptr), _ptr(col), _ptr(entry_of_csr), _ptr(G), _ptr(E),
        _ptr(qptr), _ptr(entry), _ptr(grad)), "explain_row_grads")


def explain_topk(qptr, entry, grad, k, topk_entry=None, topk_val=None, n_pos=None):
    """Per query the k best of its candidate segment [qptr[q], qptr[q + 1]) (iddgcn_explain_topk_f32): descending by
    value, ties by ascending entry id, padded with -1 / -inf; n_pos[q] = its candidates with value > 0.
    Returns (topk_entry (Q, k) int32, topk_val (Q, k), n_pos (Q,) int32), allocated when not given."""
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX:
        raise L.IddgcnError(f"explain_topk: k must be in [1, {L.TOPK_MAX}]")
    _req(qptr, _I64, None, "qptr")
    if qptr.dim() != 1 or qptr.shape[0] < 1:
        raise L.IddgcnError("explain_topk: qptr must be (Q + 1,)")
    Q = qptr.shape[0] - 1
    _req(entry, _I32, None, "entry")
    _req(grad, _F32, None, "grad")
    if entry.dim() != 1 or grad.shape != entry.shape:
        raise L.IddgcnError("explain_topk: entry and grad must be 1-d and of one length")
    _ptr_ascends(qptr, entry.numel(), "explain_topk: qptr")
    dev = qptr.device
    topk_entry = _out(topk_entry, (Q, k), _I32, dev, "topk_entry")
    topk_val = _out(topk_val, (Q, k), _F32, dev, "topk_val")
    n_pos = _out(n_pos, (Q,), _I32, dev, "n_pos")
    L.check(L.lib().iddgcn_explain_topk_f32(_stream(), Q, k, _ptr(qptr), _ptr(entry), _ptr(grad), _ptr(topk_entry),
                                            _ptr(topk_val), _ptr(n_pos)), "explain_topk")
    return topk_entry, topk_val, n_pos


# -- batched mask explainers (include/iddgcn_explain.h) -------------------------------------------
def mask_explain(E, K, S, Wa, ba, rel, h, r, t, qptr, entry, crel, ccol, crole, init_e, m, v, steps, alpha, out,
                 qids, level_ptr, num_epochs, epochs_base=0, b1=0.9, b2=0.999, eps=1e-7, target_ratios=None):
    """Every epoch of the mask training of Q triples (iddgcn_mask_explain_f32), one launch per level: launch i runs
    the queries qids[level_ptr[i]:level_ptr[i + 1]], one workgroup each; two queries of a level must share no entry,
    and queries that share one must sit in ascending levels in input order (explain.mask_schedule) — stream order is
    the only synchronisation.  E (N, D); K, S, Wa, ba: the three layers' (R, D, D), (D, D), (D, R), (R,); rel (R, D);
    h, r, t (Q,) int32; qptr (Q + 1,) int64 and entry / crel / ccol / crole (qptr[-1],) int32: explain.mask_candidates'
    lists; init_e, m, v (fp32), steps (int32): one value per stored entry of the full adjacency, m / v / steps
    updated in place; alpha: one fp32 per global step, read at epochs_base + q * num_epochs + epoch; out (qptr[-1],)
    receives the final masked values; target_ratios (R,) fp32 or None; level_ptr: a host sequence.
    D in {32, 64}, 1 <= R <= 8.  Index values are the caller's to validate (IDDGCN_CHECK_INDICES=1 checks them here)."""
    N, D = E.shape
    R = rel.shape[0]
    num_epochs, epochs_base = int(num_epochs), int(epochs_base)
    if num_epochs < 0 or epochs_base < 0:
        raise L.IddgcnError("mask_explain: num_epochs and epochs_base must be non-negative")
    _req(E, _F32, (N, D), "E")
    _req(rel, _F32, (R, D), "rel")
    _req_layers(K, S, Wa, ba, R, D, "mask_explain")
    Q, C = _req_queries(h, r, t, qptr, crel, ccol, crole, N, R)
    total = m.shape[0]
    _idx_ok(entry, C, total, "entry")
    _req(init_e, _F32, (total,), "init_e")
    _req(m, _F32, (total,), "m")
    _req(v, _F32, (total,), "v")
    _req(steps, _I32, (total,), "steps")
    _req(out, _F32, (C,), "out")
    _req(alpha, _F32, None, "alpha")
    if alpha.dim() != 1 or alpha.shape[0] < epochs_base + Q * num_epochs:
        raise L.IddgcnError("mask_explain: alpha needs one entry per global step (epochs_base + Q * num_epochs)")
    if target_ratios is not None:
        _req(target_ratios, _F32, (R,), "target_ratios")
    nq = qids.shape[0]
    _idx_ok(qids, nq, Q, "qids")
    lp = [int(x) for x in level_ptr]
    if not lp or lp[0] < 0 or lp[-1] > nq or any(b < a for a, b in zip(lp, lp[1:])):
        raise L.IddgcnError("mask_explain: level_ptr must ascend within [0, len(qids)]")
    if E.data_ptr() & 15:
        raise L.IddgcnError("mask_explain: E must be 16-byte aligned")
    _ptr_ascends(qptr, C, "mask_explain: qptr", exact=True)
    a = L.MaskExplainArgs()
    a.N, a.d, a.R, a.num_epochs, a.epochs_base = N, D, R, num_epochs, epochs_base
    a.b1, a.b2, a.eps = float(b1), float(b2), float(eps)
    # the backward reads K^l_r^T and S^l^T along rows: transposed copies, made once per call
    KT = [x.transpose(1, 2).contiguous() for x in K]
    ST = [x.t().contiguous() for x in S]
    _set_ptrs(a, h=h, r=r, t=t, qptr=qptr, entry=entry, crel=crel, ccol=ccol, crole=crole, E=E, rel=rel, K=K, KT=KT,
              S=S, ST=ST, Wa=Wa, ba=ba, init_e=init_e, m=m, v=v, steps=steps, alpha=alpha, target_ratios=target_ratios,
              out=out)
    fn, st = L.lib().iddgcn_mask_explain_f32, _stream()
    for lo, hi in zip(lp, lp[1:]):
        if hi == lo:
            continue
        a.qids = qids.data_ptr() + 4 * lo
        a.n_queries = hi - lo
        L.check(fn(st, ctypes.byref(a)), "mask_explain")
    return out


def explain_curves(E, K, S, Wa, ba, rel, h, r, t, qptr, crel, ccol, crole, cstep, cval, k, deletion=None,
                   insertion=None):
    """Deletion and insertion curves of Q explanations (iddgcn_explain_curves_f32), one launch: per query 2 (k + 1)
    edited forwards.  E (N, D); K, S, Wa, ba: the three layers' (R, D, D), (D, D), (D, R), (R,); rel (R, D); h, r, t
    (Q,) int32; qptr (Q + 1,) int64 into the candidate arrays crel / ccol / crole / cstep (int32) and cval (fp32):
    explain.curve_steps' lists (a slice of qptr keeps its absolute offsets).  Returns (deletion, insertion), (Q, k + 1)
    fp32 each, allocated when not given.  D in {32, 64}, 1 <= R <= 8, 1 <= k <= TOPK_MAX.  Index values are the
    caller's to validate (IDDGCN_CHECK_INDICES=1 checks them here)."""
    N, D = E.shape
    R = rel.shape[0]
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX:
        raise L.IddgcnError(f"explain_curves: k must be in [1, {L.TOPK_MAX}]")
    _req(E, _F32, (N, D), "E")
    _req(rel, _F32, (R, D), "rel")
    _req_layers(K, S, Wa, ba, R, D, "explain_curves")
    Q, C = _req_queries(h, r, t, qptr, crel, ccol, crole, N, R)
    _req(cstep, _I32, (C,), "cstep")
    _req(cval, _F32, (C,), "cval")
    dev = E.device
    deletion = _out(deletion, (Q, k + 1), _F32, dev, "deletion")
    insertion = _out(insertion, (Q, k + 1), _F32, dev, "insertion")
    if E.data_ptr() & 15:
        raise L.IddgcnError("explain_curves: E must be 16-byte aligned")
    _ptr_ascends(qptr, C, "explain_curves: qptr")
    if CHECK_INDEX_RANGES and Q and C and (int(cstep.min()) < -1 or int(cstep.max()) >= k):
        raise L.IddgcnError("explain_curves: cstep must lie in [-1, k)")
    a = L.ExplainCurvesArgs()
    a.N, a.d, a.R, a.k, a.Q = N, D, R, k, Q
    _set_ptrs(a, h=h, r=r, t=t, qptr=qptr, crel=crel, ccol=ccol, crole=crole, cstep=cstep, cval=cval, E=E, rel=rel,
              K=K, S=S, Wa=Wa, ba=ba, del_=deletion, ins=insertion)
    L.check(L.lib().iddgcn_explain_curves_f32(_stream(), ctypes.byref(a)), "explain_curves")
    return deletion, insertion


CF_MODES = {"flip": L.CF_FLIP, "lower": L.CF_LOWER, "raise": L.CF_RAISE}


def explain_counterfactual(E, K, S, Wa, ba, rel, h, r, t, qptr, crel, ccol, crole, cpartner, celig, cval, k,
                           toward="flip", threshold=0.5, max_cand=None, path=None, chosen=None, cstep=None,
                           n_steps=None, flipped=None, loo=None, scratch=None):
    """The greedy counterfactual search of Q queries and their occlusion tables (iddgcn_explain_counterfactual_f32):
    2 max(k, 1) launches, no host read in between.  The weights, h, r, t, qptr, crel, ccol, crole and cval as in
    explain_curves; cpartner (int32, the segment-relative index of the candidate removed together with this one, -1:
    none) and celig (int32, 0: never removed, never evaluated): explain.counterfactual_candidates' lists (a slice of
    qptr keeps its absolute offsets).  ``toward``: "flip", "lower" or "raise"; ``max_cand``: the longest segment
    (sizes the grid; None: the candidate count).  Returns a dict: ``path`` (Q, k + 1) fp32, ``chosen`` (Q, k) int32,
    ``n_steps`` and ``flipped`` (Q,) int32, ``cstep`` (int32) and ``loo`` (fp32) per candidate — allocated when not
    given; ``scratch`` (fp32 per candidate) holds the later steps' values.  D in {32, 64}, 1 <= R <= 8,
    0 <= k <= TOPK_MAX.  Index values are the caller's to validate (IDDGCN_CHECK_INDICES=1 checks them here)."""
    N, D = E.shape
    R = rel.shape[0]
    k = int(k)
    if not 0 <= k <= L.TOPK_MAX:
        raise L.IddgcnError(f"explain_counterfactual: k must be in [0, {L.TOPK_MAX}]")
    if toward not in CF_MODES:
        raise L.IddgcnError(f"explain_counterfactual: toward must be 'flip', 'lower' or 'raise', got {toward!r}")
    _req(E, _F32, (N, D), "E")
    _req(rel, _F32, (R, D), "rel")
    _req_layers(K, S, Wa, ba, R, D, "explain_counterfactual")
    Q, C = _req_queries(h, r, t, qptr, crel, ccol, crole, N, R)
    _req(cpartner, _I32, (C,), "cpartner")
    _req(celig, _I32, (C,), "celig")
    _req(cval, _F32, (C,), "cval")
    dev = E.device
    out = dict(path=_out(path, (Q, k + 1), _F32, dev, "path"), chosen=_out(chosen, (Q, k), _I32, dev, "chosen"),
               cstep=_out(cstep, (C,), _I32, dev, "cstep"), n_steps=_out(n_steps, (Q,), _I32, dev, "n_steps"),
               flipped=_out(flipped, (Q,), _I32, dev, "flipped"), loo=_out(loo, (C,), _F32, dev, "loo"))
    scratch = _out(scratch, (C,), _F32, dev, "scratch")
    if E.data_ptr() & 15:
        raise L.IddgcnError("explain_counterfactual: E must be 16-byte aligned")
    _ptr_ascends(qptr, C, "explain_counterfactual: qptr")
    if CHECK_INDEX_RANGES and Q and C:
        qp = qptr.cpu()
        lens = qp[1:] - qp[:-1]
        seg = torch.repeat_interleave(lens, lens).to(dev)                     # each candidate's segment length
        part = cpartner[int(qp[0]):int(qp[-1])]
        if seg.numel() != part.numel() or bool(((part < -1) | (part >= seg)).any()):
            raise L.IddgcnError("explain_counterfactual: cpartner must lie in [-1, the segment's length)")
    a = L.CounterfactualArgs()
    a.N, a.d, a.R, a.k, a.Q, a.mode, a.threshold = N, D, R, k, Q, CF_MODES[toward], float(threshold)
    a.max_cand = C if max_cand is None else int(max_cand)
    if a.max_cand < 0:
        raise L.IddgcnError("explain_counterfactual: max_cand must not be negative")
    _set_ptrs(a, h=h, r=r, t=t, qptr=qptr, crel=crel, ccol=ccol, crole=crole, cpartner=cpartner, celig=celig,
              cval=cval, E=E, rel=rel, K=K, S=S, Wa=Wa, ba=ba, scratch=scratch, **out)
    L.check(L.lib().iddgcn_explain_counterfactual_f32(_stream(), ctypes.byref(a)), "explain_counterfactual")
    return out


def explain_path(E, K, S, Wa, ba, rel, h, r, t, qptr, crel, ccol, crole, celig, cval, alpha, omega, attr=None,
                 total=None, p_full=None, p_base=None, gap=None, scratch=None):
    """Integrated-gradients attributions of Q queries along the path that scales their eligible candidates' values
    from 0 to the stored ones (iddgcn_explain_path_f32), two launches.  The weights, h, r, t, qptr, crel, ccol, crole,
    celig and cval as in explain_counterfactual (a slice of qptr keeps its absolute offsets); alpha, omega (m,) fp32:
    the quadrature rule's nodes and weights, 1 <= m <= PATH_MAX_STEPS.  Returns a dict: ``attr`` fp32 per candidate
    (exactly 0 where not eligible), ``total``, ``p_full``, ``p_base`` and ``gap`` = total - (p_full - p_base), (Q,)
    fp32 each — allocated when not given; ``scratch``: fp32, at least iddgcn_explain_path_scratch_floats(Q, m, D, R)
    long.  D in {32, 64}, 1 <= R <= 8.  Index values are the caller's to validate (IDDGCN_CHECK_INDICES=1 checks them
    here)."""
    N, D = E.shape
    R = rel.shape[0]
    _req(E, _F32, (N, D), "E")
    _req(rel, _F32, (R, D), "rel")
    _req_layers(K, S, Wa, ba, R, D, "explain_path")
    Q, C = _req_queries(h, r, t, qptr, crel, ccol, crole, N, R)
    _req(celig, _I32, (C,), "celig")
    _req(cval, _F32, (C,), "cval")
    _req(alpha, _F32, None, "alpha")
    m = alpha.shape[0] if alpha.dim() == 1 else -1
    _req(omega, _F32, (m,), "omega")
    if not 1 <= m <= L.PATH_MAX_STEPS:
        raise L.IddgcnError(f"explain_path: alpha and omega must be (m,) with m in [1, {L.PATH_MAX_STEPS}]")
    dev = E.device
    out = dict(attr=_out(attr, (C,), _F32, dev, "attr"), total=_out(total, (Q,), _F32, dev, "total"),
               p_full=_out(p_full, (Q,), _F32, dev, "p_full"), p_base=_out(p_base, (Q,), _F32, dev, "p_base"),
               gap=_out(gap, (Q,), _F32, dev, "gap"))
    need = int(L.lib().iddgcn_explain_path_scratch_floats(Q, m, D, R))
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=_F32, device=dev)
    _req(scratch, _F32, None, "scratch")
    if scratch.numel() < need:
        raise L.IddgcnError(f"explain_path: scratch holds {scratch.numel()} floats, {need} are needed")
    if E.data_ptr() & 15:
        raise L.IddgcnError("explain_path: E must be 16-byte aligned")
    _ptr_ascends(qptr, C, "explain_path: qptr")
    a = L.ExplainPathArgs()
    a.N, a.d, a.R, a.Q, a.m = N, D, R, Q, m
    # the backward reads K^l_r^T and S^l^T along rows: transposed copies, made once per call
    KT = [x.transpose(1, 2).contiguous() for x in K]
    ST = [x.t().contiguous() for x in S]
    _set_ptrs(a, h=h, r=r, t=t, qptr=qptr, crel=crel, ccol=ccol, crole=crole, celig=celig, cval=cval, E=E, rel=rel,
              K=K, KT=KT, S=S, ST=ST, Wa=Wa, ba=ba, alpha=alpha, omega=omega, scratch=scratch, **out)
    L.check(L.lib().iddgcn_explain_path_f32(_stream(), ctypes.byref(a)), "explain_path")
    return out


# -- explanation ground truth (include/iddgcn_ground_truth.h) ------------------------------------
def gt_sim_lists(sim, N):
    """Similarity lists of every node as a CSR (ptr [N+1], val [2n], first [2n]) and the device error flag (not
    read here).  sim: (n, 3) int64 GPU tensor."""
    _triples3(sim, "sim")
    n, dev = sim.shape[0], sim.device
    need = ctypes.c_longlong(0)
    L.check(L.lib().iddgcn_gt_sim_lists_workspace(n, ctypes.byref(need)), "gt_sim_lists_workspace")
    ws = _workspace(need.value, dev)
    ptr = torch.empty(N + 1, dtype=_I32, device=dev)
    val = torch.empty(max(2 * n, 1), dtype=_I32, device=dev)
    first = torch.empty(max(2 * n, 1), dtype=_U8, device=dev)
    err = torch.empty(1, dtype=_I32, device=dev)
    L.check(L.lib().iddgcn_gt_sim_lists(_stream(), n, N, _ptr(sim), _ptr(ptr), _ptr(val), _ptr(first), _ptr(err),
                                        _ptr(ws), ws.numel()), "gt_sim_lists")
    return ptr, val, first, err


def gt_dc_table(dc, N, R):
    """dc as a CSR over (rel, drug) of the sorted mutations (seg_ptr [R*N+1], seg_mu [M]) and the device error
    flag (not read here).  dc: (M, 3) int64 GPU tensor."""
    _triples3(dc, "dc")
    M, dev = dc.shape[0], dc.device
    need = ctypes.c_longlong(0)
    L.check(L.lib().iddgcn_gt_dc_table_workspace(M, N, R, ctypes.byref(need)), "gt_dc_table_workspace")
    ws = _workspace(need.value, dev)
    seg_ptr = torch.empty(R * N + 1, dtype=_I32, device=dev)
    seg_mu = torch.empty(max(M, 1), dtype=_I32, device=dev)
    err = torch.empty(1, dtype=_I32, device=dev)
    L.check(L.lib().iddgcn_gt_dc_table(_stream(), M, N, R, _ptr(dc), _ptr(seg_ptr), _ptr(seg_mu), _ptr(err), _ptr(ws),
                                       ws.numel()), "gt_dc_table")
    return seg_ptr, seg_mu, err


def _gt_tables(mu, drug, dc, N, R):
    (mp, mv, mf), (dp, dv, df), (sp, sm) = mu, drug, dc
    for p, v, f, nm in ((mp, mv, mf, "mu"), (dp, dv, df, "drug")):
        _req(p, _I32, (N + 1,), nm + " ptr")
        _req(v, _I32, None, nm + " val")
        _req(f, _U8, (v.shape[0],), nm + " first")
    _req(sp, _I32, (R * N + 1,), "seg_ptr")
    _req(sm, _I32, None, "seg_mu")
    return [_ptr(x) for x in (mp, mv, mf, dp, dv, df, sp, sm)]


def ground_truth_count(queries, mu, drug, dc, N, R):
    """COUNT pass: (len [Q] int64, err [1] int32), both on the device.  The queries' ids must be in range (the
    caller checks: ground_truth.construct_ground_truth)."""
    _triples3(queries, "queries")
    Q, dev = queries.shape[0], queries.device
    length = torch.empty(max(Q, 1), dtype=_I64, device=dev)
    err = torch.zeros(1, dtype=_I32, device=dev)
    L.check(L.lib().iddgcn_ground_truth_count(_stream(), Q, N, R, _ptr(queries), *_gt_tables(mu, drug, dc, N, R),
                                              _ptr(length), _ptr(err)), "ground_truth_count")
    return length[:Q], err


def gt_exclusive_scan(length):
    _req(length, _I64, None, "len")
    Q = length.shape[0]
    ptr = torch.empty(Q + 1, dtype=_I64, device=length.device)
    L.check(L.lib().iddgcn_gt_exclusive_scan(_stream(), Q, _ptr(length) if Q else None, _ptr(ptr)),
            "gt_exclusive_scan")
    return ptr


def ground_truth_fill(queries, mu, drug, dc, N, R, ptr, total, drug_rel, mu_rel):
    """FILL pass: the (total, 3) int64 triples, query q's at rows ptr[q] .. ptr[q+1]."""
    _triples3(queries, "queries")
    Q = queries.shape[0]
    _req(ptr, _I64, (Q + 1,), "ptr")
    out = torch.empty((max(int(total), 1), 3), dtype=_I64, device=queries.device)
    L.check(L.lib().iddgcn_ground_truth_fill(_stream(), Q, N, R, _ptr(queries), *_gt_tables(mu, drug, dc, N, R),
                                             _ptr(ptr), int(drug_rel), int(mu_rel), _ptr(out)), "ground_truth_fill")
    return out[:int(total)]


# -- classification metrics on the device (include/iddgcn_metrics.h) -----------------------------
def clf_metrics_workspace(n, G, device):
    """The workspace tensor iddgcn_clf_metrics needs for n elements and G groups (one byte at the least)."""
    nbytes = L.lib().iddgcn_clf_metrics_workspace(int(n), int(G))
    if nbytes < 0:
        raise L.IddgcnError(f"clf_metrics: n must be in [0, 2^31) and G in [0, {L.CLF_MAX_GROUPS}], got n={n}, G={G}")
    return torch.empty(max(int(nbytes), 1), dtype=_U8, device=device)


def clf_metrics(prob, label, group=None, G=0, threshold=0.5, counts=None, values=None, workspace=None):
    """iddgcn_clf_metrics: ``counts`` (1 + G, 9) int64 in the order of L.CLF_COUNTS and ``values`` (1 + G, 8) float64
    in the order of L.CLF_VALUES, of float32 probabilities / labels and int32 group ids (slot 0: every element,
    slot g + 1: group g).  Outputs and workspace are allocated unless given (a captured graph passes its own)."""
    _req(prob, _F32, None, "prob")
    n = prob.numel()
    if n < 1:
        raise L.IddgcnError("clf_metrics: no elements")
    _req(label, _F32, None, "label")
    if label.numel() != n:
        raise L.IddgcnError("clf_metrics: prob and label must be of one length")
    G = int(G)
    if G > 0:
        if group is None:
            raise L.IddgcnError("clf_metrics: G > 0 needs group ids")
        _req(group, _I32, None, "group")
        if group.numel() != n:
            raise L.IddgcnError("clf_metrics: prob and group must be of one length")
    if counts is None:
        counts = torch.empty((1 + G, len(L.CLF_COUNTS)), dtype=_I64, device=prob.device)
    if values is None:
        values = torch.empty((1 + G, len(L.CLF_VALUES)), dtype=_F64, device=prob.device)
    _req(counts, _I64, (1 + G, len(L.CLF_COUNTS)), "counts")
    _req(values, _F64, (1 + G, len(L.CLF_VALUES)), "values")
    if workspace is None:
        workspace = clf_metrics_workspace(n, G, prob.device)
    _req(workspace, _U8, None, "workspace")
    L.check(L.lib().iddgcn_clf_metrics(_stream(), n, G, _ptr(prob), _ptr(label), _ptr(group) if G > 0 else None,
                                       float(threshold), _ptr(counts), _ptr(values), _ptr(workspace),
                                       workspace.numel()), "clf_metrics")
    return counts, values


def keep_best(params, best, value, mode, best_value, best_epoch, epoch, improved):
    """iddgcn_keep_best_f32: best <- params if the device double ``value`` strictly improves on ``best_value``
    (mode 0: larger, 1: smaller; anything but a NaN improves while best_epoch < 0)."""
    _req(params, _F32, None, "params")
    _req(best, _F32, tuple(params.shape), "best")
    for t, nm in ((value, "value"), (best_value, "best_value")):
        _req(t, _F64, (1,), nm)
    for t, nm in ((best_epoch, "best_epoch"), (epoch, "epoch"), (improved, "improved")):
        _req(t, _I32, (1,), nm)
    L.check(L.lib().iddgcn_keep_best_f32(_stream(), params.numel(), _ptr(params), _ptr(best), _ptr(value), int(mode),
                                         _ptr(best_value), _ptr(best_epoch), _ptr(epoch), _ptr(improved)),
            "keep_best")


def clf_history_append(counts, values, hist_counts, hist_values, counter):
    """hist_*[counter] = counts / values; counter += 1 (nothing once the history is full)."""
    _req(counts, _I64, None, "counts")
    _req(values, _F64, None, "values")
    cap = hist_counts.shape[0]
    _req(hist_counts, _I64, (cap, counts.numel()), "hist_counts")
    _req(hist_values, _F64, (cap, values.numel()), "hist_values")
    _req(counter, _I32, (1,), "counter")
    L.check(L.lib().iddgcn_clf_history_append(_stream(), counts.numel(), values.numel(), _ptr(counts), _ptr(values),
                                              _ptr(hist_counts), _ptr(hist_values), cap, _ptr(counter)),
            "clf_history_append")
