"""Record tests/golden/dispatch/*.txt: the host-side dispatch of libiddgcn_hip.so (which kernel a row GEMM takes, what
every launching entry point refuses and in which order, the exported launch-geometry functions).

Nothing here launches a kernel or needs a GPU.  The goldens pin a refactor of the C-ABI layer to the library it
started from, so they are recorded against THAT library, built in a separate checkout:

    IDDGCN_LIB=/path/to/parent/iddgcn_amd/libiddgcn_hip.so python tools/record_dispatch_golden.py

tests/test_dispatch_host.py recomputes the same tables from the tree's library with the functions below and compares.
"""
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "dispatch")

# ---- iddgcn_rowgemm_kernel_id over the full product, in this order (the last axis varies fastest) ----
ID_AXES = (("D", (32, 64, 128, 256)), ("precision", (0, 1, 2, 3, 4)), ("R", (0, 1, 2, 3, 8)),
           ("v_row_stride", (0, 64, 256)), ("v_idx", (0, 1)), ("coef_idx", (0, 1)), ("a_idx", (0, 1)),
           ("act", (0, 1, 2)), ("accumulate", (0, 1)), ("planes", (0, 1, 2, 4)), ("b_trans", (0, 1)))
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"

# ---- refusals: every launching entry over D x R x precision, in this order ----
REF_D = (16, 32, 64, 128, 256)
REF_R = (-1, 0, 1, 2, 8, 9)
REF_P = (0, 1, 2, 3, 4, 5)
RC_CHAR = {0: "0", -1: "D", -2: "R", -3: "A"}      # ok, IDDGCN_E_BAD_DIM, _BAD_REL, _BAD_ARG

GEOM_ARGS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 10**6, 4 * 10**6,
             4 * 10**7, 2**31 - 1)


def id_cases():
    """The argument dicts of the kernel-id table, in the recorded order."""
    names = [n for n, _ in ID_AXES]
    for vals in itertools.product(*(v for _, v in ID_AXES)):
        yield dict(zip(names, vals))


def kernel_ids(lib):
    from iddgcn_amd import _lib
    fake = 16            # never dereferenced: iddgcn_rowgemm_kernel_id inspects the arguments only
    out = []
    for c in id_cases():
        a = _lib.RowGemmArgs(M=1000, D=c["D"], A=fake, a_idx=fake * c["a_idx"], B=fake, b_trans=c["b_trans"], C=fake,
                             accumulate=c["accumulate"], R=c["R"], coef=fake, coef_idx=fake * c["coef_idx"], V=fake,
                             v_idx=fake * c["v_idx"], v_rel_stride=4096, v_row_stride=c["v_row_stride"],
                             act=c["act"], aux=fake, planes=c["planes"], precision=c["precision"])
        out.append(lib.iddgcn_rowgemm_kernel_id(ctypes.byref(a)))
    return out


def encode_ids(ids):
    """(header line 'A=100 B=300 ...', one letter per case): letters in order of first appearance."""
    table = {}
    for i in ids:
        if i not in table:
            table[i] = LETTERS[len(table)]
    return " ".join(f"{c}={i}" for i, c in table.items()), "".join(table[i] for i in ids)


def decode_ids(text):
    """The ids of ids_text(): the letters of the case lines, a letter followed by a count standing for that many."""
    import re
    lines = text.split("\n")
    table = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in lines[0].split()}
    return [table[c] for c, n in re.findall(r"([A-Za-z])(\d*)", "".join(lines[1:])) for _ in range(int(n or 1))]


def refusal_entries():
    """name -> (how the call returns before a launch, call(lib, D, R, precision)).

    'zero': the size argument (M, T, n, n_nodes, n_seg) is 0 and the data pointers are stand-ins: the entry returns
    at its size check at the latest.  'null': the entry has no early return at size 0, so the data pointers are null
    and it returns IDDGCN_E_BAD_ARG at the latest.  Either way no call reaches the entry's first launch."""
    from iddgcn_amd import _lib
    buf = ctypes.create_string_buffer(96)
    q = (ctypes.addressof(buf) + 15) & ~15         # a 16-byte aligned stand-in (host memory, never dereferenced)
    N = None

    def rg(M, D, R, P, ptr):
        return _lib.RowGemmArgs(M=M, D=D, A=ptr, B=ptr, C=ptr, R=R, coef=ptr, V=ptr, v_row_stride=0, act=0, aux=ptr,
                                precision=P)

    tn0 = (_lib.TnArgs * 1)()
    e = {
        "iddgcn_spmm_csr_f32": ("zero", lambda L, D, R, P: L.iddgcn_spmm_csr_f32(N, 0, 4, D, q, q, q, q, q, 0)),
        "iddgcn_sddmm_csr_f32": ("zero", lambda L, D, R, P: L.iddgcn_sddmm_csr_f32(N, 0, 4, D, q, q, q, q, q)),
        "iddgcn_rowgemm_f32": ("zero", lambda L, D, R, P: L.iddgcn_rowgemm_f32(N, ctypes.byref(rg(0, D, R, P, q)))),
        "iddgcn_rowgemm_batched_f32": ("null", lambda L, D, R, P: L.iddgcn_rowgemm_batched_f32(
            N, ctypes.byref(rg(1, D, R, P, None)), 1)),
        "iddgcn_gemm_tn_f32": ("null", lambda L, D, R, P: L.iddgcn_gemm_tn_f32(N, 1, D, N, N, N, 1, N, 0, P)),
        "iddgcn_gemm_tn_batched_f32": ("zero", lambda L, D, R, P: L.iddgcn_gemm_tn_batched_f32(N, D, tn0, 0, q, 0, P)),
        "iddgcn_gemm_tn_planes_f32": ("null", lambda L, D, R, P: L.iddgcn_gemm_tn_planes_f32(N, 1, D, N, N, N, 1, N, 0)),
        "iddgcn_gemm_tn_narrow_f32": ("null", lambda L, D, R, P: L.iddgcn_gemm_tn_narrow_f32(
            N, 1, D, R, N, N, N, 1, N, N, 0)),
        "iddgcn_alpha_fwd_f32": ("zero", lambda L, D, R, P: L.iddgcn_alpha_fwd_f32(N, 0, D, R, q, N, q, q, q, q)),
        "iddgcn_combine_f32": ("zero", lambda L, D, R, P: L.iddgcn_combine_f32(N, 0, D, R, q, q, q, N, q, q, 4096, q)),
        "iddgcn_distmult_bce_f32": ("zero", lambda L, D, R, P: L.iddgcn_distmult_bce_f32(
            N, 0, D, R, q, q, q, q, q, q, N, 1.0, q, q, N, N, N, N, 1)),
        "iddgcn_distmult_bce_heads_f32": ("null", lambda L, D, R, P: L.iddgcn_distmult_bce_heads_f32(
            N, 1, D, R, N, N, N, N, N, N, N, 1.0, N, N, N, N, N, N, N, 1)),
        "iddgcn_seg_gather_reduce_f32": ("zero", lambda L, D, R, P: L.iddgcn_seg_gather_reduce_f32(
            N, 0, D, q, q, q, N, N, q, q, q)),
        "iddgcn_tail_seg_reduce_f32": ("zero", lambda L, D, R, P: L.iddgcn_tail_seg_reduce_f32(
            N, 0, D, R, q, q, q, q, q, 4096, q, 4096, q, q)),
        "iddgcn_head_bwd_node_f32": ("zero", lambda L, D, R, P: L.iddgcn_head_bwd_node_f32(
            N, 0, D, R, q, q, 4096, q, q, N, N, N, N, q, 4096, q, q)),
        "iddgcn_head_wsum_f32": ("zero", lambda L, D, R, P: L.iddgcn_head_wsum_f32(N, 0, R, q, q, q, q)),
        "iddgcn_gather_rows_f32": ("zero", lambda L, D, R, P: L.iddgcn_gather_rows_f32(N, 0, 4, q, q, q)),
        "iddgcn_reduce_slabs_f32": ("zero", lambda L, D, R, P: L.iddgcn_reduce_slabs_f32(N, 1, 0, q, q, 0, 1.0)),
        "iddgcn_adam_f32": ("zero", lambda L, D, R, P: L.iddgcn_adam_f32(N, 0, q, q, q, q, 1e-3, .9, .999, 1e-7, 0)),
        "iddgcn_adam_table_f32": ("zero", lambda L, D, R, P: L.iddgcn_adam_table_f32(
            N, 0, q, q, q, q, q, q, .9, .999, 1e-7, 0)),
        "iddgcn_rowgemm_bf16": ("zero", lambda L, D, R, P: L.iddgcn_rowgemm_bf16(N, ctypes.byref(rg(0, D, R, P, q)))),
        "iddgcn_gemm_tn_bf16": ("null", lambda L, D, R, P: L.iddgcn_gemm_tn_bf16(N, 1, D, N, N, N, 1, N, 0)),
        "iddgcn_sigma_tn_bf16": ("null", lambda L, D, R, P: L.iddgcn_sigma_tn_bf16(N, 1, D, N, N, N, N, 0, N, P)),
        "iddgcn_sigma_tn_f32": ("null", lambda L, D, R, P: L.iddgcn_sigma_tn_f32(N, 1, D, N, N, N, N, 0, N, P)),
        "iddgcn_combine_bf16": ("zero", lambda L, D, R, P: L.iddgcn_combine_bf16(N, 0, D, R, q, q, q, q, 4096, q)),
        "iddgcn_combine_planes_f32": ("zero", lambda L, D, R, P: L.iddgcn_combine_planes_f32(
            N, 0, D, R, q, q, q, q, 4096, q)),
        "iddgcn_distmult_bce_bf16": ("zero", lambda L, D, R, P: L.iddgcn_distmult_bce_bf16(
            N, 0, D, R, q, q, q, q, q, q, N, 1.0, q, q, N, N, N, N, 1)),
        "iddgcn_distmult_bce_heads_bf16": ("null", lambda L, D, R, P: L.iddgcn_distmult_bce_heads_bf16(
            N, 1, D, R, N, N, N, N, N, N, N, 1.0, N, N, N, N, N, N, N, 1)),
        "iddgcn_tail_seg_reduce_bf16": ("zero", lambda L, D, R, P: L.iddgcn_tail_seg_reduce_bf16(
            N, 0, D, R, q, q, q, q, q, 4096, q, 4096, q, q)),
        "iddgcn_tail_seg_reduce_head_bf16": ("zero", lambda L, D, R, P: L.iddgcn_tail_seg_reduce_head_bf16(
            N, 0, D, R, q, q, q, q, 4096, q, 4096, q, q, q, q, q)),
        "iddgcn_tail_seg_reduce_head_f32": ("zero", lambda L, D, R, P: L.iddgcn_tail_seg_reduce_head_f32(
            N, 0, D, R, q, q, q, q, 4096, q, 4096, q, q, q, q, q)),
        "iddgcn_head_dz_f32": ("zero", lambda L, D, R, P: L.iddgcn_head_dz_f32(N, 0, R, q, q, q, q, q, q, q)),
        "iddgcn_step_advance": ("null", lambda L, D, R, P: L.iddgcn_step_advance(N, N, N, N)),
    }
    e["_keepalive"] = ("", buf)
    return e


def refusal_cases():
    return list(itertools.product(REF_D, REF_R, REF_P))


def refusals(lib):
    """{entry: (mode, one character per (D, R, precision) case)}."""
    entries = refusal_entries()
    out = {}
    for name, (mode, call) in entries.items():
        if name.startswith("_"):
            continue
        out[name] = (mode, "".join(RC_CHAR.get(call(lib, D, R, P), "?") for D, R, P in refusal_cases()))
    return out


def geometry(lib):
    """[(function, args, value)] of the exported launch-geometry functions."""
    out = []
    for m in GEOM_ARGS:
        for d in (32, 64, 128, 256):
            out.append(("iddgcn_gemm_tn_blocks", (m, d), lib.iddgcn_gemm_tn_blocks(m, d)))
        for fn in ("iddgcn_gemm_tn_narrow_blocks", "iddgcn_distmult_blocks", "iddgcn_sigma_tn_ranges"):
            out.append((fn, (m,), getattr(lib, fn)(m)))
    return out


def geometry_text(rows):
    return "".join(f"{fn} {' '.join(map(str, args))} {v}\n" for fn, args, v in rows)


def refusals_text(table):
    return "".join(f"{name} {mode} {chars}\n" for name, (mode, chars) in table.items())


def ids_text(ids):
    """One letter per case in the order of id_cases(), runs of one letter written as the letter and their length
    (A4800), one (D, precision, R) slice of 1,152 cases per line."""
    import itertools as it
    head, chars = encode_ids(ids)
    w = 1152
    rle = lambda s: "".join(c + (str(n) if n > 1 else "") for c, n in ((c, len(list(g))) for c, g in it.groupby(s)))
    return head + "\n" + "".join(rle(chars[i:i + w]) + "\n" for i in range(0, len(chars), w))


def main():
    from iddgcn_amd import _lib
    if not os.environ.get("IDDGCN_LIB"):
        sys.exit("set IDDGCN_LIB to the library the goldens are recorded from (see the module docstring)")
    lib = _lib.load()
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for name, text in (("rowgemm_kernel_id.txt", ids_text(kernel_ids(lib))),
                       ("refusals.txt", refusals_text(refusals(lib))),
                       ("geometry.txt", geometry_text(geometry(lib)))):
        with open(os.path.join(GOLDEN_DIR, name), "w") as f:
            f.write(text)
        print(name, len(text), "bytes")


if __name__ == "__main__":
    main()
