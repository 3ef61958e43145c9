"""The host-side refusals of iddgcn_amd/ops.py, as a table of bad calls: one case per shared check (a strided view
with contiguous rows, a CSR pointer that ascends, the three layers' K / S / Wa / ba, (n, 3) int64 triples, the f32 /
bf16 entry pair, the Adam size loop, a given output) per wrapper that has it, plus a wrong dtype, a wrong shape and a
non-contiguous tensor for one argument of each of those wrappers.  Every case is refused with IddgcnError before
anything is launched, and ``match`` is the offending argument as the message names it: the intended check fired, not an
earlier one.  Shapes are the smallest that express a check (N = 8, R = 2, D = 32, six edges, two queries).

test_engine_candidate_refusals: the checks one level up, in the three Engine methods that take a candidate table
(tests/candidate_cases.py), with the whole message compared."""
import types

import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import ops
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from tests import candidate_cases as CC
from tests import ref_fidelity as RF

pytestmark = pytest.mark.gpu
N, R, D, M, Q, C, K_TOP = 8, 2, 32, 6, 2, 5, 3
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def wide(t):
    """t's values in a view whose row stride is the last dim + 4 (rows contiguous, 16-byte aligned, not adjacent)."""
    buf = torch.zeros(*t.shape[:-1], t.shape[-1] + 4, dtype=t.dtype, device=t.device)
    return buf[..., :t.shape[-1]]


def gappy(t):
    """t's shape with an inner stride of 2."""
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., ::2]


def short(t):
    """t without its last row."""
    return t[:-1].contiguous()


@pytest.fixture(scope="module")
def g(cuda):
    z = lambda *shape, dtype=F32: torch.zeros(*shape, dtype=dtype, device=cuda)           # noqa: E731
    ints = lambda vals, dtype=I32: torch.tensor(vals, dtype=dtype, device=cuda)           # noqa: E731
    g = types.SimpleNamespace()
    layers = dict(K=[z(R, D, D) for _ in range(3)], S=[z(D, D) for _ in range(3)], Wa=[z(D, R) for _ in range(3)],
                  ba=[z(R) for _ in range(3)])
    query = dict(h=ints([0, 1]), r=ints([0, 1]), t=ints([2, 3]))
    cands = dict(crel=ints([0, 1, 0, 1, 0]), ccol=ints([1, 2, 3, 4, 5]), crole=ints([0, 1, 2, 3, 0]))
    qptr = ints([0, 2, C], I64)
    seg_ptr = ints([0, 1, 2, 3, 4, 5, 6, 6, 6])
    g.rowgemm = dict(A=z(M, D), B=z(D, D), C=z(M, D))
    g.gemm_tn = dict(A=z(M, D), B=z(M, D), C=z(D, D), slab=z(ops.tn_blocks(M, D) * D * D))
    g.sigma_tn = dict(dO=z(M, D), X=z(M, D), S=z(D, D), dS=z(D, D), slab=z(D * D))
    g.combine = dict(Y=z(N, D), coef=z(M, R), V=z(R, N, D), out=z(M, D))
    slabs = dict(drel_slab=z(ops.distmult_blocks(M) * R * D), loss_slab=z(ops.distmult_blocks(M)))
    g.distmult_bce = dict(Xh=z(N, D), h_idx=ints([0, 1, 2, 3, 4, 5]), Xt=z(M, D), r_idx=ints([0, 1, 0, 1, 0, 1]),
                          rel=z(R, D), y=z(M), ds_out=z(M), do_out=z(M, D), **slabs)
    g.distmult_bce_heads = dict(seg_ptr=seg_ptr, perm=ints([0, 1, 2, 3, 4, 5]), Xh=z(N, D), Xt=z(M, D),
                                r_idx=ints([0, 1, 0, 1, 0, 1]), rel=z(R, D), y=z(M), do_out=z(M, D), dXh=z(N, D),
                                **slabs)
    g.tail_seg_reduce = dict(seg_ptr=seg_ptr, h_idx=None, W=z(M, R), dO=z(M, D), P=z(R, N, D), dP=z(R, N, D),
                             dWedge=z(M, R))
    g.tail_seg_reduce_head = dict(seg_ptr=seg_ptr, W=z(M, R), dO=z(M, D), P=z(R, N, D), dP=z(R, N, D), dWedge=z(M, R),
                                  head_dO=z(N, D), Wn=z(N, R), dwh=z(N, R))
    g.head_bwd_node = dict(dO=z(N, D), P=z(R, N, D), Ssm=z(N, R), W=z(N, R), dP=z(R, N, D), dz=z(N, R))
    g.adam = dict(var=z(10), m=z(10), v=z(10), g=z(10), alpha=1e-3, b1=0.9, b2=0.999, eps=1e-7, sparse_form=0)
    g.adam_table = dict(var=z(10), m=z(10), v=z(10), g=z(10), alpha_table=z(4), step=z(1, dtype=I32), b1=0.9, b2=0.999,
                        eps=1e-7, sparse_form=0)
    tri = ints([[0, 0, 1], [1, 1, 2], [2, 0, 3]], I64)
    g.build_adjacency = dict(triples=tri, N=N, R=R)
    g.build_scored_edges = dict(triples=tri, labels=z(3), N=N, R=R)
    g.negative_samples = dict(triples=tri, num_entities=N, seed=0)
    g.gt_sim_lists = dict(sim=tri, N=N)
    g.screen_chain = dict(q_node=ints([0, 1]), q_rel=ints([0, 1]), ES1=z(N, D), P=z(3, R, N, D), W=z(3, N, R),
                          X3=z(N, D), S2=z(D, D), S3=z(D, D), rel=z(R, D), s=z(Q, N))
    g.rank_topk = dict(s=z(Q, N), target=ints([0, 1]), k=K_TOP, fptr=ints([0, 1, 2]), fidx=ints([3, 4]),
                       greater=z(Q, dtype=I32), equal=z(Q, dtype=I32), topk_idx=z(Q, K_TOP, dtype=I32),
                       topk_val=z(Q, K_TOP))
    g.explain_seeds = dict(**query, ES1=z(N, D), P=z(3, R, N, D), W=z(3, N, R), Ssm=z(3, N, R), X=z(3, N, D),
                           K=layers["K"], S2=z(D, D), S3=z(D, D), Wa2=z(D, R), Wa3=z(D, R), rel=z(R, D),
                           G=z(Q, 2, R, D), p=z(Q))
    g.explain_row_grads = dict(h=query["h"], t=query["t"], row_ptr=z(R * (N + 1), dtype=I32), col=z(4, dtype=I32),
                               G=z(Q, 2, R, D), E=z(N, D), qptr=qptr, entry=z(C, dtype=I32), grad=z(C))
    g.explain_topk = dict(qptr=qptr, entry=z(C, dtype=I32), grad=z(C), k=K_TOP, topk_entry=z(Q, K_TOP, dtype=I32),
                          topk_val=z(Q, K_TOP), n_pos=z(Q, dtype=I32))
    g.mask_explain = dict(E=z(N, D), **layers, rel=z(R, D), **query, qptr=qptr, entry=ints([0, 1, 2, 3, 4]), **cands,
                          init_e=z(7), m=z(7), v=z(7), steps=z(7, dtype=I32), alpha=z(2 * Q), out=z(C),
                          qids=ints([0, 1]), level_ptr=[0, 2], num_epochs=2)
    g.explain_curves = dict(E=z(N, D), **layers, rel=z(R, D), **query, qptr=qptr, **cands,
                            cstep=ints([0, 1, -1, 0, 2]), cval=z(C), k=K_TOP,
                            deletion=z(Q, K_TOP + 1), insertion=z(Q, K_TOP + 1))
    return g


def bad(wrapper, **changes):
    """A case: ops.<wrapper> with its valid arguments, ``changes`` (values, or functions of the valid value) applied."""
    def call(g):
        args = dict(getattr(g, wrapper))
        for k, v in changes.items():
            args[k] = v(args[k]) if callable(v) else v
        getattr(ops, wrapper)(**args)
    return call


RANGES = True        # the case runs with ops.CHECK_INDEX_RANGES on
CASES = [
    # -- a strided view with contiguous rows: fp32, on the GPU, the shape, row stride = last dim, unit inner stride
    ("tail_seg_reduce: P row stride", bad("tail_seg_reduce", P=wide), r"\bP must be"),
    ("tail_seg_reduce: dP inner stride", bad("tail_seg_reduce", dP=gappy), r"\bdP must be"),
    ("tail_seg_reduce: P dtype", bad("tail_seg_reduce", P=torch.Tensor.double), r"\bP must be"),
    ("tail_seg_reduce_head: dP row stride", bad("tail_seg_reduce_head", dP=wide), r"\bdP must be"),
    ("tail_seg_reduce_head: P shape", bad("tail_seg_reduce_head", P=lambda t: t[:, :, :16]), r"\bP must be"),
    ("head_bwd_node: P row stride", bad("head_bwd_node", P=wide), r"\bP must be"),
    ("head_bwd_node: dP row stride", bad("head_bwd_node", dP=wide), r"\bdP must be"),
    ("head_bwd_node: dP inner stride", bad("head_bwd_node", dP=gappy), r"\bdP must be"),
    ("screen_chain: P row stride", bad("screen_chain", P=wide), r"\bP must be"),
    ("screen_chain: W row stride", bad("screen_chain", W=wide), r"\bW must be"),
    ("screen_chain: W transposed", bad("screen_chain", W=lambda t: t.transpose(1, 2)), r"\bW must be"),
    ("screen_chain: P dtype", bad("screen_chain", P=torch.Tensor.double), r"\bP must be"),
    ("screen_chain: P missing", bad("screen_chain", P=None), r"\bP must be"),
    ("explain_seeds: P row stride", bad("explain_seeds", P=wide), r"\bP must be"),
    ("explain_seeds: W row stride", bad("explain_seeds", W=wide), r"\bW must be"),
    ("explain_seeds: Ssm inner stride", bad("explain_seeds", Ssm=gappy), r"\bSsm must be"),
    ("explain_seeds: X row stride", bad("explain_seeds", X=wide), r"\bX must be"),
    ("explain_seeds: X dtype", bad("explain_seeds", X=torch.Tensor.half), r"\bX must be"),
    # -- a CSR pointer ascends within [0, limit] (or from 0 to exactly the limit), an index lies in its range
    ("rank_topk: fptr descends", bad("rank_topk", fptr=lambda t: t.flip(0).contiguous()), "fptr must ascend", RANGES),
    ("rank_topk: fptr past fidx", bad("rank_topk", fptr=lambda t: t + 1), "fptr must ascend", RANGES),
    ("rank_topk: target out of range", bad("rank_topk", target=lambda t: t + N), "target: index out of range", RANGES),
    ("explain_row_grads: qptr descends", bad("explain_row_grads", qptr=lambda t: t.flip(0).contiguous()),
     "qptr must ascend", RANGES),
    ("explain_row_grads: qptr past entry", bad("explain_row_grads", qptr=lambda t: t + 1), "qptr must ascend", RANGES),
    ("explain_row_grads: h out of range", bad("explain_row_grads", h=lambda t: t + N), "h: index out of range", RANGES),
    ("explain_topk: qptr descends", bad("explain_topk", qptr=lambda t: t.flip(0).contiguous()), "qptr must ascend",
     RANGES),
    ("explain_topk: qptr negative", bad("explain_topk", qptr=lambda t: t - 1), "qptr must ascend", RANGES),
    ("mask_explain: qptr descends", bad("mask_explain", qptr=lambda t: t.flip(0).contiguous()), "qptr must ascend",
     RANGES),
    ("mask_explain: qptr ends short of C", bad("mask_explain", qptr=lambda t: t - t.clamp(max=1)), "qptr must ascend",
     RANGES),
    ("mask_explain: qptr starts above 0", bad("mask_explain", qptr=lambda t: t.clamp(min=1)), "qptr must ascend",
     RANGES),
    ("mask_explain: crel out of range", bad("mask_explain", crel=lambda t: t + R), "crel: index out of range", RANGES),
    ("explain_curves: qptr descends", bad("explain_curves", qptr=lambda t: t.flip(0).contiguous()), "qptr must ascend",
     RANGES),
    ("explain_curves: qptr past C", bad("explain_curves", qptr=lambda t: t + 1), "qptr must ascend", RANGES),
    ("explain_curves: ccol out of range", bad("explain_curves", ccol=lambda t: t + N), "ccol: index out of range",
     RANGES),
    ("explain_curves: cstep out of range", bad("explain_curves", cstep=lambda t: t + 1), "cstep must lie", RANGES),
    ("explain_seeds: r out of range", bad("explain_seeds", r=lambda t: t + R), "r: index out of range", RANGES),
    ("screen_chain: q_node out of range", bad("screen_chain", q_node=lambda t: t - 1), "q_node: index out of range",
     RANGES),
    # -- the three layers' K, S, Wa, ba
    ("mask_explain: two-element K", bad("mask_explain", K=lambda xs: xs[:2]), "K, S, Wa, ba must hold"),
    ("mask_explain: a None layer", bad("mask_explain", S=lambda xs: [xs[0], None, xs[2]]),
     "every layer's K, S, Wa, ba"),
    ("mask_explain: K2 shape", bad("mask_explain", K=lambda xs: [xs[0], xs[1][:, :, :16].contiguous(), xs[2]]),
     "K2: expected shape"),
    ("mask_explain: ba3 dtype", bad("mask_explain", ba=lambda xs: [xs[0], xs[1], xs[2].double()]), "ba3: expected"),
    ("explain_curves: two-element K", bad("explain_curves", K=lambda xs: xs[:2]), "K, S, Wa, ba must hold"),
    ("explain_curves: four-element ba", bad("explain_curves", ba=lambda xs: xs + xs[:1]), "K, S, Wa, ba must hold"),
    ("explain_curves: a None layer", bad("explain_curves", Wa=lambda xs: [None, xs[1], xs[2]]),
     "every layer's K, S, Wa, ba"),
    ("explain_curves: S1 not contiguous", bad("explain_curves", S=lambda xs: [gappy(xs[0]), xs[1], xs[2]]),
     "S1 must be contiguous"),
    ("explain_curves: Wa2 shape", bad("explain_curves", Wa=lambda xs: [xs[0], xs[1].t().contiguous(), xs[2]]),
     "Wa2: expected shape"),
    # -- (n, 3) int64 triples
    ("build_adjacency: triples (n, 2)", bad("build_adjacency", triples=lambda t: t[:, :2].contiguous()),
     "triples must be"),
    ("build_adjacency: triples dtype", bad("build_adjacency", triples=torch.Tensor.int), "triples: expected"),
    ("build_scored_edges: triples 1-d", bad("build_scored_edges", triples=lambda t: t[:, 0].contiguous()),
     "triples must be"),
    ("build_scored_edges: triples columns", bad("build_scored_edges", triples=lambda t: t[:, :1]), "triples must be"),
    ("negative_samples: triples (n, 4)", bad("negative_samples", triples=lambda t: torch.cat([t, t[:, :1]], 1)),
     "triples must be"),
    ("negative_samples: triples not contiguous", bad("negative_samples", triples=gappy), "triples must be contiguous"),
    ("gt_sim_lists: sim (n, 2)", bad("gt_sim_lists", sim=lambda t: t[:, :2].contiguous()), "sim must be"),
    # -- the f32 / bf16 entry pair: the tables of one call share the element type
    ("rowgemm: bf16 A, fp32 C", bad("rowgemm", A=torch.Tensor.bfloat16), "C: expected"),
    ("rowgemm: fp32 A, bf16 C", bad("rowgemm", C=torch.Tensor.bfloat16), "C: expected"),
    ("rowgemm: A width", bad("rowgemm", A=lambda t: t[:, :16].contiguous()), "A must be"),
    ("rowgemm: B not contiguous", bad("rowgemm", B=gappy), "B must be contiguous"),
    ("gemm_tn: planes A outside split mode", bad("gemm_tn", a_planes=True, precision="exact"), "planes A"),
    ("gemm_tn: planes A of bf16 tables", bad("gemm_tn", A=torch.Tensor.bfloat16, B=torch.Tensor.bfloat16, a_planes=True,
                                             precision="split"), "planes A"),
    ("gemm_tn: bf16 A, fp32 B", bad("gemm_tn", A=torch.Tensor.bfloat16), "B: expected"),
    ("gemm_tn: row-GEMM precision", bad("gemm_tn", precision="exact4"), "row-GEMM form"),
    ("sigma_tn: fp32 tables, exact", bad("sigma_tn", precision="exact"), "bf16x3"),
    ("sigma_tn: fp32 tables, split", bad("sigma_tn", precision="split"), "bf16x3"),
    ("sigma_tn: bf16 tables, exact4", bad("sigma_tn", X=torch.Tensor.bfloat16, dO=torch.Tensor.bfloat16,
                                          precision="exact4"), "not a form of the bf16 pass"),
    ("sigma_tn: bf16 X, fp32 dO", bad("sigma_tn", X=torch.Tensor.bfloat16, precision="bf16x3"), "dO: expected"),
    ("sigma_tn: dS shape", bad("sigma_tn", dS=short, precision="bf16x3"), "dS: expected shape"),
    ("combine: out dtype", bad("combine", out=torch.Tensor.double), "out: expected"),
    ("combine: bf16 out without the run form", bad("combine", out=torch.Tensor.bfloat16), "y_idx and v_idx"),
    ("combine: out not contiguous", bad("combine", out=gappy), "out must be contiguous"),
    ("combine: Y dtype", bad("combine", Y=torch.Tensor.bfloat16), "Y: expected"),
    ("distmult_bce: bf16 Xt, fp32 do_out", bad("distmult_bce", Xt=torch.Tensor.bfloat16), "do_out: expected"),
    ("distmult_bce: r_idx dtype", bad("distmult_bce", r_idx=torch.Tensor.long), "r_idx: expected"),
    ("distmult_bce: y shape", bad("distmult_bce", y=short), "y: expected shape"),
    ("distmult_bce: rel not contiguous", bad("distmult_bce", rel=gappy), "rel must be contiguous"),
    ("distmult_bce_heads: bf16 Xt, fp32 do_out", bad("distmult_bce_heads", Xt=torch.Tensor.bfloat16),
     "do_out: expected"),
    ("distmult_bce_heads: fp32 Xt, bf16 do_out", bad("distmult_bce_heads", do_out=torch.Tensor.bfloat16),
     "do_out: expected"),
    ("distmult_bce_heads: Xh not contiguous", bad("distmult_bce_heads", Xh=gappy), "Xh must be contiguous"),
    ("distmult_bce_heads: perm shape", bad("distmult_bce_heads", perm=short), "perm: expected shape"),
    ("tail_seg_reduce: dO dtype", bad("tail_seg_reduce", dO=torch.Tensor.half), "dO: expected"),
    ("tail_seg_reduce: dO not contiguous", bad("tail_seg_reduce", dO=gappy), "dO must be contiguous"),
    ("tail_seg_reduce: seg_ptr shape", bad("tail_seg_reduce", seg_ptr=short), "seg_ptr: expected shape"),
    ("tail_seg_reduce_head: dO dtype", bad("tail_seg_reduce_head", dO=torch.Tensor.double), "dO: expected"),
    ("tail_seg_reduce_head: Wn shape", bad("tail_seg_reduce_head", Wn=short), "Wn: expected shape"),
    ("tail_seg_reduce_head: dwh not contiguous", bad("tail_seg_reduce_head", dwh=gappy), "dwh must be contiguous"),
    ("head_bwd_node: dO dtype", bad("head_bwd_node", dO=torch.Tensor.double), "dO: expected"),
    ("head_bwd_node: Ssm shape", bad("head_bwd_node", Ssm=short), "Ssm: expected shape"),
    ("head_bwd_node: dz not contiguous", bad("head_bwd_node", dz=gappy), "dz must be contiguous"),
    # -- the m / v / g size loop
    ("adam: m size", bad("adam", m=short), "adam: m size"),
    ("adam: g size", bad("adam", g=short), "adam: g size"),
    ("adam_table: v size", bad("adam_table", v=short), "adam: v size"),
    ("adam_table: step dtype", bad("adam_table", step=torch.Tensor.long), "step: expected"),
    # -- an output that is given is checked like one that is allocated
    ("rank_topk: greater dtype", bad("rank_topk", greater=torch.Tensor.long), "greater: expected"),
    ("rank_topk: topk_val shape", bad("rank_topk", topk_val=short), "topk_val: expected shape"),
    ("rank_topk: topk_idx not contiguous", bad("rank_topk", topk_idx=gappy), "topk_idx must be contiguous"),
    ("rank_topk: s dtype", bad("rank_topk", s=torch.Tensor.double), "s: expected"),
    ("rank_topk: target shape", bad("rank_topk", target=short), "target: expected shape"),
    ("rank_topk: fidx not contiguous", bad("rank_topk", fidx=gappy), "fidx must be contiguous"),
    ("explain_topk: n_pos shape", bad("explain_topk", n_pos=short), "n_pos: expected shape"),
    ("explain_topk: topk_entry dtype", bad("explain_topk", topk_entry=torch.Tensor.long), "topk_entry: expected"),
    ("explain_topk: qptr dtype", bad("explain_topk", qptr=torch.Tensor.int), "qptr: expected"),
    ("explain_topk: grad shape", bad("explain_topk", grad=short), "entry and grad"),
    ("explain_topk: entry not contiguous", bad("explain_topk", entry=gappy), "entry must be contiguous"),
    ("explain_seeds: G not contiguous", bad("explain_seeds", G=gappy), "G must be contiguous"),
    ("explain_seeds: p dtype", bad("explain_seeds", p=torch.Tensor.double), "p: expected"),
    ("explain_seeds: ES1 shape", bad("explain_seeds", ES1=lambda t: t[:, :16].contiguous()), "ES1: expected shape"),
    ("explain_seeds: K of two", bad("explain_seeds", K=lambda xs: xs[:2]), "K must be"),
    ("explain_curves: deletion shape", bad("explain_curves", deletion=short), "deletion: expected shape"),
    ("explain_curves: insertion dtype", bad("explain_curves", insertion=torch.Tensor.double), "insertion: expected"),
    ("explain_curves: E dtype", bad("explain_curves", E=torch.Tensor.double), "E: expected"),
    ("explain_curves: cval shape", bad("explain_curves", cval=short), "cval: expected shape"),
    ("explain_curves: rel not contiguous", bad("explain_curves", rel=gappy), "rel must be contiguous"),
    ("mask_explain: steps dtype", bad("mask_explain", steps=torch.Tensor.long), "steps: expected"),
    ("mask_explain: out shape", bad("mask_explain", out=short), "out: expected shape"),
    ("mask_explain: E not contiguous", bad("mask_explain", E=gappy), "E must be contiguous"),
    ("explain_row_grads: qptr dtype", bad("explain_row_grads", qptr=torch.Tensor.int), "qptr: expected"),
    ("explain_row_grads: E shape", bad("explain_row_grads", E=lambda t: t[:, :16].contiguous()), "E: expected shape"),
    ("explain_row_grads: G not contiguous", bad("explain_row_grads", G=gappy), "G must be contiguous"),
    ("screen_chain: s dtype", bad("screen_chain", s=torch.Tensor.double), "s: expected"),
    ("screen_chain: X3 shape", bad("screen_chain", X3=short), "X3: expected shape"),
    ("screen_chain: ES1 not contiguous", bad("screen_chain", ES1=gappy), "ES1 must be contiguous"),
    ("build_scored_edges: labels shape", bad("build_scored_edges", labels=short), "labels: expected shape"),
]


@pytest.mark.parametrize("call, match, ranges", [pytest.param(c[1], c[2], len(c) > 3, id=c[0]) for c in CASES])
def test_refused(call, match, ranges, g, monkeypatch):
    monkeypatch.setattr(ops, "CHECK_INDEX_RANGES", ranges)
    with pytest.raises(L.IddgcnError, match=match):
        call(g)


ENVELOPE = {"edit_curves": "edit_curves takes D in {32, 64}, fp32 features, 1 <= R <= 8 and an unsharded engine: use "
                           "explain.fidelity_curves(fused=False) for this engine",
            "counterfactual_search": "counterfactual_search takes D in {32, 64}, fp32 features, 1 <= R <= 8 and an "
                                     "unsharded engine: use explain.counterfactual_batched(fused=False) for this engine",
            "integrated_gradients": "integrated_gradients takes D in {32, 64}, fp32 features, 1 <= R <= 8 and an "
                                    "unsharded engine: use explain.integrated_gradients_batched(fused=False) for this "
                                    "engine"}


def test_engine_candidate_refusals(cuda):
    """Engine.edit_curves / counterfactual_search / integrated_gradients refuse a malformed call before any launch,
    with the exception type and the whole message of the table; then a good call of each returns its shapes."""
    assert (CC.N, CC.R, CC.Q, CC.C) == (N, R, Q, C)
    K = CC.K
    tri = np.array([[0, 0, 1], [1, 1, 2], [2, 0, 3], [3, 1, 0]], np.int64)
    rule = (np.array([0.25, 0.75]), np.array([0.5, 0.5]))

    def setup(n, d):
        model = RF.model_with(RF.make_params(n, R, d, np.random.default_rng(5)), n, R, d)
        eng = model._device_state()
        return eng, model._params

    eng, params = setup(N, D)
    dadj = DeviceAdjacency(get_adj_mats(tri, N, R), N, eng.device)

    def call(who, cand, eng=eng, params=params, adj=dadj, q=CC.TRIPLES, K=K, rule=rule, **kw):
        args = (K,) if who != "integrated_gradients" else rule
        return getattr(eng, who)(params, adj, q, cand, *args, **kw)

    def refused(kind, message, who, cand=None, **kw):
        with pytest.raises(kind) as e:
            call(who, CC.base(who) if cand is None else cand, **kw)
        assert type(e.value) is kind and str(e.value) == message, (who, kw, str(e.value))

    accepted = []
    for name, who, cand, message in CC.cases():
        if message is None:
            accepted.append((name, who, cand))
        else:
            refused(L.IddgcnError, message, who, cand)
    other_adj = DeviceAdjacency(get_adj_mats(tri, N + 1, R), N + 1, eng.device)
    big_eng, big_params = setup(N, 128)
    for who in CC.EXTRA:
        refused(L.IddgcnError, f"{who}: the adjacency is not this engine's size", who, adj=other_adj)
        refused(ValueError, "max_entries must be positive, got 0", who, max_entries=0)
        refused(L.IddgcnError, "triple entity index out of range [0, num_entities)", who,
                q=np.array([[0, 0, 2], [1, 1, N]], np.int64))
        refused(L.IddgcnError, ENVELOPE[who], who, eng=big_eng, params=big_params)
    for k in (0, 65):
        refused(L.IddgcnError, f"edit_curves: K must be in [1, 64], got {k}", "edit_curves", K=k)
    for k in (-1, 65):
        refused(L.IddgcnError, f"counterfactual_search: K must be in [0, 64], got {k}", "counterfactual_search", K=k)
    for m_alpha, m_omega in ((2, 3), (0, 0), (1025, 1025)):
        refused(L.IddgcnError, "integrated_gradients: alpha and omega must be (m,) with m in [1, 1024]",
                "integrated_gradients", rule=(np.full(m_alpha, 0.5), np.full(m_omega, 1.0 / max(m_omega, 1))))

    def shapes(out):
        return {k: tuple(v.shape) for k, v in out.items()} if isinstance(out, dict) else [tuple(v.shape) for v in out]

    for name, who, cand in accepted:
        none = {k: (v[:1] if k == "qptr" else v[:0]) for k, v in cand.items()}          # the same call of no query
        for q, cd in ((CC.TRIPLES, cand), (CC.TRIPLES[:0], none)):
            n, c = len(q), len(cd["rel"])
            want = {"edit_curves": [(n, K + 1), (n, K + 1)],
                    "counterfactual_search": dict(path=(n, K + 1), chosen=(n, K), n_steps=(n,), flipped=(n,),
                                                  cstep=(c,), loo=(c,)),
                    "integrated_gradients": dict(attr=(c,), total=(n,), p_full=(n,), p_base=(n,), gap=(n,))}[who]
            assert shapes(call(who, cd, q=q)) == want, (name, n)
    torch.cuda.synchronize()
