"""The fused tail + head-term reduction over fp32 rows (iddgcn_tail_seg_reduce_head_f32: D = 256, R <= 2, per-edge W)
and the head_dz that finishes the head backward after it, on the graphs of test_gpu_step_kernels.GRAPHS (an empty tail
segment, a one-edge segment, segments that are no multiple of the 4-row group, a node count that is no multiple of the
4 nodes per block).  Head segments come from an independent random h, so some heads have no edges.

  * dWedge is BITWISE tail_seg_reduce's, dP and dsum BITWISE tail_seg_reduce followed by head_bwd_node (the head term
    enters by the same single fma / add on the same operands);
  * against fp64, per element: dP within gamma(len + 3) (sum_e |W d| + |Wn hd|) — tail_ref's gamma(len + 1) terms and
    one more rounded product and add —, dsum within gamma(len + 1) (sum_e |d| + |hd|), dwh within gamma(D + 1) sum |hd P|;
  * dz of the pair against the fp64 evaluation of the same inputs: dW_r = <hd, P_r[n]> + sum over the head segment of
    <dO[e], P_r[t_e]> is a sum of (len + 1) D products, each product rounded once, then at most D + len + 1 adds on
    its way: gamma(D + len + 2) sum |products|, propagated through the softmax-sigmoid backward (softsig_bwd);
  * NaN-prefilled outputs with guard rows, P / dP as row ranges of larger tables; twice (bitwise); without dsum.

The engine A/B (fuse_tail_head True / False on one small bf16x3 engine) is at the end."""
import numpy as np
import pytest
import torch

from bounds import NAN, assert_within, gam, guard_intact, guarded, rejects
from iddgcn_amd import _lib as L
from iddgcn_amd import ops
from test_gpu_step_kernels import (GRAPHS, _gen, check_all, last_group, segsum, softsig_bwd, tail_inputs,
                                   tail_ref)

gpu = pytest.mark.gpu
I32, F64 = torch.int32, torch.float64


def fused_inputs(case, R, D, seed):
    """tail_inputs with W gathered per edge, plus the head side: segments of an independent h, the head seed and the
    node-level softmax / dynamic weights."""
    N, T, t, ptr, h, W, dO, P = tail_inputs(case, R, D, seed)
    g = _gen(seed + 2)
    h2 = torch.randint(0, N, (T,), generator=g)
    hperm = torch.argsort(h2, stable=True)
    node_k = h2[hperm].contiguous()
    hptr = torch.searchsorted(node_k, torch.arange(N + 1), right=False).to(I32)
    S = torch.softmax(torch.randn(N, R, generator=g), -1)
    return dict(N=N, T=T, R=R, D=D, t=t, ptr=ptr, We=W[h].contiguous(), dO=dO, P=P, hperm=hperm, node_k=node_k,
                hptr=hptr, S=S, Wn=torch.sigmoid(S), hd=torch.randn(N, D, generator=g))


def fused_refs(i, drop=None, head_term=True):
    """name -> (fp64 reference, bound) of the fused pair's outputs.  drop: a mask of tail edges left out;
    head_term = False leaves Wn hd out of dP (the perturbation the bar must refuse)."""
    N, D, R, t = i["N"], i["D"], i["R"], i["t"]
    tr = tail_ref(N, t, i["ptr"], None, i["We"], i["dO"], i["P"], drop=drop)
    ln = (i["ptr"][1:] - i["ptr"][:-1]).double()
    hd, Pd, d = i["hd"].double(), i["P"].double(), i["dO"].double()
    wd = i["Wn"].double().t()[:, :, None] * hd[None]                     # (R, N, D)
    absP = tr["dP"][1] / gam(ln + 1)[None, :, None]                      # sum_e |W d|
    absS = segsum(d.abs() * (1.0 if drop is None else (~drop).double()[:, None]), t, N)
    out = {"dP": (tr["dP"][0] + (wd if head_term else 0.0), gam(ln + 3)[None, :, None] * (absP + wd.abs())),
           "dsum": (tr["dsum"][0] + hd, gam(ln + 1)[:, None] * (absS + hd.abs())),
           "dWedge": tr["dWedge"]}
    q = hd[None] * Pd                                                    # (R, N, D)
    out["dwh"] = (q.sum(2).t(), gam(D + 1) * q.abs().sum(2).t())
    # dz: the head segment's dWedge rows as fp64 products of the same inputs
    dwe = torch.stack([(d * Pd[r][t]).sum(1) for r in range(R)], 1)[i["hperm"]]
    dwa = torch.stack([(d * Pd[r][t]).abs().sum(1) for r in range(R)], 1)[i["hperm"]]
    hl = (i["hptr"][1:] - i["hptr"][:-1]).double()
    dW = out["dwh"][0] + segsum(dwe, i["node_k"], N)
    A = q.abs().sum(2).t() + segsum(dwa, i["node_k"], N)
    out["dz"] = softsig_bwd(dW, gam(D + hl + 2)[:, None] * A, i["S"], i["Wn"])
    return out


def test_selfcheck_fused_bounds():
    """CPU: an fp32 evaluation passes the bars; a dropped last edge group, swapped relations and a dP without its
    head term do not."""
    i = fused_inputs("small", 2, 32, 5)
    N, R, t = i["N"], i["R"], i["t"]
    refs = fused_refs(i)
    tail32 = torch.stack([segsum(i["We"][:, r:r + 1] * i["dO"], t, N) for r in range(R)])
    dwe32 = torch.stack([(i["dO"] * i["P"][r][t]).sum(1) for r in range(R)], 1)
    dwh32 = (i["hd"][None] * i["P"]).sum(2).t()
    ds = (dwh32 + segsum(dwe32[i["hperm"]], i["node_k"], N)) * i["Wn"] * (1 - i["Wn"])
    em = {"dP": tail32 + i["Wn"].t()[:, :, None] * i["hd"][None], "dsum": segsum(i["dO"], t, N) + i["hd"],
          "dWedge": dwe32, "dwh": dwh32, "dz": (ds - (ds * i["S"]).sum(1, keepdim=True)) * i["S"]}
    check_all(em, refs, "cpu-fp32 fused tail + head")
    dropped = fused_refs(i, drop=last_group(i["ptr"], i["T"]))
    for k in ("dP", "dsum", "dWedge"):
        assert rejects(dropped[k][0], *refs[k]), f"{k}: dropping the last ragged edge group passes the bar"
    assert rejects(refs["dP"][0].flip(0), *refs["dP"]), "dP: swapped relations pass the bar"
    assert rejects(refs["dwh"][0].flip(1), *refs["dwh"]), "dwh: swapped relations pass the bar"
    assert rejects(fused_refs(i, head_term=False)["dP"][0], *refs["dP"]), "dP without Wn head_dO passes the bar"
    assert rejects(tail_ref(N, t, i["ptr"], None, i["We"], i["dO"], i["P"])["dsum"][0], *refs["dsum"]), \
        "dsum without head_dO passes the bar"


class Dev:
    """The inputs on the device, P as the row range [2, 2 + N) of an (R, N + 3, D) NaN table."""

    def __init__(self, i, cuda):
        N, R, D = i["N"], i["R"], i["D"]
        self.i, self.cuda = i, cuda
        self.Pb = torch.full((R, N + 3, D), NAN, device=cuda)
        self.Pb[:, 2:2 + N] = i["P"].to(cuda)
        for k in ("ptr", "We", "dO", "hd", "Wn", "S", "hptr"):
            setattr(self, k, i[k].to(cuda))
        self.hperm = i["hperm"].to(I32).to(cuda)

    def outputs(self):
        i = self.i
        N, T, R, D = i["N"], i["T"], i["R"], i["D"]
        o = dict(dPb=torch.full((R, N + 3, D), NAN, device=self.cuda))
        for k, shape in (("dWedge", (T, R)), ("dsum", (N, D)), ("dwh", (N, R)), ("dz", (N, R))):
            o["w_" + k], o[k] = guarded(self.cuda, *shape)
        return o

    def collect(self, o, dsum, names):
        N = self.i["N"]
        dPb = o["dPb"]
        assert bool(torch.isnan(dPb[:, :2]).all()) and bool(torch.isnan(dPb[:, 2 + N:]).all()), "dP rows outside the view"
        for k in ("dWedge", "dwh", "dz"):
            guard_intact(o["w_" + k], k)
        assert bool(torch.isnan(o["w_dsum"][-1] if dsum else o["w_dsum"]).all()), "dsum written without being asked"
        out = {k: o[k].cpu() for k in names if k != "dP" and (k != "dsum" or dsum)}
        out["dP"] = dPb[:, 2:2 + N].cpu()
        return out

    def fused(self, dsum=True):
        N = self.i["N"]
        o = self.outputs()
        ops.tail_seg_reduce_head(self.ptr, self.We, self.dO, self.Pb[:, 2:2 + N], o["dPb"][:, 2:2 + N], o["dWedge"],
                                 self.hd, self.Wn, o["dwh"], dsum=o["dsum"] if dsum else None)
        ops.head_dz(self.S, self.Wn, self.hptr, self.hperm, o["dWedge"], o["dwh"], o["dz"])
        return self.collect(o, dsum, ("dP", "dsum", "dWedge", "dwh", "dz"))

    def unfused(self, dsum=True):
        N = self.i["N"]
        o = self.outputs()
        o["dwh"].zero_()                    # not an output of this pair
        ops.tail_seg_reduce(self.ptr, None, self.We, self.dO, self.Pb[:, 2:2 + N], o["dPb"][:, 2:2 + N], o["dWedge"],
                            dsum=o["dsum"] if dsum else None)
        tail_dwe = o["dWedge"].clone()
        ops.head_bwd_node(self.hd, self.Pb[:, 2:2 + N], self.S, self.Wn, o["dPb"][:, 2:2 + N], o["dz"],
                          hseg_ptr=self.hptr, hperm=self.hperm, dWedge=o["dWedge"], dsum=o["dsum"] if dsum else None)
        assert torch.equal(tail_dwe, o["dWedge"])
        return self.collect(o, dsum, ("dP", "dsum", "dWedge", "dz"))


@gpu
@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("R", [1, 2])
def test_tail_seg_reduce_head_f32(R, case, cuda):
    i = fused_inputs(case, R, 256, 17 * R + len(case))
    what = f"tail_seg_reduce_head_f32 {case} R{R}"
    refs = fused_refs(i)
    dev = Dev(i, cuda)
    a = dev.fused()
    check_all(a, refs, what)
    b = dev.fused()
    for k in ("dP", "dsum", "dWedge", "dwh", "dz"):
        assert torch.equal(a[k], b[k]), f"{what} run twice: {k} differs"
    u = dev.unfused()
    for k in ("dWedge", "dP", "dsum"):
        assert torch.equal(a[k], u[k]), f"{what}: {k} is not bitwise the unfused pair's"
    assert_within(u["dz"], *refs["dz"], what + " (unfused pair) dz")
    c = dev.fused(dsum=False)                # the layer-2/3 call
    for k in ("dP", "dWedge", "dwh", "dz"):
        assert torch.equal(a[k], c[k]), f"{what} without dsum: {k} differs"


@gpu
def test_tail_seg_reduce_head_f32_refuses_other_shapes(cuda):
    """Shapes without a fused fp32 form are an error (IDDGCN_E_BAD_ARG), never another kernel."""
    for R, D in ((3, 256), (8, 256), (2, 128), (2, 64)):
        i = fused_inputs("tiny", R, D, 3)
        with pytest.raises(L.IddgcnError):
            Dev(i, cuda).fused()


# ---- the engine with and without the fused pair ------------------------------------------------------------
@gpu
def test_engine_fuse_tail_head_ab(cuda, monkeypatch):
    """One small bf16x3 engine, loss_and_grads with fuse_tail_head True and False: the loss (the forward is untouched)
    and the gradients that dP reaches without passing through dz — K3 and the top layer's dAE contribution — are
    bitwise equal; the unfused run meets the bars of test_gpu_model.test_wide_step_parity_vs_oracle against the
    float64 oracle (loss 1e-5 relative, scores 1e-5, gradients 2e-4 of max|g|)."""
    from iddgcn_amd.engine import Engine, FlatParams
    from iddgcn_amd.graph import get_adj_mats
    from iddgcn_amd.utils import synthetic_graph
    from oracle.ref_model import train_step_grads
    from oracle.ref_utils import get_adj_coo
    N, R, D = 301, 2, 256
    pos, neg = synthetic_graph(N, R, 1200, seed=5)
    neg = neg[:800]
    rng = np.random.default_rng(1)
    params = {"E": rng.standard_normal((N, D)) / np.sqrt(D)}
    for l in (1, 2, 3):
        params[f"K{l}"] = rng.standard_normal((R, D, D)) / D
        params[f"S{l}"] = rng.standard_normal((D, D)) / np.sqrt(D)
        params[f"relw{l}"] = rng.uniform(-.05, .05, R)
        params[f"Wa{l}"] = rng.standard_normal((D, R)) / np.sqrt(D)
        params[f"ba{l}"] = rng.standard_normal(R) * 0.1
    params["rel"] = rng.standard_normal((R, D))
    params = {k: v.astype(np.float32) for k, v in params.items()}
    eng = Engine(N, R, D, cuda, gemm="bf16x3")
    assert eng.fuse_tail_head and eng.features == "f32"
    P, G = FlatParams(N, R, D, cuda), FlatParams(N, R, D, cuda)
    P.load(params)
    adj = eng.adjacency(get_adj_mats(pos, N, R))
    tri = np.concatenate([pos, neg])
    ed = eng.edges(tri, np.concatenate([np.ones(len(pos)), np.zeros(len(neg))]))
    ws = eng.workspace(ed.T, True)
    calls = {"tail_seg_reduce_head": 0, "head_dz": 0, "head_bwd_node": 0, "tail_seg_reduce": 0}
    for name in calls:
        def counted(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    top_dAE = []
    batched = ops.rowgemm_batched

    def snap(entries):
        batched(entries)
        out, kw = entries[0][2], entries[0][3]
        if out.data_ptr() == ws.dAE[0].data_ptr() and not kw.get("accumulate"):     # the top layer: dAE_r = dP_r K_r^T
            top_dAE.append(ws.dAE.clone())
    monkeypatch.setattr(ops, "rowgemm_batched", snap)
    runs = []
    for flag in (True, False):
        eng.fuse_tail_head = flag
        before = dict(calls)
        loss_sum, p = eng.loss_and_grads(P, G, adj, ed)
        torch.cuda.synchronize()
        used = {k: calls[k] - before[k] for k in calls}
        assert used == ({"tail_seg_reduce_head": 3, "head_dz": 3, "head_bwd_node": 0, "tail_seg_reduce": 0} if flag else
                        {"tail_seg_reduce_head": 0, "head_dz": 0, "head_bwd_node": 3, "tail_seg_reduce": 3}), used
        runs.append(dict(loss=loss_sum.clone(), p=p.cpu().numpy(), g=G.to_numpy()))
    f, u = runs
    assert torch.equal(f["loss"], u["loss"])
    assert np.array_equal(f["p"], u["p"])
    assert np.array_equal(f["g"]["K3"], u["g"]["K3"]), "K3 = AE^T dP at the top layer: dP must be bitwise"
    assert len(top_dAE) == 2 and torch.equal(top_dAE[0], top_dAE[1]), "top-layer dAE = dP K^T: dP must be bitwise"
    ref_loss, ref_scores, ref_grads = train_step_grads(params, pos, neg, get_adj_coo(pos, N, R), N)
    loss = u["loss"].item() / len(tri)
    assert abs(loss - ref_loss) <= 1e-5 * ref_loss
    np.testing.assert_allclose(u["p"], ref_scores, rtol=0, atol=1e-5)
    for k, g in ref_grads.items():
        err, scale = np.abs(u["g"][k].astype(np.float64) - g).max(), np.abs(g).max()
        print(f"GRAD {k}: unfused max err {err:.3e}, fused vs unfused {np.abs(f['g'][k] - u['g'][k]).max():.3e}, "
              f"max|g| {scale:.3e}")
        assert err <= 2e-4 * scale + 1e-30, f"grad {k}: max err {err:.3e} vs max|g| {scale:.3e}"
