"""Bitwise A/B of the four fused explainer routes between two builds of the library (profiles/r21/).

usage: IDDGCN_LIB=lib.so python tools/explainers_ab.py dump OUT.npz     (a fresh process per dump, one at a time)
       python tools/explainers_ab.py compare A.npz B.npz                (exits 1 on any difference)

dump runs fidelity_curves, counterfactual_batched (three modes, with occlusion), integrated_gradients_batched (steps 1,
32, 33, 100: one chunk, a full chunk, a chunk of one, four chunks) and mask_explainer_batched (with and without target
ratios, 0, 1 and 5 epochs; also the kernel's m, v and steps afterwards) on seeded inputs the tests already have:
tests/ref_fidelity.small_case at (d, R) = (32, 1), (32, 3), (64, 2), (64, 8); the large-degree graph at D = 64 and 32
(segments of 601 and 666 candidates: past the E rows the tile kernels stage, and past one pass of the mask kernel);
fold 4's 288 test triples with the bundled weights when tests/golden has them.  Every returned array is saved.  Then,
on the last case, each fused call alone 5 + 40 times, no layered route in between: the device-event time around its
launches, median and minimum, one JSON line.
"""
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SMALL = ((32, 1), (32, 3), (64, 2), (64, 8))
IG_STEPS = (1, 32, 33, 100)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def flatten(prefix, x, out):
    """Every array of a nested dict / list / tuple result, under a path name."""
    if isinstance(x, dict):
        for k, v in x.items():
            flatten(f"{prefix}/{k}", v, out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            flatten(f"{prefix}/{i}", v, out)
    elif x is not None:
        out[prefix] = np.asarray(x)


def cases():
    """(name, model, adjacency triples, queries, explanations, mask init or None)"""
    from iddgcn_amd import _lib as L
    from iddgcn_amd import explain as X
    from iddgcn_amd import get_IDDGCN_Model
    from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
    from tests import ref_fidelity as RF
    from tests.test_mask_batched_host import fold4_case
    from tests.test_mask_grads_host import large_degree_case
    for d, R in SMALL:
        N, tri, params, q = RF.small_case(d, R)
        host = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
        yield f"small_d{d}_R{R}", RF.model_with(params, N, R, d), tri, q, RF.mixed_explanations(host, q), None
    for d in (64, 32):
        N, R, tri, q, init, params = large_degree_case(d)
        host = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
        preds = X.random_explanations(host, q, L.TOPK_MAX, seed=5)
        yield f"large_d{d}", RF.model_with(params, N, R, d), tri, q, preds, init
    if os.path.exists(os.path.join(GOLDEN, "weights_fold4.npz")):
        adjacency, test = fold4_case(lambda n: dict(np.load(os.path.join(GOLDEN, n))))
        model = get_IDDGCN_Model(845, 4, 64, 64, 123, None, 0, 4)
        model.load_weights(os.path.join(GOLDEN, "weights_fold4.npz"))
        preds = np.load(os.path.join(GOLDEN, "explain_fold4.npz"))["explaine_preds"]
        yield "fold4", model, adjacency, test, preds, None


def calls(model, tri, q, preds, init, state):
    """{name: f(stats) -> result} of the fused calls on one case; ``state`` receives the mask kernel's m, v, steps."""
    from iddgcn_amd import explain as X
    from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
    from tests.test_mask_grads_host import ratios_of
    N, R = model.num_entities, model.num_relations
    qptr = X.mask_candidates(DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu"), q)[0]
    qm = q[np.diff(qptr) > 0]                      # the relation-ratio loss refuses a triple with no candidate
    out = {"fidelity": lambda st: X.fidelity_curves(model, tri, q, preds, fused=True, stats=st)}
    for mode in ("flip", "lower", "raise"):
        out[f"counterfactual_{mode}"] = lambda st, mode=mode: X.counterfactual_batched(
            model, tri, q, toward=mode, fused=True, return_occlusion=True, stats=st)
    for m in IG_STEPS:
        out[f"ig_{m}"] = lambda st, m=m: X.integrated_gradients_batched(
            model, tri, q, steps=m, fused=True, return_attributions=True, stats=st)
    for ratios in (None, ratios_of("iddgcn", R)):
        for ep in (0, 1, 5):
            def mask(st, ratios=ratios, ep=ep):
                try:
                    res = X.mask_explainer_batched(model, tri, q if ratios is None else qm, num_epochs=ep,
                                                   init_value=init, target_ratios=ratios, return_masks=True, stats=st)
                except X.IddgcnError as e:         # 0 epochs: the C entry refuses the empty alpha; the refusal is kept
                    return {"refused": str(e)}
                return {"result": res, "state": dict(state)}
            out[f"mask_{'ratios' if ratios else 'plain'}_ep{ep}"] = mask
    return out


def dump(path):
    import torch

    from iddgcn_amd import ops
    state, inner = {}, ops.mask_explain

    def mask_explain(*a, **kw):                    # the kernel's per-entry state is local to mask_explainer_batched
        inner(*a, **kw)
        bound = inspect.signature(inner).bind(*a, **kw).arguments
        state.update({k: bound[k].cpu().numpy() for k in ("m", "v", "steps")})
    ops.mask_explain = mask_explain
    arrays, last = {}, None
    for name, *case in cases():
        last = calls(*case, state)
        for cname, f in last.items():
            flatten(f"{name}/{cname}", f(None), arrays)
        print(f"{name}: {len(arrays)} arrays so far", flush=True)
    np.savez_compressed(path, **arrays)
    timings = {}
    for cname in ("fidelity", "counterfactual_flip", "ig_32", "mask_plain_ep5"):
        ms = []
        for i in range(45):
            st = {}
            last[cname](st)
            torch.cuda.synchronize()
            if i >= 5:
                ms.append(st["launch_events"][0].elapsed_time(st["launch_events"][1]))
        timings[cname] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms))}
    lib = os.path.basename(os.environ.get("IDDGCN_LIB", "tree"))
    print(json.dumps({"lib": lib, "case": name, "arrays": len(arrays),
                      "elements": int(sum(a.size for a in arrays.values())), "device_event_ms": timings}), flush=True)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    bad = [n for n in names if n not in a.files or n not in b.files or a[n].dtype != b[n].dtype or
           a[n].shape != b[n].shape or a[n].tobytes() != b[n].tobytes()]
    for n in bad[:20]:
        print("differs:", n)
    print(f"{len(names)} arrays, {sum(a[n].size for n in a.files)} elements, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
