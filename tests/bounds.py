"""Helpers shared by the per-element-bound test modules (test_gpu_step_kernels.py, test_gpu_mfma_gemms.py): the fp32
rounding unit and gamma_k, the elementwise bar with its report, and NaN-guarded output buffers."""
import torch

F32 = torch.float32
U = 2.0 ** -24
NAN = float("nan")


def gam(k):
    """gamma_k = k u / (1 - k u): the relative error of k successive roundings (k a number or a tensor)."""
    ku = k * U
    return ku / (1 - ku)


def _idx(flat, shape):
    out = []
    for s in reversed(shape):
        out.append(flat % s)
        flat //= s
    return tuple(reversed(out))


def worst_ratio(got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def rejects(cand, ref, bound):
    """True if the bar refuses `cand`: some element is farther from the reference than its bound."""
    return bool(((cand.double() - ref).abs() > bound).any())


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound ELEMENTWISE (ref, bound: fp64 CPU tensors from the reference alone).  A non-finite
    element of `got` (a NaN sentinel that was never overwritten) fails.  Reports the worst element."""
    g = got.detach().cpu().double()
    ref, bound = ref.cpu().double(), bound.cpu().double().expand_as(ref)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{what}: reference not finite"
    bad = ~torch.isfinite(g)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} element(s) not written / not finite, first at "
                             f"{_idx(i, g.shape)}: {float(g.flatten()[i])}")
    err = (g - ref).abs()
    ratio = worst_ratio(g, ref, bound)
    print(f"BOUND {what}: worst |err| / bound = {ratio:.3g}  (max |ref| {float(ref.abs().max()) if ref.numel() else 0:.3g})")
    over = err > bound
    if over.any():
        i = int(torch.where(over, err - bound, torch.full_like(err, -1.0)).flatten().argmax())
        at = _idx(i, g.shape)
        raise AssertionError(
            f"{what}: |got - ref| > bound at {at}: got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, "
            f"err {float(err.flatten()[i]):.3e}, bound {float(bound.flatten()[i]):.3e}; "
            f"{int(over.sum())} of {g.numel()} elements out of bound")
    return ratio


def guarded(dev, n, *rest, fill=NAN):
    """An output of n rows (or n elements) allocated one row larger and prefilled with a sentinel: (whole, owned)."""
    whole = torch.full((n + 1, *rest), fill, device=dev, dtype=F32)
    return whole, whole[:n]


def guard_intact(whole, what):
    g = whole[-1]
    assert bool(torch.isnan(g).all()), f"{what}: guard past the output was written"
