"""Helpers shared by the per-element-bound test modules (test_gpu_step_kernels.py, test_gpu_mfma_gemms.py,
test_gpu_config5_kernels.py): the fp32 rounding unit and gamma_k, the elementwise bar with its report, NaN-guarded output
buffers, the interval bar of a value stored as bf16, and the per-query bar of the explainer gradients (query_bar:
test_mask_grads_host.py, test_gpu_mask_grads.py)."""
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


def query_bar(ref64, ref32, floor=1e-5):
    """The per-query bar of the explainer gradients (tests/test_gpu_explain_batched.py's within_bar): max(4 x the
    fp32 reference's own deviation, floor x max|ref64|), maxima over one query's values (numpy, from the reference
    alone)."""
    if not ref64.size:
        return 0.0
    return float(max(4 * abs(ref32 - ref64).max(), floor * abs(ref64).max()))


def guarded(dev, n, *rest, fill=NAN, dtype=F32):
    """An output of n rows (or n elements) allocated one row larger and prefilled with a sentinel: (whole, owned)."""
    whole = torch.full((n + 1, *rest), fill, device=dev, dtype=dtype)
    return whole, whole[:n]


# ---- values stored as bf16 --------------------------------------------------------------------------------------
BF16 = torch.bfloat16


def to_bf16(x):
    """fp64 -> fp32 -> bf16, both round-to-nearest-even and both monotone, back as fp64."""
    return x.float().to(BF16).double()


def bf16_interval(z, b):
    """The bf16 values a kernel may store when its fp32 value y before the rounding satisfies |y - z| <= b (z, b: fp64
    from the reference alone): rounding is monotone, so the stored value lies in [bf16(f32(z - b)), bf16(f32(z + b))].
    Returns (lo, hi) as fp64; for most elements lo == hi and the bar is bitwise."""
    z, b = z.double(), b.double().expand_as(z)
    return to_bf16(z - b), to_bf16(z + b)


def ambiguous_share(lo, hi):
    """The share of elements whose interval holds more than one bf16 value."""
    return float((lo != hi).double().mean()) if lo.numel() else 0.0


def outside_interval(cand, lo, hi):
    """Elementwise: cand (any float type) is not finite or not within [lo, hi]."""
    c = cand.detach().cpu().double()
    return ~torch.isfinite(c) | (c < lo) | (c > hi)


def rejects_interval(cand, lo, hi):
    return bool(outside_interval(cand, lo, hi).any())


def assert_bf16_interval(got, z, b, what, max_ambiguous=0.05):
    """got (stored bf16) within bf16_interval(z, b) ELEMENTWISE; a NaN sentinel fails.  The bar may hold more than one
    bf16 value on at most max_ambiguous of the elements (a condition on the reference alone).  Reports the ambiguous
    share and the worst distance from bf16(z) in bf16 units in the last place.  Returns the ambiguous share."""
    g = got.detach().cpu().double()
    z = z.cpu().double()
    assert g.shape == z.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(z.shape)}"
    assert bool(torch.isfinite(z).all()), f"{what}: reference not finite"
    lo, hi = bf16_interval(z, b)
    amb = ambiguous_share(lo, hi)
    bad = ~torch.isfinite(g)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} element(s) not written / not finite, first at {_idx(i, g.shape)}")
    mid = to_bf16(z)
    ulp = torch.where(mid != 0, 2.0 ** (torch.floor(torch.log2(mid.abs().clamp_min(1e-300))) - 7), torch.ones_like(mid))
    off = float(((g - mid).abs() / ulp).max()) if g.numel() else 0.0
    out = (g < lo) | (g > hi)
    print(f"BOUND {what}: {int(out.sum())} of {g.numel()} outside the bf16 interval; interval ambiguous on "
          f"{100 * amb:.2f}% of the elements; worst |got - bf16(ref)| = {off:.3g} bf16 ulp")
    assert amb <= max_ambiguous, f"{what}: the bar is ambiguous on {100 * amb:.1f}% of the elements"
    if out.any():
        i = int(out.flatten().nonzero()[0])
        raise AssertionError(
            f"{what}: stored bf16 outside [bf16(ref - bound), bf16(ref + bound)] at {_idx(i, g.shape)}: got "
            f"{float(g.flatten()[i])!r}, interval [{float(lo.flatten()[i])!r}, {float(hi.flatten()[i])!r}], ref "
            f"{float(z.flatten()[i])!r}; {int(out.sum())} of {g.numel()} elements outside")
    return amb


def guard_intact(whole, what):
    g = whole[-1]
    assert bool(torch.isnan(g).all()), f"{what}: guard past the output was written"
