"""The HEAD form of the fp32 tail reduction (tail_seg_reduce_kernel<256, R, false, true>, iddgcn_tail_seg_reduce_head_f32)
keeps the waves per SIMD of the plain form <256, 2, false, false> it replaces at the headline shape: the kernel is bound
by rows in flight, the VGPR allocation granule is 8, so a few more live registers would cost a whole wave.  No VGPR
spill, no scratch.  Read from the built library's code-object metadata with the reader of
tests/test_sigma_tn_b3_codeobject.py.  No GPU needed."""
import pytest

from test_sigma_tn_b3_codeobject import _metadata

# Itanium mangling of the template arguments <256, R, false, HEAD>
PLAIN2 = "tail_seg_reduce_kernelILi256ELi2ELb0ELb0EE"
HEAD = {1: "tail_seg_reduce_kernelILi256ELi1ELb0ELb1EE", 2: "tail_seg_reduce_kernelILi256ELi2ELb0ELb1EE"}


def waves_per_simd(md):
    """gfx950: 512 VGPRs per SIMD lane (unified with AGPRs), allocated in granules of 8, at most 8 waves."""
    regs = -(-(md[".vgpr_count"] + md[".agpr_count"]) // 8) * 8
    return min(8, 512 // regs)


def _one(name):
    found = _metadata(name)
    assert len(found) == 1, (name, found)
    return found[0]


def test_waves_per_simd_formula():
    assert waves_per_simd({".vgpr_count": 76, ".agpr_count": 0}) == 6
    assert waves_per_simd({".vgpr_count": 80, ".agpr_count": 0}) == 6
    assert waves_per_simd({".vgpr_count": 81, ".agpr_count": 0}) == 5
    assert waves_per_simd({".vgpr_count": 128, ".agpr_count": 0}) == 4
    assert waves_per_simd({".vgpr_count": 24, ".agpr_count": 0}) == 8


@pytest.mark.parametrize("R", [1, 2])
def test_head_form_keeps_the_plain_forms_waves(R):
    plain, head = _one(PLAIN2), _one(HEAD[R])
    assert head[".agpr_count"] == 0 and plain[".agpr_count"] == 0, (plain, head)
    assert waves_per_simd(head) >= waves_per_simd(plain), (plain, head)
    assert head[".vgpr_spill_count"] == 0 and head[".private_segment_fixed_size"] == 0, head
    assert head[".group_segment_fixed_size"] == 0 and head[".max_flat_workgroup_size"] == 256, head
