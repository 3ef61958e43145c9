"""The fused sigma' + dS pass (sigma_tn_b3_kernel) runs three waves per SIMD: a 768-thread workgroup, at most 168 VGPRs
(512 / 3, in granules of 8), no scratch, and LDS that leaves one workgroup per CU.  Read from the built library's
code-object metadata (as tools/kernel_regs.py prints it), so a later change cannot fall back to two waves per SIMD, or
start spilling, without a test saying so.  No GPU needed."""
import os
import re

import pytest

from tools import kernel_regs

INT_KEYS = (".max_flat_workgroup_size", ".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
            ".private_segment_fixed_size", ".group_segment_fixed_size")


def _metadata(substr):
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "llvm-readelf")):
        pytest.skip("no ROCm llvm tools")
    from iddgcn_amd import _lib
    found = []
    for item in re.split(r"\n\s+- \.agpr_count", kernel_regs.notes(_lib.LIB_PATH)):
        m = re.search(r"\.name:\s*(\S+)", item)
        if m and substr in m.group(1) and not m.group(1).endswith(".kd"):
            item = ".agpr_count" + item
            found.append({k: int(re.search(re.escape(k) + r":\s*(\d+)", item).group(1)) for k in INT_KEYS})
    return found


def test_sigma_tn_b3_runs_three_waves_per_simd():
    found = _metadata("sigma_tn_b3_kernel")
    assert len(found) == 1, found
    md = found[0]
    assert md[".max_flat_workgroup_size"] == 768, md        # twelve waves: eight sigma' waves and four TN waves
    assert md[".vgpr_count"] <= 168 and md[".agpr_count"] == 0, md
    # no VGPR goes to memory and the kernel has no scratch at all (SGPRs parked in lanes of a VGPR, .sgpr_spill_count,
    # cost no memory access and are inside the VGPR count above)
    assert md[".vgpr_spill_count"] == 0 and md[".private_segment_fixed_size"] == 0, md
    assert md[".group_segment_fixed_size"] <= 163840, md
