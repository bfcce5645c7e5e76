"""What the reactive QP servo's kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_mmc<NJ> keeps the joint vector, the 6 NJ entries of the Jacobian, the gradient, the box, the 6 x 6 system and the QP's held set in registers
across two nested device-side loops (csrc/mmc_kernels.hip, csrc/mmc_device.h).  Every instantiation, NJ = 6..10: no private (scratch) segment,
no spilled VGPRs, at most 512 VGPRs (one wave per SIMD, where IK_QP's 9..12-joint kernels run); 6 and 7 joints are built for two waves per SIMD
and are held to 256.  DESIGN.md section 4.20 lists the figures."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels

TWO_WAVES = (6, 7)          # csrc/mmc_device.h: kMmcTwoWavesMax


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_mmc_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    mine = {}
    for n, v in ks.items():
        m = re.search(r"5k_mmcILi(\d+)EE", n)
        if m:
            mine[int(m.group(1))] = v
    assert set(mine) == set(range(6, 11)), sorted(mine)
    for key in sorted(mine):
        print("k_mmc<NJ=%d>: %r" % (key, mine[key]))
    bad = {k: v for k, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in mine.values())                     # at least one wave per SIMD
    assert all(mine[k]["vgpr_count"] <= 256 for k in TWO_WAVES)                   # two waves per SIMD
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robotics-toolbox-python_amd", "csrc", "mmc_device.h")).read()
    assert int(re.search(r"kMmcTwoWavesMax = (\d+);", src).group(1)) == max(TWO_WAVES)
