"""What the resolved-rate kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside librtbhip.so,
read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_rrmc<NJ> keeps the joint vector, the 6 NJ entries of the finished Jacobian, the error, the system matrix and the solve in registers across a
loop of up to `steps` iterations (csrc/rrmc_kernels.hip, csrc/rrmc_device.h).  Every compile-time instantiation, NJ = 1..10, is held to what
tests/test_code_object_notes_ik_vjp.py holds k_ik_vjp to: no private (scratch) segment, no spilled registers, inside the budget of two waves per
SIMD (256 VGPRs).  DESIGN.md section 4.19 lists the figures."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_rrmc_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    mine = {}
    for n, v in ks.items():
        m = re.search(r"6k_rrmcILi(\d+)EE", n)
        if m:
            mine[int(m.group(1))] = v
    assert set(mine) == set(range(1, 11)), sorted(mine)
    for key in sorted(mine):
        print("k_rrmc<NJ=%d>: %r" % (key, mine[key]))
    bad = {k: v for k, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 256 for v in mine.values())          # two waves per SIMD
