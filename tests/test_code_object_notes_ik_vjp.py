"""What the inverse-kinematics adjoint kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_ik_vjp<NJ> keeps the 6 NJ entries of the finished Jacobian, the triangle of J_a J_a^T + d^2 I and the solve in registers
(csrc/ikgrad_kernels.hip, csrc/ikgrad_device.h).  Every compile-time instantiation, NJ = 1..10, must do so without a private (scratch) segment
and without spilled registers, inside the budget of two waves per SIMD (256 VGPRs).  The run-time-n kernel k_ik_vjp_any reads its Jacobian from
LDS and is listed once."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_ik_vjp_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    mine = {}
    for n, v in ks.items():
        m = re.search(r"8k_ik_vjpILi(\d+)EE", n)
        if m:
            mine[int(m.group(1))] = v
    assert set(mine) == set(range(1, 11)), sorted(mine)
    for key in sorted(mine):
        print("k_ik_vjp<NJ=%d>: %r" % (key, mine[key]))
    bad = {k: v for k, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 256 for v in mine.values())          # two waves per SIMD
    rt = [v for n, v in ks.items() if "12k_ik_vjp_any" in n]
    assert len(rt) == 1
    print("k_ik_vjp_any: %r" % (rt[0],))
    assert not rt[0]["vgpr_spill_count"]
