"""What the all-frame adjoint kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_frames_vjp<NJ> keeps seven doubles per joint, the walk's pose, the running wrench sums and one chunk of G in flight in registers
(csrc/frames_vjp_kernels.hip).  Every compile-time instantiation, NJ = 1..8, must do so without a private (scratch) segment and without spilled
registers.  The run-time-n kernel k_frames_vjp_rt keeps its per-joint state in private memory by design and is exempt."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_frames_vjp_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    mine = {}
    for n, v in ks.items():
        m = re.search(r"12k_frames_vjpILi(\d)EE", n)
        if m:
            mine[int(m.group(1))] = v
    assert set(mine) == set(range(1, 9)), sorted(mine)
    for key in sorted(mine):
        print("k_frames_vjp<NJ=%d>: %r" % (key, mine[key]))
    bad = {k: v for k, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in mine.values())
    assert sum(1 for n in ks if "15k_frames_vjp_rt" in n) == 1
