"""What the operational-space kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_opspace<NJ, MDH, ALLREV> and k_tree_opspace<NG> (csrc/opspace_kernels.hip, csrc/tree_opspace_kernels.hip, csrc/opspace_device.h) run the
recursion's passes and then a tail that holds two or three 6 x 6 matrices in registers.  J and M stay in the lane's LDS row, one wave per SIMD
(launch bound 1: up to 512 registers a lane).  Every instantiation -- the register forms of the tail, 1..8 joints, and the run-time-n form,
9..16 -- must do so without a private (scratch) segment and without spilled registers."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_opspace_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    dh, tree = {}, {}
    for n, v in ks.items():
        m = re.search(r"9k_opspaceILi(\d+)ELb([01])ELb([01])EE", n)
        if m:
            dh[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = v
        m = re.search(r"14k_tree_opspaceILi(\d+)EE", n)
        if m:
            tree[int(m.group(1))] = v
    assert set(dh) == {(n, a, b) for n in range(1, 17) for a in (0, 1) for b in (0, 1)}, sorted(dh)
    assert set(tree) == set(range(1, 17)), sorted(tree)
    for key in sorted(dh):
        print("k_opspace<NJ=%d, MDH=%d, ALLREV=%d>: %r" % (key + (dh[key],)))
    for key in sorted(tree):
        print("k_tree_opspace<NG=%d>: %r" % (key, tree[key]))
    every = list(dh.values()) + list(tree.values())
    bad = [v for v in every if v["private_segment_fixed_size"] or v["vgpr_spill_count"]]
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in every)                  # one wave per SIMD
