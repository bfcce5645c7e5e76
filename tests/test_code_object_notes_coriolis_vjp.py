"""What the Coriolis-matrix adjoint kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_coriolis_vjp<NJ, MDH> and k_tree_coriolis_vjp<NG> keep the two-field tape -- 18 doubles per link, 24 per group -- its sine, cosine and partial
angle adjoint, and the 2 n accumulators of gq and gqd in registers across the passes (csrc/coriolis_vjp_kernels.hip,
csrc/tree_coriolis_vjp_kernels.hip) and are built for one wave per SIMD.  Every compile-time instantiation that exists must do so without a private
(scratch) segment, without spilled vector registers and within the 512 registers of a lane; the set that exists holds at least NJ = 1..7 in both DH
conventions (Panda is 7) and NG = 1..6 (UR5 is 6).  The run-time-n kernels keep their tapes in private memory by design and are exempt."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_coriolis_vjp_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    dh, tree = {}, {}
    for n, v in ks.items():
        m = re.search(r"14k_coriolis_vjpILi(\d+)ELb([01])EE", n)
        if m:
            dh[(int(m.group(1)), int(m.group(2)))] = v
        m = re.search(r"19k_tree_coriolis_vjpILi(\d+)EE", n)
        if m:
            tree[int(m.group(1))] = v
    assert set(dh) >= {(nj, mdh) for nj in range(1, 8) for mdh in (0, 1)}, sorted(dh)
    assert set(tree) >= set(range(1, 7)), sorted(tree)
    for key in sorted(dh):
        print("k_coriolis_vjp<NJ=%d, MDH=%d>: %r" % (key + (dh[key],)))
    for key in sorted(tree):
        print("k_tree_coriolis_vjp<NG=%d>: %r" % (key, tree[key]))
    both = dict(dh)
    both.update({("tree", k): v for k, v in tree.items()})
    bad = {k: v for k, v in both.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in both.values())
    assert sum(1 for n in ks if "17k_coriolis_vjp_rt" in n) == 2 and sum(1 for n in ks if "22k_tree_coriolis_vjp_rt" in n) == 1
