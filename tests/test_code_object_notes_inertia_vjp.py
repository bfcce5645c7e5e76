"""What the inertia-matrix adjoint kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_inertia_vjp<NJ, MDH> and k_tree_inertia_vjp<NG> keep a tape of 12 doubles per link (group), its sine, cosine and partial angle adjoint, and the n
accumulators of gq in registers across the unit-acceleration passes (csrc/inertia_vjp_kernels.hip, csrc/tree_inertia_vjp_kernels.hip) and are built
for one wave per SIMD.  Every compile-time instantiation, NJ / NG = 1..8, both DH conventions, must do so without a private (scratch) segment and
without spilled vector registers.  The run-time-n kernels keep their tapes in private memory by design and are exempt."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_inertia_vjp_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    dh, tree = {}, {}
    for n, v in ks.items():
        m = re.search(r"13k_inertia_vjpILi(\d)ELb([01])EE", n)
        if m:
            dh[(int(m.group(1)), int(m.group(2)))] = v
        m = re.search(r"18k_tree_inertia_vjpILi(\d)EE", n)
        if m:
            tree[int(m.group(1))] = v
    assert set(dh) == {(nj, mdh) for nj in range(1, 9) for mdh in (0, 1)}, sorted(dh)
    assert set(tree) == set(range(1, 9)), sorted(tree)
    for key in sorted(dh):
        print("k_inertia_vjp<NJ=%d, MDH=%d>: %r" % (key + (dh[key],)))
    for key in sorted(tree):
        print("k_tree_inertia_vjp<NG=%d>: %r" % (key, tree[key]))
    both = dict(dh)
    both.update({("tree", k): v for k, v in tree.items()})
    bad = {k: v for k, v in both.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in both.values())
    assert sum(1 for n in ks if "16k_inertia_vjp_rt" in n) == 2 and sum(1 for n in ks if "21k_tree_inertia_vjp_rt" in n) == 1
