"""What the inverse-dynamics adjoint kernels look like to the hardware (no GPU needed; the metadata notes of the gfx950 code objects inside
librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

k_rne_vjp<NJ, MDH, S> keeps a tape of 15 doubles per link in registers (csrc/rne_vjp_kernels.hip) and is built for one wave per SIMD -- the whole
512-entry register file.  Every compile-time instantiation, NJ = 1..8 in both conventions and both storage types, must do so without a private
(scratch) segment and without spilled registers.  The run-time-n kernel k_rne_vjp_rt keeps its tape in private memory by design and is exempt."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_rne_vjp_instantiations_have_no_scratch_and_no_spills(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    mine = {}
    for n, v in ks.items():
        m = re.search(r"9k_rne_vjpILi(\d)ELb([01])E([df])E", n)
        if m:
            mine[(int(m.group(1)), int(m.group(2)), m.group(3))] = v
    assert set(mine) == {(nj, mdh, s) for nj in range(1, 9) for mdh in (0, 1) for s in "df"}, sorted(mine)
    for key in sorted(mine):
        print("k_rne_vjp<NJ=%d, MDH=%d, %s>: %r" % (key + (mine[key],)))
    bad = {k: v for k, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"]}
    assert not bad, bad
    assert all(v["vgpr_count"] <= 512 for v in mine.values())
    assert sum(1 for n in ks if "12k_rne_vjp_rt" in n) == 4
