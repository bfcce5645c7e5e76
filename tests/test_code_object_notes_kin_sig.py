"""What the structure instantiations of k_kin_reg / k_kin_reg_f32 look like to the hardware (no GPU needed; the metadata notes of the gfx950 code
objects inside librtbhip.so, read as tests/test_code_object_notes.py reads them -- notes only, no instruction text).

The general fused fkine + Jacobian kernel runs three waves per SIMD (RTB_REG_WAVES: at most 168 VGPRs) with its state in registers; an instantiation
for a robot's constants (Panda ETS, Panda URDF, UR: T+J, T only, J only, packed; fp64 and float32 rows) does less work per wave and must not pay for it
with occupancy: no private (scratch) segment, no spilled registers, at most 168 VGPRs."""
import os
import re

import pytest

from test_code_object_notes import LLVM, _kernels

SIGS = {"panda_ets": (7, 9265531810339127745), "panda_urdf": (7, 9265109580693144001), "ur": (6, 9223656143355924545)}


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="ROCm llvm tools not found")
def test_kin_reg_signature_instantiations_keep_three_waves_and_no_scratch(tmp_path):
    import __graft_entry__ as g
    g.build_lib()
    ks = _kernels(str(tmp_path))
    for name, (nj, sig) in SIGS.items():
        mine = {n: v for n, v in ks.items() if re.search(r"(9k_kin_reg|13k_kin_reg_f32)ILi%dELb[01]ELb[01]ELb[01]ELy%dEE" % (nj, sig), n)}
        forms = {re.search(r"(k_kin_reg(?:_f32)?)ILi\dE(Lb[01]ELb[01]ELb[01])", n).groups() for n in mine}
        want = {(k, f) for k in ("k_kin_reg", "k_kin_reg_f32") for f in ("Lb1ELb1ELb0", "Lb1ELb0ELb0", "Lb0ELb1ELb0", "Lb1ELb1ELb1")}      # T+J, T, J, packed
        assert forms == want, (name, sorted(forms))
        bad = {n[:80]: v for n, v in mine.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"] or v["vgpr_count"] > 168}
        assert not bad, (name, bad)
