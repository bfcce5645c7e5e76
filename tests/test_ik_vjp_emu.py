"""The implicit-function adjoint of the inverse kinematics on the CPU (no GPU needed): the lane body and the tile fill / flush phases of
k_ik_vjp / k_ik_vjp_any (csrc/ikgrad_device.h, csrc/kin_vjp.h, csrc/vjp_tile.h) compiled host-side by this test
(tests/emu_ik_vjp/emu_ik_vjp.cpp, linked against tests/emu/libemu.so for the chain compiler and the replayed jacob0) and held against the oracle
of tests/ik_vjp_cases.py -- oracle.jacob0 and numpy.linalg.solve -- at its bound, 1e-9 of the row's largest reference magnitude.  The device runs
the same source through another compiler: tests/test_ik_vjp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import ik_vjp_cases as cases

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_ik_vjp", "emu_ik_vjp.cpp")
SO = os.path.join(ROOT, "tests", "emu_ik_vjp", "libemu_ik_vjp.so")
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32
N = 70          # a full tile and a ragged one; the run-time-n form's rounds of 25 .. 64 rows end inside both


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the chain compiler, the registry and emu_kin (built if stale)
    import __graft_entry__ as g
    digest = g.source_digest(emu_harness._deps() + [SRC])
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        emu_dir = os.path.dirname(emu_harness.EMU_SO)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include"),
                               "-shared", SRC, "-o", SO, "-L" + emu_dir, "-l:libemu.so", "-Wl,-rpath," + emu_dir])
        open(stamp, "w").write(digest)
    so = C.CDLL(SO)
    so.emu_ik_vjp.argtypes = [_u64, _vp, _i64, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _i32]
    so.emu_pose_pullback.argtypes, so.emu_pose_pullback.restype = [_vp, _vp, _i64, _vp], None
    assert base is not None
    return so


def _run(lib, ets, q, Tep, gq, mask, damping, success=None, want=(True, True), force_rt=False, fill=np.nan):
    """-> [gTep (N, 4, 4), gtwist (N, 6)]; an output not wanted is handed over as NULL and comes back as the untouched buffer"""
    p = emu_harness._p
    h = emu_harness.chain_handle(ets)
    q, Tep, gq = (np.ascontiguousarray(x, dtype=np.float64) for x in (q, Tep, gq))
    we = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
    ok = None if success is None else np.ascontiguousarray(success, dtype=np.int32)
    n = q.shape[0]
    gT, tw = np.full((n, 4, 4), fill), np.full((n, 6), fill)
    assert lib.emu_ik_vjp(h, p(q), n, p(Tep), p(ok), p(we), float(damping), p(gq), p(gT) if want[0] else None, p(tw) if want[1] else None, int(force_rt)) == 0
    return gT, tw


def _tiled(name, mask_name):
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mask_name)
    t = lambda a: cases.tiled(a, N)
    return ets, t(q), t(Tep), t(gq), mask, damping, t(tw), t(gT)


def test_the_cases_are_what_they_claim(lib):
    assert [cases.model(n).n for n in cases.REG] == list(range(1, 11)) and [cases.model(n).n for n in cases.ANY] == [11, 16, 32]
    assert cases.model("panda").n == 7 and cases.model("UR5").n == 6 and cases.model("poe").n == 6
    pf = list(cases.model("prisflip").ets.joints())
    assert any(not e.isrotation for e in pf) and any(e.isflip for e in pf) and len(pf) == 7
    assert all(cases.model(n).ets.q_width == cases.model(n).n for n in cases.ALL)
    for name in cases.ALL:
        n = cases.model(name).n
        for mk, (mask, damping) in cases.masks_of(n).items():
            assert len(cases.used_rows(mask)) <= n and (damping == 0.1) == (n < 6)
        if n >= 6:
            q, Tep, gq, J, draws, replaced = cases.inputs(name)
            print("ik_vjp case %s: %d of %d draws replaced (cond > 1e4)" % (name, replaced, draws))
            assert 3 * replaced <= draws
            for mask in (None, cases.TRANS):
                Ja = J[:, cases.used_rows(mask)]
                assert np.linalg.cond(Ja @ Ja.transpose(0, 2, 1)).max() <= cases.COND_MAX
    assert set(cases.every_case()) == {(name, mk) for name in cases.ALL for mk in cases.masks_of(cases.model(name).n)}


@pytest.mark.parametrize("name,mask_name", cases.every_case())
def test_lane_body_equals_the_oracle(lib, name, mask_name):
    ets, q, Tep, gq, mask, damping, tw, gT = _tiled(name, mask_name)
    got_T, got_tw = _run(lib, ets, q, Tep, gq, mask, damping)
    e_tw, e_T = cases.row_error(got_tw, tw), cases.row_error(got_T, gT)
    print("ik_vjp lane %s/%s (n = %d): gtwist %.3e, gTep %.3e of the row's |ref|max" % (name, mask_name, ets.n, e_tw, e_T))
    assert e_tw <= cases.BOUND and e_T <= cases.BOUND
    unused = [r for r in range(6) if r not in cases.used_rows(mask)]
    assert not got_tw[:, unused].any() and not got_T[:, 3, :].any()
    other = cases.same_answer(mask_name)
    if other:                                    # the positive weights drop out: the reference of the unit mask, and the unit mask's own bits
        ref_tw = cases.tiled(cases.case(name, other)[6], N)
        assert cases.row_error(got_tw, ref_tw) <= cases.BOUND
        assert np.array_equal(got_tw, _run(lib, ets, q, Tep, gq, cases.case(name, other)[4], damping)[1])


@pytest.mark.parametrize("name,mask_name", [c for c in cases.every_case() if c[0] in ("n1", "n3", "n5", "n6", "n10", "panda", "UR5", "prisflip", "poe")])
def test_run_time_n_form_on_the_register_forms_chains(lib, name, mask_name):
    """k_ik_vjp_any's body (the Jacobian read from the LDS row) on chains the register tile also serves; n11, n16 and n32 take it in
    test_lane_body_equals_the_oracle"""
    ets, q, Tep, gq, mask, damping, tw, gT = _tiled(name, mask_name)
    got_T, got_tw = _run(lib, ets, q, Tep, gq, mask, damping, force_rt=True)
    e_tw, e_T = cases.row_error(got_tw, tw), cases.row_error(got_T, gT)
    print("ik_vjp run-time-n %s/%s: gtwist %.3e, gTep %.3e" % (name, mask_name, e_tw, e_T))
    assert e_tw <= cases.BOUND and e_T <= cases.BOUND


@pytest.mark.parametrize("name", ["n2", "panda", "n11"])
def test_rows_without_success_are_zeros(lib, name):
    mk = sorted(cases.masks_of(cases.model(name).n))[0]
    ets, q, Tep, gq, mask, damping, tw, gT = _tiled(name, mk)
    ok = (np.arange(N) % 2).astype(np.int32)
    all_T, all_tw = _run(lib, ets, q, Tep, gq, mask, damping)
    got_T, got_tw = _run(lib, ets, q, Tep, gq, mask, damping, success=ok)
    assert not got_T[ok == 0].any() and not got_tw[ok == 0].any()
    assert np.array_equal(got_T[ok == 1], all_T[ok == 1]) and np.array_equal(got_tw[ok == 1], all_tw[ok == 1])
    # a row that is not a solution may hold anything: its zeros are selected, not multiplied
    q2 = np.array(q)
    q2[ok == 0] = np.nan
    got_T, got_tw = _run(lib, ets, q2, Tep, gq, mask, damping, success=ok)
    assert not got_T[ok == 0].any() and not got_tw[ok == 0].any() and np.isfinite(got_tw).all()


@pytest.mark.parametrize("name", ["n4", "panda", "n16"])
def test_a_null_output_is_not_written(lib, name):
    mk = sorted(cases.masks_of(cases.model(name).n))[0]
    ets, q, Tep, gq, mask, damping, tw, gT = _tiled(name, mk)
    both = _run(lib, ets, q, Tep, gq, mask, damping)
    only_T = _run(lib, ets, q, Tep, gq, mask, damping, want=(True, False), fill=7.0)
    only_tw = _run(lib, ets, q, Tep, gq, mask, damping, want=(False, True), fill=7.0)
    assert np.array_equal(only_T[0], both[0]) and (only_T[1] == 7.0).all()
    assert np.array_equal(only_tw[1], both[1]) and (only_tw[0] == 7.0).all()


@pytest.mark.parametrize("name,mask_name", cases.every_case())
def test_the_pose_pullback_of_gTep_is_the_twist(lib, name, mask_name):
    """gTep is the tangent-space gradient at Tep: the project's own vjp_pose_pullback (csrc/kin_vjp.h) returns the twist from it, to 1e-14 of the
    row's largest magnitude (six rounded terms on a rotation the oracle left orthonormal to an ulp or two)"""
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mask_name)
    got_T, got_tw = _run(lib, ets, q, Tep, gq, mask, damping)
    back = np.full(got_tw.shape, np.nan)
    Tc, Gc = np.ascontiguousarray(Tep), np.ascontiguousarray(got_T)
    lib.emu_pose_pullback(emu_harness._p(Tc), emu_harness._p(Gc), Tc.shape[0], emu_harness._p(back))
    err = cases.row_error(back, got_tw)
    print("ik_vjp pullback %s/%s: %.3e" % (name, mask_name, err))
    assert err <= 1e-14
    assert cases.row_error(cases.pullback(Tc, Gc), got_tw) <= 1e-14          # and the NumPy restatement of the same contraction


@pytest.mark.parametrize("name,mask_name", [c for c in cases.every_case() if cases.masks_of(cases.model(c[0]).n)[c[1]][1] == 0.0])
def test_the_closed_form_is_the_minimum_norm_one(lib, name, mask_name):
    """undamped: y_a = pinv(J_a)^T gq -- the adjoint of dq = pinv(J_a) nu_a, the minimum-norm solution of J_a dq = nu_a"""
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mask_name)
    J = cases.inputs(name)[3]
    rows = cases.used_rows(mask)
    ref = np.zeros(tw.shape)
    for i in range(J.shape[0]):
        ref[i, rows] = np.linalg.pinv(J[i][rows]).T @ gq[i]
    got = _run(lib, ets, q, Tep, gq, mask, damping)[1]
    err = cases.row_error(got, ref)
    print("ik_vjp minimum norm %s/%s: %.3e" % (name, mask_name, err))
    assert err <= cases.BOUND


def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include ikgrad_kernels.hip: the launcher is a
    weak reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case("n2", "short")
    p = emu_harness._p
    h = emu_harness.chain_handle(ets)
    q, Tep, gq, out = np.array(q), np.array(Tep), np.array(gq), np.zeros((q.shape[0], 16))
    we = np.ascontiguousarray(mask, dtype=np.float64)
    proto = C.CFUNCTYPE(C.c_int, _u64, _vp, _i64, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp)      # a prototype of this test's own
    call = proto(("rtbhip_ik_vjp", emu))
    assert call(h, p(q), q.shape[0], p(Tep), None, p(we), 0.1, p(gq), p(out), None, None) == -1
    assert emu.rtbhip_last_error().decode() == "ik_vjp: not built into this library"
    assert call(h, p(q), 0, p(Tep), None, p(we), 0.1, p(gq), p(out), None, None) == 0 and not out.any()
