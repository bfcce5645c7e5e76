"""The adjoint of the Newton-Euler recursion on the CPU (no GPU needed): the per-lane body of k_rne_vjp (csrc/rne_vjp_kernels.hip: rne_vjp_lane)
compiled host-side by this test (tests/emu_rne_vjp/emu_rne_vjp.cpp, linked against tests/emu/libemu.so for rtbhip_dyn_create and the link table)
and held against the oracle of tests/rne_vjp_cases.py -- Richardson differences of the compiled reference -- at rne's bound,
1e-9 max(1, |ref|max), plus the exact identity gqdd = (reference inertia rows) . gtau at the same bound.  The device runs the same source through
another compiler: tests/test_rne_vjp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import rne_vjp_cases as cases
import vjp_census_cases as census

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_rne_vjp", "emu_rne_vjp.cpp")
SO = os.path.join(ROOT, "tests", "emu_rne_vjp", "libemu_rne_vjp.so")
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the link-table compiler and registry (built if stale)
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
    so.emu_rne_vjp.argtypes = [_u64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32]
    assert base is not None
    return so


def _run(lib, rb, q, qd, qdd, g, gravity=None, fext=None, force_rt=False):
    p = emu_harness._p
    L = np.ascontiguousarray(rb.L24())
    h = _u64(0)
    assert emu_harness.lib().rtbhip_dyn_create(p(L), rb.n, int(rb.mdh), C.byref(h)) == 0
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    q, qd, qdd, g, fext = arr(q), arr(qd), arr(qdd), arr(g), arr(fext)
    gc = np.ascontiguousarray(rb._gravity_c(gravity))
    out = [np.full(q.shape, np.nan) for _ in range(3)]
    assert lib.emu_rne_vjp(h.value, p(q), p(qd), p(qdd), q.shape[0], p(gc), p(fext), p(g), p(out[0]), p(out[1]), p(out[2]), int(force_rt)) == 0
    return out


N = 24


@pytest.mark.parametrize("name", sorted(cases.ROBOTS))
def test_lane_body_equals_the_oracle(lib, name):
    rb, q, qd, qdd, g, gravity, fext, ref = cases.case(name, N)
    got = _run(lib, rb, q, qd, qdd, g)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        err = cases.rel_err(a, b)
        print("rne_vjp lane %s %s: rel err %.3e" % (name, what, err))
        assert err <= cases.BOUND, (name, what, err)
    assert cases.rel_err(got[2], cases.inertia_gqdd(rb, q, g)) <= cases.BOUND


CENSUS_DH = ["n4s", "n4m", "n6m", "n7s"] + sorted(census.STRUCTURED)          # register forms the zoo above leaves out; exact zeros and special angles


@pytest.mark.parametrize("name", CENSUS_DH)
def test_lane_body_equals_the_oracle_on_the_census_robots(lib, name):
    """the robots tests/vjp_census_cases.py adds for the device, where this driver instantiates their joint count: a host-side slip in those bodies
    fails without a GPU"""
    rb, q, qd, qdd, g, ref = census.rne_case(name)
    got = _run(lib, rb, q, qd, qdd, g)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        err = cases.rel_err(a, b)
        print("rne_vjp lane %s %s: rel err %.3e" % (name, what, err))
        assert err <= cases.BOUND, (name, what, err)
    assert cases.rel_err(got[2], cases.inertia_gqdd(rb, q, g)) <= cases.BOUND


@pytest.mark.parametrize("name", ["puma560", "panda", "n5s", "n5m"])
@pytest.mark.parametrize("variant", ["noqd", "noqdd", "gravity", "fext", "base"])
def test_lane_body_variants(lib, name, variant):
    rb, q, qd, qdd, g, gravity, fext, ref = cases.case(name, N, variant)
    got = _run(lib, rb, q, qd, qdd, g, gravity, fext)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        if b is not None:
            assert cases.rel_err(a, b) <= cases.BOUND, (name, variant, what, cases.rel_err(a, b))


@pytest.mark.parametrize("name", ["puma560", "panda", "n3s", "n8m"])
def test_run_time_n_form_agrees(lib, name):
    """the NJ = 0 body (private-memory tape, serves 9..32 joints on the device) on chains the compile-time body also serves"""
    rb, q, qd, qdd, g, gravity, fext, ref = cases.case(name, N)
    got = _run(lib, rb, q, qd, qdd, g, force_rt=True)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        assert cases.rel_err(a, b) <= cases.BOUND, (name, what, cases.rel_err(a, b))


def test_prismatic_chain_is_not_served(lib):
    from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH
    rb = DHRobot([RevoluteDH(a=0.3, m=1.0), PrismaticDH(alpha=0.5, m=1.0)])
    p = emu_harness._p
    L = np.ascontiguousarray(rb.L24())
    h = _u64(0)
    assert emu_harness.lib().rtbhip_dyn_create(p(L), rb.n, int(rb.mdh), C.byref(h)) == 0
    x = np.zeros((1, rb.n))
    assert lib.emu_rne_vjp(h.value, p(x), p(x), p(x), 1, p(np.zeros(3)), None, p(x), p(x.copy()), p(x.copy()), p(x.copy()), 0) == -2



def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include rne_vjp_kernels.hip: the launcher is a
    weak reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    rb = cases.robot("puma560")
    p = emu_harness._p
    L = np.ascontiguousarray(rb.L24())
    h = _u64(0)
    assert emu.rtbhip_dyn_create(p(L), rb.n, int(rb.mdh), C.byref(h)) == 0
    x, g = np.zeros((2, rb.n)), np.zeros(3)
    proto = C.CFUNCTYPE(C.c_int, _u64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp)       # a prototype of this test's own: the shared CDLL object is left as it is
    call = proto(("rtbhip_rne_vjp", emu))
    assert call(h.value, p(x), p(x), p(x), 2, p(g), None, p(x), p(x.copy()), None, None, 0, None) == -1
    assert emu.rtbhip_last_error().decode() == "rne_vjp: not built into this library"
