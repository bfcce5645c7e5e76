"""The adjoint of the link-tree Newton-Euler recursion on the CPU (no GPU needed): the per-lane body of k_tree_rne_vjp
(csrc/tree_rne_vjp_kernels.hip: tree_rne_vjp_lane) compiled host-side by this test (tests/emu_tree_rne_vjp/emu_tree_rne_vjp.cpp, linked against
tests/emu/libemu.so for rtbhip_tree_create and the group table) and held against the oracle of tests/tree_rne_vjp_cases.py -- Richardson
differences of the restated reference -- at 1e-9 max(1, |ref|max), plus the exact identity gqdd = (reference inertia rows) . gtau at the same
bound.  The device runs the same source through another compiler: tests/test_tree_rne_vjp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import tree_rne_vjp_cases as cases
import vjp_census_cases as census

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_tree_rne_vjp", "emu_tree_rne_vjp.cpp")
SO = os.path.join(ROOT, "tests", "emu_tree_rne_vjp", "libemu_tree_rne_vjp.so")
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the group-table compiler and registry (built if stale)
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
    so.emu_tree_rne_vjp.argtypes = [_u64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32]
    assert base is not None
    return so


def tree_handle(rob):
    """the robot's group table compiled by the emu library's own copy of tree.cpp"""
    from rtbhip._lib import rtbhip_tree_group
    recs = rob.group_table()
    arr = (rtbhip_tree_group * len(recs))()
    for k, r in enumerate(recs):
        arr[k].parent, arr[k].kind, arr[k].flip, arr[k].jindex = r["parent"], r["kind"], r["flip"], r["jindex"]
        arr[k].T[:] = list(np.ascontiguousarray(r["T"]).reshape(16))
        arr[k].m = r["m"]
        arr[k].h[:] = list(r["h"])
        arr[k].I[:] = list(r["I"])
    h = _u64(0)
    create = C.CFUNCTYPE(C.c_int, C.POINTER(rtbhip_tree_group), _i32, C.POINTER(_u64))(("rtbhip_tree_create", emu_harness.lib()))
    assert create(arr, len(recs), C.byref(h)) == 0, emu_harness.lib().rtbhip_last_error()
    return h.value


def _run(lib, rob, q, qd, qdd, g, gravity, force_rt=False):
    p = emu_harness._p
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    q, qd, qdd, g = arr(q), arr(qd), arr(qdd), arr(g)
    gc = np.ascontiguousarray(gravity, dtype=np.float64)
    out = [np.full(q.shape, np.nan) for _ in range(3)]
    assert lib.emu_tree_rne_vjp(tree_handle(rob), p(q), p(qd), p(qdd), q.shape[0], p(gc), p(g), p(out[0]), p(out[1]), p(out[2]), int(force_rt)) == 0
    return out


@pytest.mark.parametrize("name", cases.ROBOTS)
def test_lane_body_equals_the_oracle(lib, name):
    rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name)
    got = _run(lib, rob, q, qd, qdd, g, gravity)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        err = cases.rel_err(a, b)
        print("tree_rne_vjp lane %s %s: rel err %.3e (|ref|max %.3g)" % (name, what, err, np.abs(b).max()))
        assert err <= cases.BOUND, (name, what, err)


@pytest.mark.parametrize("name", ["t2", "t4"])
def test_lane_body_equals_the_oracle_on_the_census_trees(lib, name):
    """the 2- and 4-group trees tests/vjp_census_cases.py adds for the device: register forms the robots above leave out"""
    rob, orc, q, qd, qdd, g, gravity, ref = census.tree_rne_case(name)
    got = _run(lib, rob, q, qd, qdd, g, gravity)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        err = cases.rel_err(a, b)
        print("tree_rne_vjp lane %s %s: rel err %.3e (|ref|max %.3g)" % (name, what, err, np.abs(b).max()))
        assert err <= cases.BOUND, (name, what, err)
    assert cases.rel_err(got[2], cases.inertia_gqdd(orc, q, g)) <= cases.BOUND


@pytest.mark.parametrize("name", cases.AUTO)
def test_gqdd_is_the_inertia_identity(lib, name):
    rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name)
    got = _run(lib, rob, q, qd, qdd, g, gravity)
    assert cases.rel_err(got[2], cases.inertia_gqdd(orc, q, g)) <= cases.BOUND


@pytest.mark.parametrize("name", ["chain3", "tree6", "tree9", "UR5", "hand4"])
@pytest.mark.parametrize("variant", ["noqd", "noqdd", "gravity"])
def test_lane_body_variants(lib, name, variant):
    rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name, variant)
    got = _run(lib, rob, q, qd, qdd, g, gravity)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        if b is not None:
            assert cases.rel_err(a, b) <= cases.BOUND, (name, variant, what, cases.rel_err(a, b))


@pytest.mark.parametrize("name", ["one_p", "chain8", "tree5", "tree8", "UR5", "hand4"])
def test_run_time_n_form_agrees(lib, name):
    """the NG = 0 body (private-memory tape, serves 9..24 groups on the device) on robots the compile-time body also serves"""
    rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name)
    got = _run(lib, rob, q, qd, qdd, g, gravity, force_rt=True)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        assert cases.rel_err(a, b) <= cases.BOUND, (name, what, cases.rel_err(a, b))


def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include tree_rne_vjp_kernels.hip: the launcher
    is a weak reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    rob, _ = cases.robot("chain3")
    p = emu_harness._p
    x, g = np.zeros((2, rob.n)), np.zeros(3)
    proto = C.CFUNCTYPE(C.c_int, _u64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp)       # a prototype of this test's own: the shared CDLL object is left as it is
    call = proto(("rtbhip_tree_rne_vjp", emu))
    assert call(tree_handle(rob), p(x), p(x), p(x), 2, p(g), p(x), p(x.copy()), None, None, 0, None) == -1
    assert emu.rtbhip_last_error().decode() == "tree_rne_vjp: not built into this library"
