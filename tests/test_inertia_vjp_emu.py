"""The adjoint of the joint-space inertia matrix on the CPU (no GPU needed): the per-lane bodies of k_inertia_vjp (csrc/inertia_vjp_kernels.hip:
inertia_vjp_lane) and k_tree_inertia_vjp (csrc/tree_inertia_vjp_kernels.hip: tree_inertia_vjp_lane) compiled host-side by this test
(tests/emu_inertia_vjp/emu_inertia_vjp.cpp, linked against tests/emu/libemu.so for the table compilers) and held against the oracle of
tests/inertia_vjp_cases.py -- Richardson differences of the reference's inertia matrix, contracted with a non-symmetric gM -- at
1e-9 max(1, |ref|max).  The device runs the same source through another compiler: tests/test_inertia_vjp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import inertia_vjp_cases as cases
import vjp_census_cases as census

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_inertia_vjp", "emu_inertia_vjp.cpp")
SO = os.path.join(ROOT, "tests", "emu_inertia_vjp", "libemu_inertia_vjp.so")
UNITS = [os.path.join(ROOT, "robotics-toolbox-python_amd", "csrc", f) for f in ("inertia_vjp_kernels.hip", "tree_inertia_vjp_kernels.hip")]
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32
N = 5


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the table compilers and registries (built if stale)
    import __graft_entry__ as g
    digest = g.source_digest(emu_harness._deps() + [SRC] + UNITS)
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        emu_dir = os.path.dirname(emu_harness.EMU_SO)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include"),
                               "-shared", SRC, "-o", SO, "-L" + emu_dir, "-l:libemu.so", "-Wl,-rpath," + emu_dir])
        open(stamp, "w").write(digest)
    so = C.CDLL(SO)
    so.emu_inertia_vjp.argtypes = [_u64, _vp, _i64, _vp, _vp, _i32]
    so.emu_tree_inertia_vjp.argtypes = [_u64, _vp, _i64, _vp, _vp, _i32]
    assert base is not None
    return so


def dyn_handle(rb):
    p = emu_harness._p
    L = np.ascontiguousarray(rb.L24())
    h = _u64(0)
    assert emu_harness.lib().rtbhip_dyn_create(p(L), rb.n, int(rb.mdh), C.byref(h)) == 0
    return h.value


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


def _run(fn, handle, q, g, force_rt=False, want=0):
    p = emu_harness._p
    q, g = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(g, dtype=np.float64)
    out = np.full(q.shape, np.nan)
    assert fn(handle, p(q), q.shape[0], p(g), p(out), int(force_rt)) == want
    return out


@pytest.mark.parametrize("name", sorted(cases.DH_ROBOTS))
def test_dh_lane_body_equals_the_oracle(lib, name):
    rb, q, g, ref = cases.dh_case(name, N)
    got = _run(lib.emu_inertia_vjp, dyn_handle(rb), q, g)
    err = cases.rel_err(got, ref)
    print("inertia_vjp lane %s: rel err %.3e (|ref|max %.3g)" % (name, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)


@pytest.mark.parametrize("name", cases.TREES)
def test_tree_lane_body_equals_the_oracle(lib, name):
    rob, orc, q, g, ref = cases.tree_case(name)
    got = _run(lib.emu_tree_inertia_vjp, tree_handle(rob), q[:N], g[:N])
    err = cases.rel_err(got, ref[:N])
    print("tree_inertia_vjp lane %s: rel err %.3e (|ref|max %.3g)" % (name, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)


CENSUS_DH = ["n4s", "n4m", "n6m", "n7s"] + sorted(census.STRUCTURED)          # register forms the zoo above leaves out; exact zeros and special angles


@pytest.mark.parametrize("name", CENSUS_DH)
def test_dh_lane_body_equals_the_oracle_on_the_census_robots(lib, name):
    """the robots tests/vjp_census_cases.py adds for the device, where this driver instantiates their joint count"""
    rb, q, g, ref = census.inertia_dh_case(name)
    err = cases.rel_err(_run(lib.emu_inertia_vjp, dyn_handle(rb), q, g), ref)
    print("inertia_vjp lane %s: rel err %.3e (|ref|max %.3g)" % (name, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)


@pytest.mark.parametrize("name", ["t2", "t4"])
def test_tree_lane_body_equals_the_oracle_on_the_census_trees(lib, name):
    rob, orc, q, g, ref = census.inertia_tree_case(name)
    err = cases.rel_err(_run(lib.emu_tree_inertia_vjp, tree_handle(rob), q, g), ref)
    print("tree_inertia_vjp lane %s: rel err %.3e (|ref|max %.3g)" % (name, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)


@pytest.mark.parametrize("name", ["puma560", "panda", "n1s", "n3s", "n8m"])
def test_dh_run_time_n_form_agrees(lib, name):
    """the NJ = 0 body (private-memory tape, serves 9..16 joints on the device) on chains the compile-time body also serves"""
    rb, q, g, ref = cases.dh_case(name, N)
    assert cases.rel_err(_run(lib.emu_inertia_vjp, dyn_handle(rb), q, g, force_rt=True), ref) <= cases.BOUND


@pytest.mark.parametrize("name", ["one_p", "chain8", "tree5", "tree8", "UR5"])
def test_tree_run_time_n_form_agrees(lib, name):
    """the NG = 0 body (private-memory tape, serves 9..20 joints on the device) on robots the compile-time body also serves"""
    rob, orc, q, g, ref = cases.tree_case(name)
    assert cases.rel_err(_run(lib.emu_tree_inertia_vjp, tree_handle(rob), q, g, force_rt=True), ref) <= cases.BOUND


@pytest.mark.parametrize("name", ["panda", "n5s"])
def test_dh_mirrored_entries_both_count(lib, name):
    """a gM that is zero except at one (i, j), i != j, gives the same gq as its transpose, and a non-zero one"""
    rb, q, g, ref = cases.dh_case(name, N)
    one = np.zeros_like(g)
    one[:, 1, 3] = 0.7
    a = _run(lib.emu_inertia_vjp, dyn_handle(rb), q, one)
    b = _run(lib.emu_inertia_vjp, dyn_handle(rb), q, np.ascontiguousarray(one.transpose(0, 2, 1)))
    assert np.array_equal(a, b) and np.abs(a).max() > 0


def test_the_motor_inertia_contributes_nothing(lib):
    """G^2 Jm sits on M's diagonal and is a constant of q: a gM on the diagonal of a one-joint chain has gradient zero"""
    rb, q, g, ref = cases.dh_case("n1s", N)
    assert np.array_equal(_run(lib.emu_inertia_vjp, dyn_handle(rb), q, g), np.zeros_like(q)) and np.abs(ref).max() <= 1e-9


def test_prismatic_chain_and_hand_numbered_tree_are_not_served(lib):
    from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH
    rb = DHRobot([RevoluteDH(a=0.3, m=1.0), PrismaticDH(alpha=0.5, m=1.0)])
    _run(lib.emu_inertia_vjp, dyn_handle(rb), np.zeros((1, 2)), np.zeros((1, 2, 2)), want=-2)
    rob, _ = cases.tree_robot(cases.HAND)
    _run(lib.emu_tree_inertia_vjp, tree_handle(rob), np.zeros((1, rob.n)), np.zeros((1, rob.n, rob.n)), want=-3)


def test_a_library_linked_without_the_kernel_units_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that includes neither inertia_vjp_kernels.hip nor
    tree_inertia_vjp_kernels.hip: the launchers are weak references there, the library loads, and the entry points say what is missing"""
    emu = emu_harness.lib()
    p = emu_harness._p
    proto = C.CFUNCTYPE(C.c_int, _u64, _vp, _i64, _vp, _vp, _i32, _vp)       # a prototype of this test's own: the shared CDLL object is left as it is
    rb = cases.dh_robot("puma560")
    x, m = np.zeros((2, rb.n)), np.zeros((2, rb.n, rb.n))
    assert proto(("rtbhip_inertia_vjp", emu))(dyn_handle(rb), p(x), 2, p(m), p(x.copy()), 0, None) == -1
    assert emu.rtbhip_last_error().decode() == "inertia_vjp: not built into this library"
    rob, _ = cases.tree_robot("chain3")
    x, m = np.zeros((2, rob.n)), np.zeros((2, rob.n, rob.n))
    assert proto(("rtbhip_tree_inertia_vjp", emu))(tree_handle(rob), p(x), 2, p(m), p(x.copy()), 0, None) == -1
    assert emu.rtbhip_last_error().decode() == "tree_inertia_vjp: not built into this library"
