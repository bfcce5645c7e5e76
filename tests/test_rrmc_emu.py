"""Resolved-rate motion control on the CPU (no GPU needed): the lane body and the tile fill / flush phases of k_rrmc (csrc/rrmc_device.h,
csrc/kin_vjp.h, csrc/vjp_tile.h) compiled host-side by this test (tests/emu_rrmc/emu_rrmc.cpp, linked against tests/emu/libemu.so for the chain
compiler) and held against the NumPy oracle of tests/rrmc_cases.py at its bounds.  This replay is also where the bounds' constants come from:
every test prints the largest ratio |replay - oracle| / (eps cond^2 max|ref|) it sees, and rrmc_cases.K / K_LOOP are 8 x the largest of them.
The device runs the same source through another compiler: tests/test_rrmc.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import rrmc_cases as cases
from rtbhip import _lib

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_rrmc", "emu_rrmc.cpp")
SO = os.path.join(ROOT, "tests", "emu_rrmc", "libemu_rrmc.so")
N = 70          # a full tile and a ragged one


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the chain compiler and the registry (built if stale)
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
    so.emu_rrmc.argtypes, so.emu_rrmc.restype = [C.POINTER(_lib.rtbhip_rrmc_args)], C.c_int
    assert base is not None
    return so


def run(lib, ets, q, Tep, qnull, method, damping, gain6, threshold, dt, steps, want=(True, True), fill=np.nan):
    """-> (qd, q_out, arrived, its); an output not wanted is handed over as NULL and comes back as the untouched buffer"""
    q, Tep = (np.ascontiguousarray(x, dtype=np.float64) for x in (q, Tep))
    qn = None if qnull is None else np.ascontiguousarray(qnull, dtype=np.float64)
    n = q.shape[0]
    qd, qo, arrived, its = np.full(q.shape, fill), np.full(q.shape, fill), np.full(n, 7, dtype=np.uint8), np.full(n, -7, dtype=np.int32)
    a = _lib.rtbhip_rrmc_args()
    a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(a), method, emu_harness.chain_handle(ets), n, Tep.reshape(-1, 16).shape[0]
    a.q, a.Tep, a.qnull = q.ctypes.data, Tep.ctypes.data, None if qn is None else qn.ctypes.data
    a.gain6 = (C.c_double * 6)(*gain6)
    a.threshold, a.damping, a.dt, a.steps = threshold, damping, dt, steps
    a.qd, a.q_out = qd.ctypes.data if want[0] else None, qo.ctypes.data if want[1] else None
    a.arrived, a.its = arrived.ctypes.data, its.ctypes.data
    assert lib.emu_rrmc(C.byref(a)) == 0
    return qd, qo, arrived, its


def test_the_cases_are_what_they_claim():
    assert [cases.model(n).n for n in cases.REG] == list(range(1, 11))
    assert cases.model("panda").n == 7 and cases.model("UR5").n == 6 and cases.model("poe").n == 6 and cases.model("prisflip").n == 7
    for name in cases.ALL:
        q, drawn, replaced = cases.draws(name)
        print("rrmc draws %s: %d of %d replaced (cond > 1e3)" % (name, replaced, drawn))
        assert 3 * replaced <= drawn, (name, replaced, drawn)
        for method in cases.METHODS:
            assert max(np.linalg.cond(j) for j in cases.jacob(name, q, method)) <= cases.COND_MAX * (1 + 1e-9)
    assert cases.K == 8.0 * cases.K_MEASURED and cases.K_LOOP == 8.0 * cases.K_LOOP_MEASURED


@pytest.mark.parametrize("name", cases.LOOP_ROBOTS)
@pytest.mark.parametrize("method", cases.METHODS, ids=[cases.METHOD_NAMES[m] for m in cases.METHODS])
def test_the_loop_rows_are_of_their_three_kinds_and_none_is_left_out(name, method):
    """the device's loop test (tests/test_rrmc.py) compares arrived and its exactly: on the oracle alone no row is near the threshold, and the
    three kinds of rows interleaved in a wave behave as named"""
    ets, q, Tep, qn, ref, replaced = cases.loop_case(name, method, 0.0, False)
    kind = np.arange(q.shape[0]) % 3
    print("rrmc loop rows %s/%s: its %s, %d candidates replaced" % (name, cases.METHOD_NAMES[method], ref["its"].tolist(), replaced))
    assert not ref["near"].any()
    assert (ref["arrived"][kind == 0] & (ref["its"][kind == 0] == 1)).all()
    assert (ref["arrived"][kind == 1] & (ref["its"][kind == 1] >= 2)).all()
    assert (~ref["arrived"][kind == 2] & (ref["its"][kind == 2] == cases.STEPS)).all()


@pytest.mark.parametrize("case", cases.every_case(), ids=cases.case_id)
def test_single_step_equals_the_oracle(lib, case):
    name, method, damping, null = case
    ets, q, Tep, qn, ref = cases.step_case(*case)
    t = lambda a: None if a is None else cases.tiled(a, N)
    qd, qo, arrived, its = run(lib, ets, t(q), t(Tep), t(qn), method, damping, cases.GAIN_STEP, cases.THRESHOLD, 0.0, 1)
    r = cases.ratio(qd, t(ref["qd"]), t(ref["cond"]))
    print("rrmc replay step %s: ratio %.3f (K_MEASURED %.3f)" % (cases.case_id(case), r.max(), cases.K_MEASURED))
    assert r.max() <= cases.K
    keep = ~t(ref["near"])
    assert np.array_equal(arrived[keep] != 0, t(ref["arrived"])[keep]) and (its == 1).all()
    assert np.array_equal(qo, t(q))              # dt = 0: q + 0 qd


@pytest.mark.parametrize("case", cases.every_case(), ids=cases.case_id)
def test_loop_equals_the_oracle(lib, case):
    name, method, damping, null = case
    ets, q, Tep, qn, ref, _ = cases.loop_case(*case)
    t = lambda a: None if a is None else cases.tiled(a, N)
    qd, qo, arrived, its = run(lib, ets, t(q), t(Tep), t(qn), method, damping, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    r = cases.ratio(qo, t(ref["q"]), t(ref["cond"])) / t(ref["amp"])
    print("rrmc replay loop %s: ratio %.3f (K_LOOP_MEASURED %.3f), its %d..%d" % (cases.case_id(case), r.max(), cases.K_LOOP_MEASURED, its.min(), its.max()))
    assert np.array_equal(arrived != 0, t(ref["arrived"])) and np.array_equal(its, t(ref["its"]))
    assert r.max() <= cases.K_LOOP


@pytest.mark.skipif(not cases.reference_available(), reason="needs oracle/_ref (the reference's compiled extension and its byte-compiled classes)")
def test_the_readme_loop_on_the_references_own_classes(lib):
    """the README loop on the Panda, run on the reference's own p_servo and ETS.jacobe: the NumPy oracle of rrmc_cases equals it (flags exactly), and
    so does the replayed kernel within the loop bound"""
    ets, q, Tep, qn, ref, _ = cases.loop_case("panda", 1, 0.0, False)
    rq, rarr, rits = cases.readme_loop_on_the_reference(q, Tep, cases.GAIN_LOOP[0], cases.THRESHOLD, cases.DT, cases.STEPS)
    assert np.array_equal(rarr, ref["arrived"]) and np.array_equal(rits, ref["its"])
    assert (cases.ratio(ref["q"], rq, ref["cond"]) / ref["amp"]).max() <= cases.K_LOOP          # the oracle against the reference
    qd, qo, arrived, its = run(lib, ets, q, Tep, None, 1, 0.0, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    r = cases.ratio(qo, rq, ref["cond"]) / ref["amp"]
    print("rrmc replay README loop against the reference's classes: ratio %.3f (K_LOOP %.1f)" % (r.max(), cases.K_LOOP))
    assert np.array_equal(arrived != 0, rarr) and np.array_equal(its, rits) and r.max() <= cases.K_LOOP


@pytest.mark.parametrize("name", ["n2", "UR5", "panda", "n10"])
def test_a_null_output_is_not_written_and_one_tep_is_the_broadcast(lib, name):
    ets, q, Tep, qn, ref, _ = cases.loop_case(name, 1, 0.0, False)
    args = (1, 0.0, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    t = lambda a: cases.tiled(a, N)
    both = run(lib, ets, t(q), t(Tep), None, *args)
    only_qd = run(lib, ets, t(q), t(Tep), None, *args, want=(True, False), fill=7.0)
    only_q = run(lib, ets, t(q), t(Tep), None, *args, want=(False, True), fill=7.0)
    assert np.array_equal(only_qd[0], both[0]) and (only_qd[1] == 7.0).all() and np.array_equal(only_q[1], both[1]) and (only_q[0] == 7.0).all()
    for o in (only_qd, only_q):
        assert np.array_equal(o[2], both[2]) and np.array_equal(o[3], both[3])
    one = run(lib, ets, t(q), Tep[4], None, *args)
    bc = run(lib, ets, t(q), np.broadcast_to(Tep[4], (N, 4, 4)), None, *args)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one, bc))


def test_a_row_that_is_not_finite_runs_out_its_steps_and_stays_in_its_row(lib):
    ets, q, Tep, qn, ref, _ = cases.loop_case("UR5", 1, 0.0, False)
    t = lambda a: cases.tiled(a, N)
    args = (1, 0.0, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    base = run(lib, ets, t(q), t(Tep), None, *args)
    q2 = np.array(t(q))
    q2[5, 2] = np.nan
    q2[66, 0] = np.inf
    got = run(lib, ets, q2, t(Tep), None, *args)
    others = np.delete(np.arange(N), [5, 66])
    for x, y in zip(got, base):
        assert np.array_equal(x[others], y[others])
    assert not np.isfinite(got[0][[5, 66]]).any() and not np.isfinite(got[1][[5, 66]]).any()
    assert (got[2][[5, 66]] == 0).all() and (got[3][[5, 66]] == cases.STEPS).all()


def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include rrmc_kernels.hip: the launcher is a weak
    reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    ets, q, Tep, qn, ref = cases.step_case("n2", 1, 0.0, False)
    q, Tep, out = np.array(q), np.array(Tep), np.zeros(q.shape)
    a = _lib.rtbhip_rrmc_args()
    a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(a), 1, emu_harness.chain_handle(ets), q.shape[0], q.shape[0]
    a.q, a.Tep, a.qd, a.steps, a.threshold = q.ctypes.data, Tep.ctypes.data, out.ctypes.data, 1, 0.1
    call = C.CFUNCTYPE(C.c_int, C.POINTER(_lib.rtbhip_rrmc_args))(("rtbhip_rrmc", emu))
    assert call(C.byref(a)) == -1 and emu.rtbhip_last_error().decode() == "rrmc: not built into this library"
    a.N = a.nTep = 0
    assert call(C.byref(a)) == 0 and not out.any()
