"""The reactive QP servo on the CPU (no GPU needed): the lane body and the tile fill / flush phases of k_mmc (csrc/mmc_device.h, csrc/kin_vjp.h,
csrc/vjp_tile.h) compiled host-side by this test (tests/emu_mmc/emu_mmc.cpp, linked against tests/emu/libemu.so for the chain compiler) and held
against the NumPy oracle of tests/mmc_cases.py at its bounds.  This replay is also where the bounds' constants come from: every test prints the
largest ratio it sees, and mmc_cases.K / K_LOOP are 8 x the largest of them.  The oracle itself is asserted here -- how many draws it replaced,
what its rows hold, that scipy's SLSQP finds the same minimiser.  The device runs the same source through another compiler: tests/test_mmc.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import mmc_cases as cases
from rtbhip import _lib

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_mmc", "emu_mmc.cpp")
SO = os.path.join(ROOT, "tests", "emu_mmc", "libemu_mmc.so")
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
    so.emu_mmc.argtypes, so.emu_mmc.restype = [C.POINTER(_lib.rtbhip_mmc_args)], C.c_int
    assert base is not None
    return so


def run(lib, ets, q, Tep, su, method, gain6, threshold, dt, steps, want=(True, True), fill=np.nan):
    """-> (qd, q_out, arrived, its, status); an output not wanted is handed over as NULL and comes back as the untouched buffer"""
    q, Tep = (np.ascontiguousarray(x, dtype=np.float64) for x in (q, Tep))
    n = q.shape[0]
    qd, qo = np.full(q.shape, fill), np.full(q.shape, fill)
    arrived, its, status = np.full(n, 7, dtype=np.uint8), np.full(n, -7, dtype=np.int32), np.full(n, 77, dtype=np.uint8)
    qlim = np.ascontiguousarray(su.qlim)
    a = _lib.rtbhip_mmc_args()
    a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(a), method, emu_harness.chain_handle(ets), n, Tep.reshape(-1, 16).shape[0]
    a.q, a.Tep, a.qlim, a.qdlim = q.ctypes.data, Tep.ctypes.data, qlim.ctypes.data, None if su.qdlim is None else su.qdlim.ctypes.data
    a.gain6 = (C.c_double * 6)(*gain6)
    a.threshold, a.dt, a.steps = threshold, dt, steps
    a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = su.Y, su.ks, su.km, su.ps, su.pi, su.dgain
    a.qd, a.q_out = qd.ctypes.data if want[0] else None, qo.ctypes.data if want[1] else None
    a.arrived, a.its, a.status = arrived.ctypes.data, its.ctypes.data, status.ctypes.data
    assert lib.emu_mmc(C.byref(a)) == 0
    return qd, qo, arrived, its, status


# ------------------------------------------------------------------------------------------------ the oracle alone
def test_the_cases_are_what_they_claim():
    """the draws: at most a third replaced; in every case at least a third of the rows hold a joint, some row holds two; across the cases both
    sides and both kinds of bound occur; no slack beyond 10"""
    assert [cases.model(n).n for n in cases.ROBOTS] == [6, 7, 8, 9, 10]
    sides, kinds, sizes = set(), set(), {}
    for case in cases.every_case():
        ets, q, Tep, su, ref, drawn, replaced = cases.step_case(case)
        held = [len(r["held"]) for r in ref["first"]]
        print("mmc draws %s: %d of %d replaced %r; held-set sizes %s; largest slack %.3f" % (cases.case_id(case), sum(replaced.values()), drawn, replaced,
                                                                                             np.bincount(held).tolist(), ref["slack"].max()))
        assert 3 * sum(replaced.values()) <= drawn, (case, replaced, drawn)
        assert max(r["cond"] for r in ref["first"]) <= cases.COND_MAX
        assert 3 * sum(h >= 1 for h in held) >= len(held), (case, held)
        assert max(held) >= 2, (case, held)
        for r in ref["first"]:
            for kind, side in r["kinds"]:
                kinds.add(kind)
                sides.add(side)
        for h in held:
            sizes[h] = sizes.get(h, 0) + 1
        assert ref["slack"].max() <= cases.SLACK_MAX and not ref["status"].any()
        if case[4] == "narrow":         # both dampers of the narrow joint are active on every row
            j = cases.NARROW_JOINT
            assert (su.qlim[1, j] - q[:, j] <= su.pi).all() and (q[:, j] - su.qlim[0, j] <= su.pi).all() and su.qlim[1, j] - su.qlim[0, j] < 2 * np.pi
    print("mmc held-set sizes over all cases: %r" % sorted(sizes.items()))
    assert sides == {0, 1} and kinds == {"damper", "box"}
    assert cases.K == 8.0 * cases.K_MEASURED and cases.K_LOOP == 8.0 * cases.K_LOOP_MEASURED and cases.K_MEASURED <= 1e4


def test_the_enumeration_is_the_minimiser_scipy_finds():
    """the oracle's QP pinned on scipy.optimize.minimize(method="SLSQP") in (qd, delta) with the equality rows and the box, a handful of rows"""
    opt = pytest.importorskip("scipy.optimize")
    from oracle import oracle
    import rrmc_cases as rc
    checked = 0
    for case in [("panda", 1, True, True, "plain"), ("UR5", 0, True, True, "plain"), ("n10", 1, False, True, "plain"), ("panda", 1, True, True, "narrow")]:
        name, method = case[0], case[1]
        ets, q, Tep, su, ref, _, _ = cases.step_case(case)
        n = q.shape[1]
        for i in (0, 7, 13):
            r = ref["first"][i]
            J = cases.jacob(name, q[i:i + 1], method)[0]
            v = np.asarray(cases.gain_of(case)) * r["e"]
            c = oracle.jacobm(rc._chain(name), q[i:i + 1], "all")[0].reshape(-1) / su.km if su.km > 0 else np.zeros(n)
            lo, hi, _, _ = cases.box_of(su, q[i])
            w = su.ks / r["s"]
            f = lambda x: 0.5 * su.Y * x[:n] @ x[:n] + 0.5 * w * x[n:] @ x[n:] - c @ x[:n]
            df = lambda x: np.concatenate([su.Y * x[:n] - c, w * x[n:]])
            A = np.hstack([J, np.eye(6)])
            x0 = np.concatenate([np.clip(np.zeros(n), lo, hi), v])
            x0[n:] = v - J @ x0[:n]
            res = opt.minimize(f, x0, jac=df, method="SLSQP", bounds=list(zip(lo, hi)) + [(None, None)] * 6,
                               constraints=[dict(type="eq", fun=lambda x: A @ x - v, jac=lambda x: A)], options=dict(ftol=1e-15, maxiter=500))
            assert res.success, (case, i, res.message)
            scale = max(np.abs(r["qd"]).max(), 1.0)
            assert np.abs(res.x[:n] - r["qd"]).max() <= 1e-5 * scale, (case, i, np.abs(res.x[:n] - r["qd"]).max())
            ours = np.concatenate([r["qd"], v - J @ r["qd"]])
            assert f(ours) <= f(res.x) + 1e-9 * max(1.0, abs(f(res.x)))          # and the enumeration's point is no worse
            checked += 1
    assert checked == 12


@pytest.mark.parametrize("name", cases.LOOP_ROBOTS)
@pytest.mark.parametrize("method", cases.METHODS, ids=[cases.METHOD_NAMES[m] for m in cases.METHODS])
def test_the_loop_rows_are_of_their_three_kinds(name, method):
    ets, q, Tep, su, ref, replaced = cases.loop_case(name, method)
    kind = np.arange(q.shape[0]) % 3
    print("mmc loop rows %s/%s: its %s, %d candidates replaced, largest slack %.3f" % (name, cases.METHOD_NAMES[method], ref["its"].tolist(), replaced,
                                                                                      ref["slack"].max()))
    assert not ref["near"].any() and not ref["status"].any() and not ref["degenerate"].any()
    assert (ref["arrived"][kind == 0] & (ref["its"][kind == 0] == 1)).all()
    assert (ref["arrived"][kind == 1] & (ref["its"][kind == 1] >= 2)).all()
    assert (~ref["arrived"][kind == 2] & (ref["its"][kind == 2] == cases.STEPS)).all()


# ------------------------------------------------------------------------------------------------ the replay against the oracle
@pytest.mark.parametrize("case", cases.every_case(), ids=cases.case_id)
def test_single_step_equals_the_oracle(lib, case):
    ets, q, Tep, su, ref, _, _ = cases.step_case(case)
    qd, qo, arrived, its, status = run(lib, ets, q, Tep, su, case[1], cases.gain_of(case), cases.THRESHOLD, 0.0, 1)
    r = cases.step_ratio(qd, ref)
    print("mmc replay step %s: ratio %.3f (K_MEASURED %.3f)" % (cases.case_id(case), r.max(), cases.K_MEASURED))
    assert r.max() <= cases.K
    assert np.array_equal(arrived != 0, ref["arrived"]) and (its == 1).all() and np.array_equal(status, ref["status"])
    assert np.array_equal(qo, q)                 # dt = 0: q + 0 qd


@pytest.mark.parametrize("name", cases.LOOP_ROBOTS)
@pytest.mark.parametrize("method", cases.METHODS, ids=[cases.METHOD_NAMES[m] for m in cases.METHODS])
def test_loop_equals_the_oracle(lib, name, method):
    ets, q, Tep, su, ref, _ = cases.loop_case(name, method)
    t = lambda a: cases.tiled(a, N)
    qd, qo, arrived, its, status = run(lib, ets, t(q), t(Tep), su, method, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    r = cases.rc.ratio(qo, t(ref["q"]), t(ref["cond"])) / t(ref["amp"])
    print("mmc replay loop %s/%s: ratio %.3f (K_LOOP_MEASURED %.3f), its %d..%d" % (name, cases.METHOD_NAMES[method], r.max(), cases.K_LOOP_MEASURED,
                                                                                   its.min(), its.max()))
    assert np.array_equal(arrived != 0, t(ref["arrived"])) and np.array_equal(its, t(ref["its"])) and np.array_equal(status, t(ref["status"]))
    assert r.max() <= cases.K_LOOP


def test_a_slack_beyond_ten_sets_status_bit_one(lib):
    """no other case has a slack above 10 (the issue's cases are built so): here the gains are 40 times the case's, the oracle's slack is past 20
    on some rows and clear of 10 on all, and bit 1 must be the oracle's on every row -- set where |v - J qd|inf > 10, clear elsewhere"""
    ets, q, Tep, su, gain6, ref = cases.slack_case()
    qd, qo, arrived, its, status = run(lib, ets, q, Tep, su, 1, gain6, cases.THRESHOLD, 0.0, 1)
    print("mmc replay slack rows: oracle slack %s, status %s" % (np.round(ref["slack"], 2).tolist(), status.tolist()))
    assert np.array_equal(status, ref["status"]) and (status == 2).any() and np.array_equal(arrived != 0, ref["arrived"])
    assert cases.step_ratio(qd, ref).max() <= cases.K


# ------------------------------------------------------------------------------------------------ the tile phases
@pytest.mark.parametrize("name", ["UR5", "panda", "n10"])
def test_tile_phases_between_guard_rows(lib, name):
    """N = 1, 63, 64, 65, 70 inside larger buffers: the rows before and after the batch keep their pattern, every live row is written"""
    case = (name, 1, True, True, "plain")
    ets, q, Tep, su, ref, _, _ = cases.step_case(case)
    n = q.shape[1]
    for rows in (1, 63, 64, 65, 70):
        G = 3
        tq, tT = cases.tiled(q, rows), cases.tiled(Tep, rows)
        a = _lib.rtbhip_mmc_args()
        bufs = dict(qd=np.full((rows + 2 * G, n), 7.5), q_out=np.full((rows + 2 * G, n), 7.5), arrived=np.full(rows + 2 * G, 9, dtype=np.uint8),
                    its=np.full(rows + 2 * G, -9, dtype=np.int32), status=np.full(rows + 2 * G, 99, dtype=np.uint8))
        qin, Tin = np.ascontiguousarray(tq), np.ascontiguousarray(tT)
        qlim = np.ascontiguousarray(su.qlim)
        a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(a), 1, emu_harness.chain_handle(ets), rows, rows
        a.q, a.Tep, a.qlim, a.qdlim = qin.ctypes.data, Tin.ctypes.data, qlim.ctypes.data, su.qdlim.ctypes.data
        a.gain6 = (C.c_double * 6)(*cases.gain_of(case))
        a.threshold, a.dt, a.steps = cases.THRESHOLD, 0.5, 1
        a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = su.Y, su.ks, su.km, su.ps, su.pi, su.dgain
        for k, b in bufs.items():
            setattr(a, k, b.ctypes.data + G * b.strides[0])
        assert lib.emu_mmc(C.byref(a)) == 0
        for k, b in bufs.items():
            guard = np.concatenate([b[:G], b[rows + G:]])
            assert (guard == guard.flat[0]).all(), (name, rows, k)
        live = {k: b[G:rows + G] for k, b in bufs.items()}
        assert cases.step_ratio(live["qd"], {"qd": cases.tiled(ref["qd"], rows), "first": [ref["first"][i % len(ref["first"])] for i in range(rows)]}).max() <= cases.K
        assert np.array_equal(live["q_out"], tq + 0.5 * live["qd"]) and (live["its"] == 1).all() and not live["status"].any()
        assert np.array_equal(live["arrived"] != 0, cases.tiled(ref["arrived"], rows))


@pytest.mark.parametrize("name", ["UR5", "panda", "n10"])
def test_a_null_output_is_not_written_and_one_tep_is_the_broadcast(lib, name):
    ets, q, Tep, su, ref, _ = cases.loop_case(name, 1)
    args = (su, 1, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
    t = lambda a: cases.tiled(a, N)
    both = run(lib, ets, t(q), t(Tep), *args)
    only_qd = run(lib, ets, t(q), t(Tep), *args, want=(True, False), fill=7.0)
    only_q = run(lib, ets, t(q), t(Tep), *args, want=(False, True), fill=7.0)
    assert np.array_equal(only_qd[0], both[0]) and (only_qd[1] == 7.0).all() and np.array_equal(only_q[1], both[1]) and (only_q[0] == 7.0).all()
    for o in (only_qd, only_q):
        assert all(np.array_equal(o[k], both[k]) for k in (2, 3, 4))
    one = run(lib, ets, t(q), Tep[4], *args)
    bc = run(lib, ets, t(q), np.broadcast_to(Tep[4], (N, 4, 4)), *args)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one, bc))


@pytest.mark.parametrize("steps", [1, cases.STEPS])
def test_unsolvable_rows_keep_to_their_rows(lib, steps):
    """an empty box and a q that is not finite: status bit 0, rate and q non-finite, never arrived, its = steps; every other row keeps its bits"""
    ets, q, Tep, su, ref = cases.unsolvable_case("panda")
    args = (su, 1, cases.gain_of(("panda", 1, True, True, "plain")), cases.THRESHOLD, 0.05, steps)
    good = cases.step_case(("panda", 1, True, True, "plain"))[1]
    base = run(lib, ets, good, Tep, *args)
    q2 = np.array(q)
    q2[11, 3] = np.nan
    q2[17, 0] = np.inf
    got = run(lib, ets, q2, Tep, *args)
    bad = [cases.UNSOLVABLE_ROW, 11, 17]
    others = np.delete(np.arange(q.shape[0]), bad)
    for x, y in zip(got, base):
        assert np.array_equal(x[others], y[others])
    assert not np.isfinite(got[0][bad]).any() and not np.isfinite(got[1][bad]).any()
    assert (got[2][bad] == 0).all() and (got[3][bad] == steps).all() and (got[4][bad] == 1).all() and not (base[4] & 1).any()
    if steps == 1:
        assert np.array_equal(got[4][:q.shape[0]], np.where(np.isin(np.arange(q.shape[0]), bad), 1, 0))
        assert np.array_equal(run(lib, ets, q, Tep, *args)[4], ref["status"])          # the oracle's own verdict on the empty box


def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include mmc_kernels.hip: the launcher is a weak
    reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    ets, q, Tep, su, ref, _, _ = cases.step_case(("UR5", 1, True, True, "plain"))
    q, Tep, out, qlim = np.array(q), np.array(Tep), np.zeros(q.shape), np.ascontiguousarray(su.qlim)
    a = _lib.rtbhip_mmc_args()
    a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(a), 1, emu_harness.chain_handle(ets), q.shape[0], q.shape[0]
    a.q, a.Tep, a.qlim, a.qd, a.steps, a.threshold = q.ctypes.data, Tep.ctypes.data, qlim.ctypes.data, out.ctypes.data, 1, 0.1
    a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = su.Y, su.ks, su.km, su.ps, su.pi, su.dgain
    call = C.CFUNCTYPE(C.c_int, C.POINTER(_lib.rtbhip_mmc_args))(("rtbhip_mmc", emu))
    assert call(C.byref(a)) == -1 and emu.rtbhip_last_error().decode() == "mmc: not built into this library"
    a.N = a.nTep = 0
    assert call(C.byref(a)) == 0 and not out.any()
