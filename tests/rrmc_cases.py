"""Shared by tests/test_rrmc.py and tests/test_rrmc_emu.py (not a test module): the robots, the draws and the ORACLE of resolved-rate motion
control (rtbhip_rrmc).

Robots: those of tests/ik_vjp_cases.py -- REG n1..n10 (one of every register form), panda, UR5, poe, prisflip.

Oracle (float64, NumPy): the loop of include/rtbhip.h's comment, literally.  Per row, for it = 0 .. steps - 1:
    T, J = fkine(q), jacob(q)     oracle.fkine / oracle.jacob0 / oracle.jacobe of the case's chain (the PoE robot: the closed form of oracle/poe.py,
                                  its jacobe the rotation of its jacob0);  method 1 "rpy": jacobe, method 0 "angle-axis": jacob0
    e    = p_servo's error        "rpy": [t ; tr2rpy] of inv(T) Tep with oracle/poe.py's tr2rpy_zyx -- the restatement tests/test_p_servo.py holds
                                  against the reference's own p_servo;  "angle-axis": oracle.angle_axis
    arr  = sum|e| < threshold ;  r = gain6 * e - J qnull ;  qd = qnull + X r ;  q = q + dt qd ;  its = it + 1 ;  stop if arr
with X = numpy.linalg.pinv(J) undamped and J^T (J J^T + d^2 I)^-1 with numpy.linalg.inv damped (for n < 6 the same matrix as
(J^T J + d^2 I)^-1 J^T).  It shares nothing with the kernel: no LDL^T, no register walk, LAPACK's SVD.

Draws: q ~ U(-3, 3); a draw is replaced while cond(J) > 1e3 (jacob0 and jacobe share their singular values), and at most a third of the draws
may be replaced (asserted by a test).  Single-step targets are Tep = fkine(q + delta), |delta|inf = 0.01 on every third row and 0.3 on the others.
Loop targets are of three kinds interleaved row by row -- |delta|inf = 0.01, 0.3 and 2.0 (below six joints the last is moved 0.5 along each
base axis as well: a short chain's least-squares steps reach any pose of its own) -- and a candidate row is replaced while the ORACLE's own
trajectory from it leaves cond(J) <= 1e3, is not finite, amplifies a perturbation of 1e-9 in q more than 1e5 times, or comes within 1e-9 threshold of the threshold at any step (so `arrived` and `its` are
decided by more than rounding); in the undamped cases without qnull of LOOP_ROBOTS (the device's loop test) it is also replaced until it behaves as its kind is named: arrived at the first
evaluation, arrived after two or more steps, not arrived in 8.  The code under test takes no part in any of this.

Bound per row:  K eps cond(J)^2 max|qd_ref|  for the single step, and  K_LOOP eps cmax^2 amp max|q_ref|  for the loop's q_out, cmax the largest
cond(J) along the oracle's trajectory of that row and amp >= 1 that trajectory's own amplification of a perturbation of q: full Newton steps that do
not arrive in 8 iterations are chaotic (measured on the oracle: 1e2 .. 1e5 on the far rows, below 1 on every row that arrives), which is the loop
map's conditioning and not the kernel's -- without the factor the far rows alone would set K_LOOP and the bound would say nothing about the
others.  amp is the oracle's loop run twice, on q and on q + 1e-9 (signs alternating over the joints).  K and K_LOOP are 8 x the largest ratio |dev - ref| / (eps cond^2 max|ref|) the CPU replay of the lane
body (tests/test_rrmc_emu.py) shows against this oracle over every case of this file -- the margin of opspace_cases.K; the device compiler
contracts nothing in this kernel (fp contract off, every fused multiply-add written)."""
import functools

import numpy as np

from oracle import oracle, poe
from helpers import chain_from_ets
import ik_vjp_cases as ikc
from ik_vjp_cases import tiled, model            # noqa: F401 (re-exported for the tests)

EPS = 2.220446049250313e-16
COND_MAX = 1e3
ROWS = 24
THRESHOLD = 0.1
DAMPINGS = (0.0, 0.1)
METHODS = (1, 0)                                 # 1 "rpy" / jacobe (the reference's default), 0 "angle-axis" / jacob0
METHOD_NAMES = {1: "rpy", 0: "angle-axis"}
GAIN_STEP = (1.0, 2.0, 0.5, 1.5, 0.75, 1.25)     # the single step: six unequal gains
GAIN_LOOP, DT = (2.0,) * 6, 0.5                  # the loop: gain dt = 1, full Newton steps
STEPS = 8
DELTAS = (0.01, 0.3, 2.0)                        # the loop's three kinds of rows
AMP_STEP, AMP_MAX = 1e-9, 1e5                    # a loop row's trajectory may amplify a perturbation of q by no more than this (judged on the oracle)
FAR_OFFSET = 0.5                                 # ... and what moves a far target off the reachable set of a chain of fewer than 6 joints (m, each axis)

REG = ikc.REG
ROBOTS = ["panda", "UR5", "poe", "prisflip"]
ALL = REG + ROBOTS
LOOP_ROBOTS = ["n3", "UR5", "panda", "n10"]

# measured: the largest |replay - oracle| / (eps cond^2 max|ref|) over every case of this file (tests/test_rrmc_emu.py prints them)
K_MEASURED, K_LOOP_MEASURED = 256.7, 39.1       # (n1-angle-axis-d0.1-qnull: 256.667; n1-angle-axis-d0.1-plain: 39.001)
K, K_LOOP = 8.0 * K_MEASURED, 8.0 * K_LOOP_MEASURED


@functools.lru_cache(maxsize=None)
def _chain(name):
    return None if name == "poe" else chain_from_ets(model(name).ets)


def fkine(name, q):
    return np.asarray(model(name).fkine(np.ascontiguousarray(q)))


def jacob(name, q, method):
    """(N, 6, n): jacobe for method 1, jacob0 for method 0"""
    q = np.ascontiguousarray(q)
    ch = _chain(name)
    if method == 0:
        return np.asarray(model(name).jacob0(q))
    if ch is not None:
        return np.asarray(oracle.jacobe(ch, q))
    J0, T = np.asarray(model(name).jacob0(q)), fkine(name, q)
    Rt = np.swapaxes(T[:, :3, :3], 1, 2)
    return np.concatenate([Rt @ J0[:, :3], Rt @ J0[:, 3:]], axis=1)


def servo_error(T, Tep, method):
    if method == 0:
        return oracle.angle_axis(T, Tep)
    eT = np.linalg.inv(T) @ Tep
    return np.concatenate([eT[:3, 3], poe.tr2rpy_zyx(eT[:3, :3])])


def pinv(J, damping):
    if damping == 0.0:
        return np.linalg.pinv(J)
    return J.T @ np.linalg.inv(J @ J.T + damping * damping * np.eye(6))


def reference(name, method, q, Tep, qnull, damping, gain6, threshold, dt, steps):
    """the oracle's loop -> dict(qd, q, arrived, its, cond: the largest cond(J) along the row's trajectory, near: the row came within
    1e-9 threshold of the threshold, finite)"""
    q = np.array(q, dtype=np.float64)
    N, n = q.shape
    Tep = np.broadcast_to(np.asarray(Tep).reshape(-1, 4, 4), (N, 4, 4))
    gain6 = np.asarray(gain6, dtype=np.float64)
    qd, its, arrived, live = np.zeros((N, n)), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool), np.ones(N, dtype=bool)
    cmax, near, finite = np.zeros(N), np.zeros(N, dtype=bool), np.ones(N, dtype=bool)
    for it in range(steps):
        idx = np.flatnonzero(live)
        if not idx.size:
            break
        T, J = fkine(name, q[idx]), jacob(name, q[idx], method)
        for a, i in enumerate(idx):
            if not (np.isfinite(T[a]).all() and np.isfinite(J[a]).all()):
                finite[i], live[i] = False, False
                continue
            e = servo_error(T[a], Tep[i], method)
            s = np.abs(e).sum()
            near[i] |= abs(s - threshold) <= 1e-9 * threshold
            qn = np.zeros(n) if qnull is None else qnull[i]
            qd[i] = qn + pinv(J[a], damping) @ (gain6 * e - J[a] @ qn)
            cmax[i] = max(cmax[i], np.linalg.cond(J[a]))
            q[i] = q[i] + dt * qd[i]
            its[i], arrived[i], live[i] = it + 1, s < threshold, not s < threshold
            if not np.isfinite(q[i]).all():
                finite[i], live[i] = False, False
    return dict(qd=qd, q=q, arrived=arrived, its=its, cond=cmax, near=near, finite=finite)


def amplification(name, method, q, Tep, qnull, damping, ref):
    """per row: how much the oracle's own loop amplifies a perturbation of q by AMP_STEP (inf for a row whose flags change under it)"""
    sign = np.where(np.arange(q.shape[1]) % 2 == 0, 1.0, -1.0)
    other = reference(name, method, q + AMP_STEP * sign, Tep, qnull, damping, GAIN_LOOP, THRESHOLD, DT, STEPS)
    amp = np.abs(other["q"] - ref["q"]).max(axis=1) / AMP_STEP
    same = (other["its"] == ref["its"]) & (other["arrived"] == ref["arrived"]) & other["finite"]
    return np.where(same, amp, np.inf)


def _rng(*key):
    """a generator seeded by the key's text (the same in every process)"""
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate("/".join(str(k) for k in key))))


def _delta(rng, n, size):
    u = rng.uniform(-1.0, 1.0, n)
    return size * u / np.abs(u).max()


@functools.lru_cache(maxsize=None)
def draws(name, rows=ROWS, seed=0):
    """(q (rows, n), drawn, replaced): q ~ U(-3, 3), a draw replaced while cond(J) > COND_MAX; read-only"""
    n = model(name).n
    rng = _rng("q", name, rows, seed)
    cand = rng.uniform(-3.0, 3.0, (4 * rows, n))
    c = np.array([np.linalg.cond(j) for j in jacob(name, cand, 0)])
    keep = np.flatnonzero(c <= COND_MAX)[:rows]
    assert keep.size == rows, (name, "too few well-conditioned draws")
    q = np.ascontiguousarray(cand[keep])
    q.setflags(write=False)
    drawn = int(keep[-1]) + 1
    return q, drawn, drawn - rows


@functools.lru_cache(maxsize=None)
def step_inputs(name, rows=ROWS, seed=0):
    """(q, Tep, qnull) of the single step; read-only"""
    q = draws(name, rows, seed)[0]
    rng = _rng("step", name, rows, seed)
    n = q.shape[1]
    d = np.array([_delta(rng, n, 0.01 if i % 3 == 0 else 0.3) for i in range(rows)])
    Tep = np.ascontiguousarray(fkine(name, q + d))
    qnull = rng.uniform(-0.5, 0.5, (rows, n))
    for a in (Tep, qnull):
        a.setflags(write=False)
    return q, Tep, qnull


@functools.lru_cache(maxsize=None)
def step_case(name, method, damping, null, rows=ROWS, seed=0):
    """-> (ets, q, Tep, qnull | None, reference dict) of one resolved-rate step with GAIN_STEP and THRESHOLD"""
    q, Tep, qnull = step_inputs(name, rows, seed)
    qn = qnull if null else None
    ref = reference(name, method, q, Tep, qn, damping, GAIN_STEP, THRESHOLD, 0.0, 1)
    assert ref["finite"].all()
    return model(name).ets, q, Tep, qn, ref


@functools.lru_cache(maxsize=None)
def loop_case(name, method, damping, null, rows=ROWS, seed=0):
    """-> (ets, q, Tep, qnull | None, reference dict, replaced) of the loop: STEPS iterations with GAIN_LOOP, DT and THRESHOLD; row i is of kind i % 3.
    The candidates of a kind are judged by the oracle's own trajectories (the module docstring) and the first rows / 3 that pass are taken."""
    n = model(name).n
    strict = damping == 0.0 and not null and name in LOOP_ROBOTS
    per = (rows + 2) // 3
    pool = (16 if rows <= ROWS else 6) * per
    rng = _rng("loop", name, method, damping, null, rows, seed)
    picked, replaced = [], 0
    for kind in range(3):
        q = draws(name, pool, 100 + seed + kind)[0]
        d = np.array([_delta(rng, n, DELTAS[kind]) for _ in range(pool)])
        Tep = np.array(fkine(name, q + d))
        if kind == 2 and n < 6:
            Tep[:, :3, 3] += FAR_OFFSET              # a short chain's least-squares steps reach any pose of its own: off its reachable set
        qnull = rng.uniform(-0.5, 0.5, (pool, n))
        ref = reference(name, method, q, Tep, qnull if null else None, damping, GAIN_LOOP, THRESHOLD, DT, STEPS)
        ok = ref["finite"] & ~ref["near"] & (ref["cond"] <= COND_MAX) & (amplification(name, method, q, Tep, qnull if null else None, damping, ref) <= AMP_MAX)
        if strict:
            ok &= [ref["arrived"] & (ref["its"] == 1), ref["arrived"] & (ref["its"] >= 2), ~ref["arrived"]][kind]
        good = np.flatnonzero(ok)[:per]
        assert good.size == per, (name, method, damping, null, kind, "too few acceptable candidates", int(ok.sum()))
        replaced += int(good[-1]) + 1 - per
        picked.append((q[good], Tep[good], qnull[good]))
    order = [(i % 3, i // 3) for i in range(rows)]
    q, Tep, qnull = (np.ascontiguousarray([picked[k][a][j] for k, j in order]) for a in range(3))
    qn = qnull if null else None
    ref = reference(name, method, q, Tep, qn, damping, GAIN_LOOP, THRESHOLD, DT, STEPS)
    assert ref["finite"].all() and not ref["near"].any()
    ref["amp"] = np.maximum(1.0, amplification(name, method, q, Tep, qn, damping, ref))
    assert (ref["amp"] <= AMP_MAX).all()
    for a in (q, Tep, qnull):
        a.setflags(write=False)
    return model(name).ets, q, Tep, qn, ref, replaced


def readme_loop_on_the_reference(q, Tep, gain, threshold, dt, steps):
    """The README's loop -- `v, arrived = rtb.p_servo(panda.fkine(panda.q), Tep, 1); panda.qd = np.linalg.pinv(panda.jacobe(panda.q)) @ v`, stepped
    by dt -- on the reference's OWN p_servo and ETS classes over its own compiled extension (oracle/ref_classes.py), row by row
    -> (q_out, arrived, its)"""
    from oracle import ref_classes
    ns = ref_classes.load_reference()
    panda = ref_classes.panda(ns)
    q = np.array(q, dtype=np.float64)
    arrived, its = np.zeros(q.shape[0], dtype=bool), np.zeros(q.shape[0], dtype=np.int32)
    for i in range(q.shape[0]):
        for it in range(steps):
            v, arr = ns.p_servo.p_servo(np.array(panda.eval(q[i])), Tep[i], gain=gain, threshold=threshold, method="rpy")
            q[i] = q[i] + dt * (np.linalg.pinv(np.array(panda.jacobe(q[i]))) @ v)
            its[i], arrived[i] = it + 1, bool(arr)
            if arr:
                break
    return q, arrived, its


def reference_available():
    from oracle import ref_classes, ref_harness
    return ref_classes.available() and ref_harness.available()


def every_case():
    return [(name, method, damping, null) for name in ALL for method in METHODS for damping in DAMPINGS for null in (False, True)]


def case_id(c):
    return "%s-%s-d%g-%s" % (c[0], METHOD_NAMES[c[1]], c[2], "qnull" if c[3] else "plain")


def ratio(got, ref, cond):
    """per row: |got - ref|max / (eps cond^2 |ref|max)"""
    got, ref = np.asarray(got).reshape(ref.shape[0], -1), np.asarray(ref).reshape(ref.shape[0], -1)
    scale = np.abs(ref).max(axis=1)
    assert (scale > 0).all()
    return np.abs(got - ref).max(axis=1) / (EPS * cond ** 2 * scale)
