"""Shared by tests/test_mmc.py and tests/test_mmc_emu.py (not a test module): the robots, the draws and the ORACLE of the reactive QP servo
(rtbhip_mmc).

Oracle (float64, NumPy): the definition of include/rtbhip.h's comment, literally.  Per row, for it = 0 .. steps - 1:
    T, J0 = fkine(q), jacob0(q) ;  J = jacobe(q) for method 1 "rpy", J0 for method 0 "angle-axis"      rrmc_cases.fkine / jacob
    e   = p_servo's error (rrmc_cases.servo_error) ;  s = sum|e| ;  arr = s < threshold ;  v = gain6 * e
    qd  = argmin over (qd, delta) of  1/2 Y |qd|^2 + 1/2 (ks / s) |delta|^2 - (1 / km) jacobm(q)^T qd,   J qd + delta = v,  lo <= qd <= hi
    q   = q + dt qd ;  its = it + 1 ;  if arr: stop
with jacobm = oracle.jacobm (all six axes, of J0), the box [-qdlim, qdlim] tightened by the dampers, both sides of a joint independently:
    qlim_hi - q <= pi:  hi = min(hi,  damper_gain ((qlim_hi - q) - ps) / (pi - ps))
    q - qlim_lo <= pi:  lo = max(lo, -damper_gain ((q - qlim_lo) - ps) / (pi - ps))
The QP is solved by ENUMERATION: candidate held sets in order of size, each with both sides of its joints; for each the full KKT system in
(qd, delta, the six equality multipliers, the held joints' multipliers) by numpy.linalg.solve; the first primal-feasible point with non-negative
multipliers is kept -- the minimiser of a strictly convex QP is unique.  It shares nothing with the device's method: no elimination of the slack,
no 6 x 6 system, no active-set walk.  tests/test_mmc_emu.py pins it on scipy.optimize.minimize(method="SLSQP").
A row is UNSOLVABLE (status bit 0, rate and q non-finite from there on, never arrived, its = steps) when its box is empty (lo_j > hi_j) or its q
is not finite.  NOTE: a joint inside ps of ONE limit only makes that side's bound cross zero; the box is empty when that bound crosses the other
side's -- a joint past its limit by more than ps + qdlim (pi - ps) / damper_gain, or a joint within ps of both limits.

Robots: the 6..10-joint chains of rrmc_cases, one per instantiation of k_mmc.  qlim = +-3.2 supplied explicitly, pi = 0.9, ps = 0.05,
qdlim = 2.0, Y = 0.01, ks = 1, km = 1 on the arms and 16 on the random chains (KM below).  q ~ U(-3, 3); targets fkine(q + delta), |delta|inf 0.3 and 1.0 on alternate rows.  A draw is replaced while
cond(J) > 1e3, the oracle finds the box empty, the KKT point is degenerate (a free joint within 1e-9 of a bound, a held joint's multiplier
below 1e-9), or sum|e| is within 1e-9 of the threshold; at most a third of the draws may be replaced (asserted by a test).  The code under test takes no part in any of this.

Bound per row, single step:  |qd - ref| <= K eps c scale,  c = max(cond(J)^2, cond(J_F J_F^T + d^2 I)) at the oracle's free set F,
d^2 = Y s / ks, scale = max(|qd_ref|inf, |g|inf), g = jacobm / (Y km): the rate is a difference of terms of size g.
Loop: rrmc_cases' form, K_LOOP eps cmax^2 amp max|q_ref|, cmax the largest cond(J) along the oracle's trajectory and amp >= 1 that trajectory's
own amplification of a perturbation of 1e-9 in q.  Loop rows are of three kinds chosen by the oracle's trajectories alone: arrived at once,
arrived after two or more steps, not arrived in 8; a candidate is replaced when it comes within 1e-9 of the threshold, amplifies more than 1e5
times, meets an empty box or a degenerate KKT point on its way.
K and K_LOOP are 8 x the largest ratio the CPU replay (tests/test_mmc_emu.py) shows against this oracle over every case of this file."""
import functools
import itertools

import numpy as np

from oracle import oracle
import rrmc_cases as rc
from rrmc_cases import tiled, model, fkine, jacob, servo_error            # noqa: F401 (re-exported for the tests)

EPS = rc.EPS
COND_MAX = 1e3
ROWS = 24
THRESHOLD = 0.1
METHODS = (1, 0)
METHOD_NAMES = rc.METHOD_NAMES
GAIN_STEP = (1.0, 2.0, 0.5, 1.5, 0.75, 1.25)          # six unequal gains, times GAIN_SCALE[velocity box?]
# The gains are the cases' to choose, and are chosen on the oracle alone: without the velocity box only a damper can bind, and it binds only for a
# large v; with the box whatever of v lies beyond qdlim's reach goes into the slack.  At these scales at least a third of the rows of every case
# hold a joint and no slack exceeds 10 (tests/test_mmc_emu.py asserts both and prints the counts).
GAIN_SCALE = {True: 2.0, False: 5.0}
# ... and, as km below, per robot where a robot needs it: without the box n10 (links of metres: its v is mostly translation, and goes into the
# slack before it reaches a damper) runs with a stiffer slack, ks, and the gain that then keeps a third of its rows on a damper
NOBOX = {"n10": dict(gain=6.0, ks=4.0)}
GAIN_LOOP, DT = (2.0,) * 6, 0.25
STEPS = 8
AMP_STEP, AMP_MAX = 1e-9, 1e5
DEGENERATE = 1e-9
SLACK_MAX = 10.0

ROBOTS = ["UR5", "panda", "n8", "n9", "n10"]          # 6, 7, 8, 9, 10 joints
LOOP_ROBOTS = ["UR5", "panda", "n10"]
QLIM, PI, PS, QDLIM = 3.2, 0.9, 0.05, 2.0
Y, KS, DGAIN = 0.01, 1.0, 1.0
# km when the manipulability term is on.  The random chains n8..n10 have links of metres: their jacobm, and with it g = jacobm / (Y km), is ~16 times
# an arm's (|g|inf up to 160 rad/s against 10 on the Panda and the UR5); km scales it back to where the arms -- and the probe of DESIGN.md 4.20 -- run
KM = {"UR5": 1.0, "panda": 1.0, "n8": 16.0, "n9": 16.0, "n10": 16.0}
NARROW_JOINT, NARROW = 2, 0.8                        # the "narrow" variant: this joint's limits are +-0.8, a range below 2 pi
STEP_DELTAS = (0.3, 1.0)
LOOP_DELTAS = (0.01, 0.3, 1.0)

# measured: the largest |replay - oracle| / bound-without-K over every case of this file (tests/test_mmc_emu.py prints them)
K_MEASURED, K_LOOP_MEASURED = 2.822, 0.351          # (n9-rpy-km0-box: 2.822; the loop on n10 / rpy: 0.351)
K, K_LOOP = 8.0 * K_MEASURED, 8.0 * K_LOOP_MEASURED


class Setup:
    """the scalars and the host arrays of one launch"""

    def __init__(self, n, km=1.0, box=True, narrow=False, ks=KS):
        self.Y, self.ks, self.km, self.ps, self.pi, self.dgain = Y, ks, km, PS, PI, DGAIN
        self.qlim = np.array([[-QLIM] * n, [QLIM] * n])
        if narrow:
            self.qlim[:, NARROW_JOINT] = (-NARROW, NARROW)
        self.qdlim = np.full(n, QDLIM) if box else None
        self.qlim.setflags(write=False)


def box_of(su, q):
    """(lo, hi, kind_lo, kind_hi) of one row: the bounds and what set them ("box", "damper" or None)"""
    n = q.shape[0]
    hi = np.full(n, np.inf) if su.qdlim is None else np.array(su.qdlim, dtype=np.float64)
    lo = -hi
    klo, khi = [None if su.qdlim is None else "box"] * n, [None if su.qdlim is None else "box"] * n
    for j in range(n):
        up, dn = su.qlim[1, j] - q[j], q[j] - su.qlim[0, j]
        if up <= su.pi:
            b = su.dgain * (up - su.ps) / (su.pi - su.ps)
            if b < hi[j]:
                hi[j], khi[j] = b, "damper"
        if dn <= su.pi:
            b = -su.dgain * (dn - su.ps) / (su.pi - su.ps)
            if b > lo[j]:
                lo[j], klo[j] = b, "damper"
    return lo, hi, klo, khi


TOL = 1e-12


def solve_qp(J, v, s, jm, lo, hi, su):
    """the enumeration of the module docstring -> dict(qd, delta, held: {joint: side 0 lower / 1 upper}, lam: the held joints' multipliers)"""
    n = J.shape[1]
    c = jm / su.km if su.km > 0 else np.zeros(n)
    w = su.ks / s
    d0 = n + 12
    base = np.zeros((d0, d0))
    base[:n, :n] = su.Y * np.eye(n)
    base[:n, n + 6:] = J.T
    base[n:n + 6, n:n + 6] = w * np.eye(6)
    base[n:n + 6, n + 6:] = np.eye(6)
    base[n + 6:, :n] = J
    base[n + 6:, n:n + 6] = np.eye(6)
    rhs = np.concatenate([c, np.zeros(6), v])
    for k in range(n + 1):
        cands = [(S, sd) for S in itertools.combinations(range(n), k) for sd in itertools.product((0, 1), repeat=k)]
        cands = [(S, sd) for S, sd in cands if all(np.isfinite(hi[j] if t else lo[j]) for j, t in zip(S, sd))]
        if not cands:
            continue
        m = len(cands)
        A = np.zeros((m, d0 + k, d0 + k))
        b = np.zeros((m, d0 + k))
        A[:, :d0, :d0] = base
        b[:, :d0] = rhs
        sgn = np.ones((m, k))
        for a, (S, sd) in enumerate(cands):
            for i, (j, t) in enumerate(zip(S, sd)):
                A[a, j, d0 + i] = 1.0
                A[a, d0 + i, j] = 1.0
                b[a, d0 + i] = hi[j] if t else lo[j]
                sgn[a, i] = 1.0 if t else -1.0
        z = np.linalg.solve(A, b[:, :, None])[:, :, 0]
        qd, lam = z[:, :n], z[:, d0:] * sgn
        ok = (qd >= lo - TOL).all(axis=1) & (qd <= hi + TOL).all(axis=1) & (lam >= -TOL).all(axis=1)
        if ok.any():
            a = int(np.flatnonzero(ok)[0])
            S, sd = cands[a]
            return dict(qd=qd[a], delta=z[a, n:n + 6], held=dict(zip(S, sd)), lam=lam[a])
    raise AssertionError("no KKT point found: the box is not empty, so this cannot happen")


def _step(name, method, q, Tep, gain6, su, detail=False):
    """one evaluation of one row -> dict(qd | None when unsolvable, s, cond, ...)"""
    ch = rc._chain(name)
    q1 = q[None]
    T, J0 = fkine(name, q1)[0], np.asarray(model(name).jacob0(np.ascontiguousarray(q1)))[0]
    J = jacob(name, q1, method)[0]
    e = servo_error(T, Tep, method)
    s = float(np.abs(e).sum())
    v = np.asarray(gain6) * e
    jm = oracle.jacobm(ch, q1, "all")[0].reshape(-1) if su.km > 0 else np.zeros(q.shape[0])
    lo, hi, klo, khi = box_of(su, q)
    out = dict(s=s, cond=float(np.linalg.cond(J)), empty=bool((lo > hi).any()), e=e)
    if out["empty"]:
        out["qd"] = None
        return out
    sol = solve_qp(J, v, s, jm, lo, hi, su)
    qd = sol["qd"]
    free = [j for j in range(q.shape[0]) if j not in sol["held"]]
    margin = min([min(qd[j] - lo[j], hi[j] - qd[j]) for j in free], default=np.inf)
    out.update(qd=qd, held=sol["held"], slack=float(np.abs(v - J @ qd).max()),
               degenerate=bool(margin < DEGENERATE or (sol["lam"] < DEGENERATE).any()))
    if detail:
        g = jm / (su.Y * su.km) if su.km > 0 else np.zeros(q.shape[0])
        JF = J[:, free]
        out.update(g=g, cF=float(np.linalg.cond(JF @ JF.T + su.Y * s / su.ks * np.eye(6))),
                   kinds=[(khi[j] if t else klo[j], t) for j, t in sol["held"].items()])
    return out


def reference(name, method, q, Tep, gain6, threshold, dt, steps, su):
    """the oracle's loop -> dict(qd, q, arrived, its, status, cond: the largest cond(J) along the row's trajectory, near, degenerate, slack: the
    largest along the way, first: the detail of every row's first evaluation)"""
    q = np.array(q, dtype=np.float64)
    N, n = q.shape
    Tep = np.broadcast_to(np.asarray(Tep).reshape(-1, 4, 4), (N, 4, 4))
    qd, its, arrived = np.zeros((N, n)), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
    status, cmax, near, degen, slack = np.zeros(N, dtype=np.uint8), np.zeros(N), np.zeros(N, dtype=bool), np.zeros(N, dtype=bool), np.zeros(N)
    first = [None] * N
    for i in range(N):
        for it in range(steps):
            its[i] = it + 1
            if not np.isfinite(q[i]).all():
                status[i] |= 1
                qd[i], q[i] = np.nan, np.nan
                continue
            r = _step(name, method, q[i], Tep[i], gain6, su, detail=it == 0)
            if it == 0:
                first[i] = r
            cmax[i] = max(cmax[i], r["cond"])
            near[i] |= abs(r["s"] - threshold) <= 1e-9 * threshold
            if r["qd"] is None:
                status[i] |= 1
                qd[i], q[i] = np.nan, np.nan
                continue
            degen[i] |= r["degenerate"]
            slack[i] = max(slack[i], r["slack"])
            if r["slack"] > SLACK_MAX:
                status[i] |= 2
            qd[i] = r["qd"]
            q[i] = q[i] + dt * qd[i]
            if r["s"] < threshold:
                arrived[i] = True
                break
    return dict(qd=qd, q=q, arrived=arrived, its=its, status=status, cond=cmax, near=near, degenerate=degen, slack=slack, first=first)


def amplification(name, method, q, Tep, su, ref):
    sign = np.where(np.arange(q.shape[1]) % 2 == 0, 1.0, -1.0)
    other = reference(name, method, q + AMP_STEP * sign, Tep, GAIN_LOOP, THRESHOLD, DT, STEPS, su)
    amp = np.abs(other["q"] - ref["q"]).max(axis=1) / AMP_STEP
    same = (other["its"] == ref["its"]) & (other["arrived"] == ref["arrived"]) & (other["status"] == ref["status"])
    return np.where(same & np.isfinite(amp), amp, np.inf)


def _rng(*key):
    return rc._rng("mmc", *key)


def _candidates(name, narrow, count, *key):
    """q ~ U(-3, 3) with cond(J) <= COND_MAX (the narrow variant: its joint inside +-0.09, where both of its dampers are active)"""
    n = model(name).n
    rng = _rng("q", name, narrow, count, *key)
    q = rng.uniform(-3.0, 3.0, (4 * count, n))
    if narrow:
        q[:, NARROW_JOINT] = rng.uniform(-0.09, 0.09, 4 * count)
    c = np.array([np.linalg.cond(j) for j in jacob(name, q, 0)])
    return q, c <= COND_MAX, rng


# a case of the single step: (robot, method, km on, velocity box, variant "plain" | "narrow")
def every_case():
    grid = [(name, method, km, box, "plain") for name in ROBOTS for method in METHODS for km in (True, False) for box in (True, False)]
    return grid + [(name, 1, True, True, "narrow") for name in ROBOTS]


def case_id(c):
    return "%s-%s-%s-%s%s" % (c[0], METHOD_NAMES[c[1]], "km" if c[2] else "km0", "box" if c[3] else "nobox", "" if c[4] == "plain" else "-" + c[4])


def gain_of(case):
    scale = GAIN_SCALE[bool(case[3])] if case[3] or case[0] not in NOBOX else NOBOX[case[0]]["gain"]
    return tuple(scale * g for g in GAIN_STEP)


def setup_of(case):
    name, method, km, box, variant = case
    ks = KS if box or name not in NOBOX else NOBOX[name]["ks"]
    return Setup(model(name).n, km=KM[name] if km else 0.0, box=box, narrow=variant == "narrow", ks=ks)


@functools.lru_cache(maxsize=None)
def step_case(case, rows=ROWS):
    """-> (ets, q, Tep, setup, reference dict, drawn, replaced: {reason: count}) of one step with gain_of(case) and THRESHOLD; arrays read-only"""
    name, method, km, box, variant = case
    su = setup_of(case)
    n = model(name).n
    cand, good, rng = _candidates(name, variant == "narrow", rows, "step", method, km, box)
    keep, teps, replaced, drawn = [], [], dict(cond=0, empty=0, degenerate=0, near=0), 0
    for i in range(cand.shape[0]):
        drawn += 1
        u = rng.uniform(-1.0, 1.0, n)
        Tep = fkine(name, (cand[i] + STEP_DELTAS[len(keep) % 2] * u / np.abs(u).max())[None])[0]
        if not good[i]:
            replaced["cond"] += 1
            continue
        r = _step(name, method, cand[i], Tep, gain_of(case), su)
        if r["empty"] or r["degenerate"]:
            replaced["empty" if r["empty"] else "degenerate"] += 1
            continue
        if abs(r["s"] - THRESHOLD) <= 1e-9 * THRESHOLD:          # `arrived` is compared on every row: decided by more than rounding
            replaced["near"] += 1
            continue
        keep.append(i)
        teps.append(Tep)
        if len(keep) == rows:
            break
    assert len(keep) == rows, (case, "too few acceptable draws")
    q, Tep = np.ascontiguousarray(cand[keep]), np.ascontiguousarray(teps)
    ref = reference(name, method, q, Tep, gain_of(case), THRESHOLD, 0.0, 1, su)
    assert not (ref["status"] & 1).any() and not ref["degenerate"].any() and not ref["near"].any()
    for a in (q, Tep):
        a.setflags(write=False)
    return model(name).ets, q, Tep, su, ref, drawn, replaced


def step_bound(ref):
    """per row: eps c scale of the module docstring (without K)"""
    f = ref["first"]
    c = np.array([max(r["cond"] ** 2, r["cF"]) for r in f])
    scale = np.array([max(np.abs(r["qd"]).max(), np.abs(r["g"]).max()) for r in f])
    return EPS * c * scale


def step_ratio(got, ref):
    return np.abs(np.asarray(got) - ref["qd"]).max(axis=1) / step_bound(ref)


@functools.lru_cache(maxsize=None)
def loop_case(name, method, rows=ROWS):
    """-> (ets, q, Tep, setup, reference dict, replaced) of the loop: STEPS iterations with GAIN_LOOP, DT, THRESHOLD; row i is of kind i % 3 --
    arrived at the first evaluation, arrived after two or more steps, not arrived in STEPS -- chosen on the oracle's own trajectories"""
    n = model(name).n
    su = Setup(n, km=KM[name])
    per = (rows + 2) // 3
    pool = 6 * per
    picked, replaced = [], 0
    for kind in range(3):
        cand, good, rng = _candidates(name, False, pool, "loop", method, kind)
        q = cand[good][:pool]
        d = np.array([LOOP_DELTAS[kind] * u / np.abs(u).max() for u in rng.uniform(-1.0, 1.0, (q.shape[0], n))])
        Tep = np.array(fkine(name, q + d))
        ref = reference(name, method, q, Tep, GAIN_LOOP, THRESHOLD, DT, STEPS, su)
        ok = ~ref["near"] & (ref["status"] == 0) & ~ref["degenerate"] & (ref["cond"] <= COND_MAX)
        ok &= [ref["arrived"] & (ref["its"] == 1), ref["arrived"] & (ref["its"] >= 2), ~ref["arrived"]][kind]
        idx = np.flatnonzero(ok)
        amp = amplification(name, method, q[idx], Tep[idx], su, {k: ref[k][idx] for k in ("q", "its", "arrived", "status")})
        good_idx = idx[amp <= AMP_MAX][:per]
        assert good_idx.size == per, (name, method, kind, "too few acceptable candidates", int(ok.sum()))
        replaced += int(good_idx[-1]) + 1 - per
        picked.append((q[good_idx], Tep[good_idx]))
    order = [(i % 3, i // 3) for i in range(rows)]
    q, Tep = (np.ascontiguousarray([picked[k][a][j] for k, j in order]) for a in range(2))
    ref = reference(name, method, q, Tep, GAIN_LOOP, THRESHOLD, DT, STEPS, su)
    assert not ref["near"].any() and not ref["status"].any()
    ref["amp"] = np.maximum(1.0, amplification(name, method, q, Tep, su, ref))
    assert (ref["amp"] <= AMP_MAX).all()
    for a in (q, Tep):
        a.setflags(write=False)
    return model(name).ets, q, Tep, su, ref, replaced


def loop_ratio(got, ref):
    return rc.ratio(got, ref["q"], ref["cond"]) / ref["amp"]


UNSOLVABLE_ROW, UNSOLVABLE_JOINT = 5, 1


@functools.lru_cache(maxsize=None)
def unsolvable_case(name, method=1):
    """the plain step case of `name` with one row's joint put past its upper limit by 1.7 rad: the damper asks for a retreat of
    (1.7 + ps) / (pi - ps) = 2.06 rad/s, the velocity box allows 2.0 -- the box is empty -> (ets, q, Tep, setup, reference of one step)"""
    case = (name, method, True, True, "plain")
    ets, q, Tep, su, ref, _, _ = step_case(case)
    q = np.array(q)
    q[UNSOLVABLE_ROW, UNSOLVABLE_JOINT] = QLIM + 1.7
    ref = reference(name, method, q, Tep, gain_of(case), THRESHOLD, 0.0, 1, su)
    assert ref["status"][UNSOLVABLE_ROW] == 1 and ref["first"][UNSOLVABLE_ROW]["empty"] and not np.delete(ref["status"], UNSOLVABLE_ROW).any()
    q.setflags(write=False)
    return ets, q, Tep, su, ref


SLACK_ROWS = 8


@functools.lru_cache(maxsize=None)
def slack_case(name="panda", method=1):
    """status bit 1: the plain no-box case of `name` with its gains times 40 -- v is far beyond what the slack's weight lets the arm follow, so the
    oracle's slack is well past 10 on some rows (asserted: above 20) and well clear of it on all (none within 10 +- 1)
    -> (ets, q, Tep, setup, gain6, reference of one step)"""
    case = (name, method, True, False, "plain")
    ets, q, Tep, su, _, _, _ = step_case(case)
    gain6 = tuple(40.0 * g for g in gain_of(case))
    keep = []
    for i in range(q.shape[0]):
        r = _step(name, method, q[i], Tep[i], gain6, su)
        if not r["empty"] and not r["degenerate"] and abs(r["slack"] - SLACK_MAX) > 1.0:
            keep.append(i)
    keep = keep[:SLACK_ROWS]
    assert len(keep) == SLACK_ROWS
    q, Tep = np.ascontiguousarray(q[keep]), np.ascontiguousarray(Tep[keep])
    ref = reference(name, method, q, Tep, gain6, THRESHOLD, 0.0, 1, su)
    assert (ref["slack"] > 20.0).any() and ((ref["status"] == 2) == (ref["slack"] > SLACK_MAX)).all() and not (ref["status"] & 1).any()
    for a in (q, Tep):
        a.setflags(write=False)
    return ets, q, Tep, su, gain6, ref
