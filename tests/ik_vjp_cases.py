"""Shared by tests/test_ik_vjp.py and tests/test_ik_vjp_emu.py (not a test module): the chains, the masks, the inputs and the ORACLE of the
implicit-function adjoint of the inverse kinematics (rtbhip_ik_vjp).

Oracle (float64): the Jacobian of the case's chain from the compiled reference restated in oracle/ (oracle.jacob0; the PoE robot's from the closed
form of oracle/poe.py) and numpy.linalg.solve, restating the definition: with a the rows whose mask weight is not zero and d the damping

    y_a = (J_a J_a^T + d^2 I)^-1 J_a gq,   y = 0 elsewhere           gtwist = y
    gTep[:3, 3] = y_v,   gTep[:3, :3] = 1/2 [y_w]x R_p,   bottom row 0

It shares nothing with the kernel: no LDL^T, no identity embedding, LAPACK's pivoted LU on the a x a system.

Inputs: q is drawn, Tep = fkine(q) from the oracle (so q IS a solution, no solve needed), gq ~ U(-1, 1).  Chains of 6 joints and more run undamped:
a draw with cond(J_a J_a^T) > 1e4 for the full or the translation mask is replaced by the next one, and at most one third of the draws may be
replaced (asserted when the case is built).  Chains of fewer than 6 joints use masks of at most n rows and d = 0.1: positive definite whatever the
geometry.

Bound, for the device and for the CPU replay of the lane body: 1e-9 of the row's largest reference magnitude.  Rounding amplification is about
6 x 2.2e-16 x cond <= 1.4e-11, which leaves roughly 70x for the other compiler's contraction choices and for the oracle's own solve."""
import functools

import numpy as np

from oracle import oracle, chains, poe
from helpers import mixed_spec, product_ets, chain_from_ets
from link_frames_vjp_cases import random_spec, tiled            # (tiled: re-exported for the tests)

BOUND = 1e-9
COND_MAX = 1e4
ROWS = 24
DAMPING_SHORT = 0.1

REG = ["n%d" % n for n in range(1, 11)]                          # one of every register form
ANY = ["n11", "n16", "n32"]                                      # the run-time-n form
ROBOTS = ["panda", "UR5", "prisflip", "poe"]
ALL = REG + ANY + ROBOTS

# random_spec's seed per joint count (100 + n unless listed): a six- or seven-joint chain of mixed joint kinds is often rank-deficient in its
# rotation rows everywhere (two revolute axes) -- these are chains whose uniform draws are mostly well conditioned, picked on the oracle's Jacobian
SEEDS = {6: 402, 7: 292, 9: 146}

_ONE = [("tx", 0.2), ("Rz", None), ("ty", 0.3)]                  # one joint that moves the x row its mask uses

ONES = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
TRANS = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
WEIGHTS = (1.0, 2.0, 0.5, 3.0, 0.25, 1.5)                        # unequal, positive: must give what ONES gives (the weights drop out)


def _short(n, weights=False):
    w = WEIGHTS if weights else ONES
    return tuple(w[r] if r < n else 0.0 for r in range(6))


def masks_of(n):
    """{name: (mask or None = all ones, damping)} of a chain of n joints"""
    if n >= 6:
        return {"ones": (None, 0.0), "trans": (TRANS, 0.0), "weights": (WEIGHTS, 0.0)}
    m = {"short": (_short(n), DAMPING_SHORT), "shortw": (_short(n, True), DAMPING_SHORT)}
    if n >= 3:
        m["trans"] = (TRANS, DAMPING_SHORT)
    return m


def same_answer(mask_name):
    """the mask whose reference a weighted mask must reproduce"""
    return {"weights": "ones", "shortw": "short"}.get(mask_name)


def used_rows(mask):
    return [r for r in range(6) if mask is None or mask[r] != 0.0]


class _Model:
    def __init__(self, ets, fkine, jacob0):
        self.ets, self.fkine, self.jacob0, self.n = ets, fkine, jacob0, ets.n


def _poe_robot():
    import rtbhip
    rng = np.random.default_rng(5)
    S = [poe.unit_revolute(rng.normal(size=3), rng.uniform(-0.5, 0.5, 3)) for _ in range(5)] + [poe.unit_prismatic(rng.normal(size=3))]
    S = [S[0], S[1], S[5], S[2], S[3], S[4]]
    T0 = np.eye(4)
    a = rng.normal(size=3)
    T0[:3, :3] = poe.rodrigues(a / np.linalg.norm(a), rng.uniform(-3, 3))
    T0[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    r = poe.PoE(S, T0)
    links = []
    for s in r.S:
        if np.linalg.norm(s[3:]) == 0.0:
            links.append(rtbhip.PoEPrismatic(s[:3]))
        else:
            links.append(rtbhip.PoERevolute(s[3:], np.cross(s[3:], s[:3])))
    return rtbhip.PoERobot(links, r.T0), r


@functools.lru_cache(maxsize=None)
def model(name):
    """the product's ETS of a case (kept alive: its handle is reused) with the oracle's fkine and jacob0 of the same chain"""
    import rtbhip
    if name == "poe":
        robot, r = _poe_robot()
        m = _Model(robot.ets(), r.fkine, r.jacob0)
        m.robot = robot
        return m
    if name == "panda":
        ets = rtbhip.models.Panda().ets()                        # with its tool: the flange is the chain's last constant
    elif name == "UR5":
        ets = rtbhip.urdf.load("UR5").ets()
    elif name == "prisflip":
        ets = product_ets(mixed_spec())                          # three prismatic joints, three flipped ones
    else:
        n = int(name[1:])
        ets = product_ets(_ONE if n == 1 else random_spec(n, SEEDS.get(n, 100 + n)))
    ch = chain_from_ets(ets)
    return _Model(ets, lambda q: oracle.fkine(ch, q), lambda q: oracle.jacob0(ch, q))


def reference(J, Tep, gq, mask, damping):
    """(gtwist (N, 6), gTep (N, 4, 4)) of the module docstring"""
    N = J.shape[0]
    rows = used_rows(mask)
    tw, gT = np.zeros((N, 6)), np.zeros((N, 4, 4))
    for i in range(N):
        Ja = J[i][rows]
        tw[i, rows] = np.linalg.solve(Ja @ Ja.T + damping * damping * np.eye(len(rows)), Ja @ gq[i])
        w = tw[i, 3:]
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        gT[i, :3, :3] = 0.5 * K @ Tep[i, :3, :3]
        gT[i, :3, 3] = tw[i, :3]
    return tw, gT


def _cond(J, mask):
    Ja = J[used_rows(mask)]
    return np.linalg.cond(Ja @ Ja.T)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(q (ROWS, n), Tep (ROWS, 4, 4), gq (ROWS, n), J (ROWS, 6, n), draws, replaced): fixed seed; read-only"""
    m = model(name)
    n = m.n
    rng = np.random.default_rng(7000 + sum(ord(c) for c in name))
    cand = rng.uniform(-3.0, 3.0, (4 * ROWS, n))
    Jc = m.jacob0(cand)
    keep, replaced = [], 0
    for i in range(cand.shape[0]):
        if n >= 6 and max(_cond(Jc[i], None), _cond(Jc[i], TRANS)) > COND_MAX:
            replaced += 1
            continue
        keep.append(i)
        if len(keep) == ROWS:
            break
    assert len(keep) == ROWS, (name, "too few well-conditioned draws")
    draws = ROWS + replaced
    assert 3 * replaced <= draws, (name, "more than one third of the draws replaced", replaced, draws)
    q = np.ascontiguousarray(cand[keep])
    J = np.ascontiguousarray(Jc[keep])
    Tep = np.ascontiguousarray(m.fkine(q))
    gq = rng.uniform(-1.0, 1.0, (ROWS, n))
    for a in (q, Tep, gq, J):
        a.setflags(write=False)
    return q, Tep, gq, J, draws, replaced


@functools.lru_cache(maxsize=None)
def case(name, mask_name):
    """(ets, q, Tep, gq, mask (6 floats or None), damping, reference gtwist (ROWS, 6), reference gTep (ROWS, 4, 4)); the arrays are read-only"""
    m = model(name)
    mask, damping = masks_of(m.n)[mask_name]
    q, Tep, gq, J, _, _ = inputs(name)
    tw, gT = reference(J, Tep, gq, mask, damping)
    for a in (tw, gT):
        a.setflags(write=False)
    return m.ets, q, Tep, gq, mask, damping, tw, gT


def every_case():
    out = []
    for name in ALL:
        n = 7 if name in ("panda", "prisflip") else 6 if name in ("UR5", "poe") else int(name[1:])
        out += [(name, mk) for mk in masks_of(n)]
    return out


def row_error(got, ref):
    """max over the rows of |got - ref|max / |ref|max of the row"""
    got, ref = np.asarray(got).reshape(ref.shape[0], -1), np.asarray(ref).reshape(ref.shape[0], -1)
    scale = np.abs(ref).max(axis=1)
    assert (scale > 0).all()
    return float((np.abs(got - ref).max(axis=1) / scale).max())


def distinct(name, N, seed=1):
    """(q, Tep, gq) of N DISTINCT rows, no oracle and no conditioning filter: for comparisons of bits and of one device result with another"""
    m = model(name)
    rng = np.random.default_rng(9000 + seed + sum(ord(c) for c in name))
    q = rng.uniform(-3.0, 3.0, (N, m.n))
    return q, np.ascontiguousarray(m.fkine(q)), rng.uniform(-1.0, 1.0, (N, m.n))


def pullback(Tep, gT):
    """NumPy restatement of vjp_pose_pullback without a base: (g_p ; m), m = sum_c R_c x gT_c"""
    R, G = Tep[:, :3, :3], gT[:, :3, :3]
    return np.concatenate([gT[:, :3, 3], np.cross(R, G, axisa=1, axisb=1).sum(axis=1)], axis=1)
