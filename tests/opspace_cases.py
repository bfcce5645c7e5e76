"""Shared by tests/test_opspace.py and tests/test_opspace_emu.py (not a test module): the robots, the inputs and the ORACLE of the
operational-space dynamics (rtbhip_opspace / rtbhip_tree_opspace).

Oracle (float64), each row with the reference's single-q formula (robot/Dynamics.py:1000-1009, 1260-1269; robot/Robot.py:871-881):

    Ji = numpy.linalg.inv(J) for six joints, numpy.linalg.pinv(J) otherwise
    Mx = Ji.T @ M @ Ji,   Gx = Ji.T @ g
    asada = 0 if matrix_rank(J) < 6 else min(e) / max(e), e = numpy.linalg.eig of the selected rows and columns of Mx

with M from oracle.inertia_dh / oracle.erobot.erobot_inertia, g from oracle.rne_dh / erobot_rne at qd = qdd = 0 and J from oracle.jacob0 on the
robot's own chain.  It shares nothing with the kernel: no LDL^T, no Gram matrix, no Jacobi sweeps.

Inputs: q ~ U(-3, 3), seeded; a row is redrawn while cond(J) > 1e3, and at most one third of the draws may be replaced (asserted when the case is
built, counted on the oracle's Jacobian alone).  The branched tree has no single path through all its joints: its J is a seeded (6, n) matrix
with entries ~ U(-1, 1), under the same condition rule -- the entry point takes any Jacobian.

Bound, per row, for the device and for the CPU replay:  K eps cond(J)^2 max|ref|  (X enters twice).  For the Asada ratio the reference
magnitude is 1: the ratio is lambda_min measured in units of lambda_max, and lambda_min carries the absolute error of Mx, eps cond(J)^2 |Mx|max
~ eps cond(J)^2 lambda_max.  K = 8 x the largest err / (eps cond(J)^2 max|ref|) the CPU replay shows over all cases (tests/test_opspace_emu.py
prints it; DESIGN.md records it); the factor 8 covers the device compiler's different but contraction-free evaluation of the same source.

The modified-DH chain with a prismatic FIRST joint has a non-symmetric M (the reference's recursion: DESIGN.md); Mx and Gx are held to the oracle
there, Asada's measure is not compared: the kernel symmetrises the block, a general eig of a matrix that is not symmetric answers another question."""
import functools

import numpy as np

import rtbhip
from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH, RevoluteMDH, PrismaticMDH
from oracle import oracle, erobot as oer
from helpers import chain_from_ets
import rne_vjp_cases as dhc
import tree_rne_vjp_cases as trc

EPS = 2.220446049250313e-16
COND_MAX = 1e3
ROWS = 16
K_MEASURED = 3.17         # the largest err / (eps cond(J)^2 max|ref|) of the CPU replay over every case and output: 3.163 on tree7, 3.147 on n9s
                          # (the Gram paths; the LU path stays below 0.08) -- test_opspace_emu.py prints every figure
K = 8.0 * K_MEASURED
AXES = {"all": 63, "trans": 7, "rot": 56}
GRAVITY = np.array([0.4, -1.1, -9.0])

DH = ["puma560", "panda", "n3s", "n8m", "n9s", "n16s", "pris6", "mdhp6"]
TREES = ["UR5", "KinovaGen3", "tree7"]
ALL = DH + TREES
REFUSED = "hand4"
NONSYMMETRIC = ("mdhp6",)


def with_prismatic(n, mdh, which, seed):
    """dhc.random_robot's recipe with joint `which` prismatic"""
    rng = np.random.default_rng(seed)
    links = []
    for j in range(n):
        A = rng.uniform(-1, 1, (3, 3))
        I = 0.05 * (A @ A.T) + 0.02 * np.eye(3)
        dyn = dict(m=rng.uniform(0.5, 3.0), r=rng.uniform(-0.2, 0.2, 3), I=I, Jm=rng.uniform(1e-4, 5e-4), G=rng.uniform(-60, 60),
                   B=rng.uniform(1e-4, 2e-3), Tc=[rng.uniform(0.1, 0.5), -rng.uniform(0.1, 0.5)])
        geo = dict(a=rng.uniform(-0.4, 0.4), alpha=rng.uniform(-1.5, 1.5), offset=rng.uniform(-0.5, 0.5))
        if j == which:
            links.append((PrismaticMDH if mdh else PrismaticDH)(theta=rng.uniform(-1, 1), **geo, **dyn))
        else:
            links.append((RevoluteMDH if mdh else RevoluteDH)(d=rng.uniform(-0.4, 0.4), **geo, **dyn))
    return DHRobot(links, name="pris%d%s" % (n, "m" if mdh else "s"))


@functools.lru_cache(maxsize=None)
def _tree(name):
    """(ERobot, the oracle's link list).  KinovaGen3: the arm alone -- the gripper's subtree left out, as the reference removes gripper links
    from robot.links -- so that the path to the last link moves all 7 joints (with its six finger joints the robot has 13)"""
    if name != "KinovaGen3":
        return trc.robot(name)
    er = rtbhip.urdf.load(name).erobot(("robotiq_arg2f_base_link",))
    orc = []
    for l in er.links:                                        # (tree_rne_vjp_cases._urdf: er.links is already in depth-first order)
        items = [(e.axis, None, e.isflip) if e.isjoint else np.array(e.T) for e in l.ets]
        orc.append(dict(name=l.name, parent=None if l.parent is None else l.parent.name, ets=items, m=l.m, r=l.r))
    return er, orc


@functools.lru_cache(maxsize=None)
def robot(name):
    if name in ("puma560", "panda", "n3s", "n8m", "n9s"):
        return dhc.robot(name)
    if name == "n16s":
        return dhc.random_robot(16, 0, 132)
    if name == "pris6":
        return with_prismatic(6, False, 2, 41)
    if name == "mdhp6":
        return with_prismatic(6, True, 0, 43)
    return _tree(name)[0]


def is_tree(name):
    return name in TREES or name == REFUSED


def gravity3(name):
    """what the raw entry point is handed as grav3"""
    rb = robot(name)
    return np.ascontiguousarray(GRAVITY) if is_tree(name) else rb._gravity_c(GRAVITY)


def inertia(name, q):
    rb = robot(name)
    if is_tree(name):
        return oer.erobot_inertia(_tree(name)[1], q)
    return oracle.inertia_dh(rb.L24(), rb.mdh, q)


def gravload(name, q):
    rb = robot(name)
    z = np.zeros_like(q)
    if is_tree(name):
        return oer.erobot_rne(_tree(name)[1], q, z, z, GRAVITY)
    return oracle.rne_dh(rb.L24(), rb.mdh, q, z, z, gravity3(name))


@functools.lru_cache(maxsize=None)
def end_link(name):
    """a tree's link whose path from the base moves every joint (None for a DH arm: its tool frame)"""
    if not is_tree(name):
        return None
    rb = robot(name)
    for l in reversed(rb.links):
        if rb.ets(None, l).n == rb.n:
            return l
    raise ValueError("no path of %s moves all its joints" % name)


@functools.lru_cache(maxsize=None)
def _chain(name):
    rb = robot(name)
    return chain_from_ets(rb.ets(None, end_link(name)) if is_tree(name) else rb.ets())


def has_path(name):
    return name != "tree7"


def jacob0(name, q, representation=None):
    ch = _chain(name)
    return oracle.jacob0(ch, q) if representation is None else oracle.jacob0_analytical(ch, q, representation)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(q (ROWS, n), J (ROWS, 6, n), draws, replaced): fixed seed, read-only"""
    n = robot(name).n
    rng = np.random.default_rng(8000 + sum(ord(c) for c in name))
    cand = rng.uniform(-3.0, 3.0, (6 * ROWS, n))
    Jc = jacob0(name, cand) if has_path(name) else rng.uniform(-1.0, 1.0, (6 * ROWS, 6, n))
    keep, replaced = [], 0
    for i in range(cand.shape[0]):
        if np.linalg.cond(Jc[i]) > COND_MAX:
            replaced += 1
            continue
        keep.append(i)
        if len(keep) == ROWS:
            break
    assert len(keep) == ROWS, (name, "too few well-conditioned draws")
    draws = ROWS + replaced
    q, J = np.ascontiguousarray(cand[keep]), np.ascontiguousarray(Jc[keep])
    q.setflags(write=False); J.setflags(write=False)
    return q, J, draws, replaced


def formula(M, g, J, axes=63):
    """one row with the reference's single-q formula -> (Mx, Gx, asada)"""
    Ji = np.linalg.inv(J) if J.shape[1] == 6 else np.linalg.pinv(J)
    Mx, Gx = Ji.T @ M @ Ji, Ji.T @ g
    if np.linalg.matrix_rank(J) < 6:
        return Mx, Gx, 0.0
    d = [r for r in range(6) if (axes >> r) & 1]
    e = np.linalg.eig(Mx[d][:, d])[0]
    return Mx, Gx, float(np.real(np.min(e) / np.max(e)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """{"Mx": (ROWS, 6, 6), "Gx": (ROWS, 6), "all" / "trans" / "rot": (ROWS,), "cond": (ROWS,)}: computed once, read-only"""
    q, J, _, _ = inputs(name)
    M, g = inertia(name, q), gravload(name, q)
    out = {"Mx": np.zeros((ROWS, 6, 6)), "Gx": np.zeros((ROWS, 6)), "cond": np.array([np.linalg.cond(Ji) for Ji in J])}
    for key in AXES:
        out[key] = np.zeros(ROWS)
    for i in range(ROWS):
        for key, mask in AXES.items():
            out["Mx"][i], out["Gx"][i], out[key][i] = formula(M[i], g[i], J[i], mask)
    for a in out.values():
        a.setflags(write=False)
    return out


def tiled(x, N):
    return np.ascontiguousarray(x[np.arange(N) % x.shape[0]])


def ratio(got, ref, cond, unit=False):
    """the largest err / (eps cond^2 max|ref|) over the rows; unit: the reference magnitude is 1 (the Asada ratio)"""
    got, ref = np.asarray(got).reshape(len(cond), -1), np.asarray(ref).reshape(len(cond), -1)
    scale = np.ones(len(cond)) if unit else np.abs(ref).max(axis=1)
    return float((np.abs(got - ref).max(axis=1) / (EPS * cond ** 2 * scale)).max())
