"""Shared by tests/test_vjp_census.py and the CPU replays tests/test_*_vjp_emu.py (not a test module): the robots that take the six fused adjoint
kernel families -- k_rne_vjp (fp64 and float32), k_tree_rne_vjp, k_inertia_vjp, k_tree_inertia_vjp, k_coriolis_vjp, k_tree_coriolis_vjp -- through
the instantiations and the size classes that the zoo of the sibling modules (rne_vjp_cases, tree_rne_vjp_cases, inertia_vjp_cases,
coriolis_vjp_cases) leaves out.  The robots' recipes, the input distributions, the stencil, its step and the bound are the siblings'.

DH robots, rne_vjp_cases.random_robot(n, mdh, 100 + 2 n + mdh), both conventions:
    every family   n = 4, 6, 7 (register forms the zoo has in one convention only, or not at all), 10, 13, 15 (run-time n)
    rne_vjp also   n = 16, 23, 24 (the tile passes 48 KB between them: 47 616 and 49 664 bytes), 31, 32 (the stride turns even: exactly 64 KiB)
Structured DH robots -- the random tables have "nothing special about them"; these have exact zeros and special angles, Tc = 0 throughout (so qd
may hold exact zeros), offset = 0 (so a q of k pi / 2 IS the joint angle), and two of them B = 0, Jm = 0, G = 1:
    planar4s   a planar 4R arm, standard DH: every alpha = 0, every d = 0                                              (B = Jm = 0, G = 1)
    ortho4m    4 joints, modified DH: alpha in {0, +-pi/2}, a = 0 and d = 0 alternating
    wrist6m    6 joints, modified DH, a spherical wrist; wrist link 4 is massless with a zero inertia tensor and r = 0  (B = Jm = 0, G = 1)
    ortho7s    7 joints, standard DH: alpha = +-pi/2 throughout, links 2 and 5 with a = d = 0
Their q is drawn as the siblings draw it, then rows 3, 40 and 64 of every 65 are set to exact multiples of pi / 2 (0 included); qd is exactly 0
in row 17 of every 65 and in column r mod n of every row r = 2 mod 7.

Trees, tree_rne_vjp_cases.random_tree(default_rng(seed), n_links) through ERobot: 2, 4 (register forms), 10, 12, 20, 24 groups (run-time n; 24
serves tree_rne_vjp only, the other two families stop at 20).  What each seed gives is asserted in tree_robot().

Rows: a DH case has 65 distinct rows.  A tree case has R distinct rows repeated cyclically to 65 (tree_rne_vjp_cases.tiled): the tree oracles are
Python loops.  R = 4 for tree_rne_vjp and for inertia up to 12 groups, R = 2 for inertia at 20 groups and Coriolis at 10 and 12 groups, R = 4 for
Coriolis at 2 and 4 groups.  Tree Coriolis at 20 groups costs 38 s of oracle per row: that case has none, and the device test holds it to the
composition of 2 n tree_rne_vjp launches on 65 distinct rows instead (tests/test_vjp_census.py)."""
import functools
import math

import numpy as np

import rne_vjp_cases as dh_cases
import tree_rne_vjp_cases as tree_cases
import inertia_vjp_cases as inertia_cases
import coriolis_vjp_cases as coriolis_cases
from rne_vjp_cases import random_robot, richardson, rel_err, H, BOUND        # the same robots, the same stencil, the same bound
from tree_rne_vjp_cases import random_tree, dfs, _props, tiled
from rtbhip import ERobot
from rtbhip.dh import DHRobot, RevoluteDH, RevoluteMDH

N = 65                                    # one full tile and a one-row ragged tile
DH_N = (4, 6, 7, 10, 13, 15)              # every family
RNE_N = (16, 23, 24, 31, 32)              # rne_vjp alone: the two LDS thresholds
RNE_SIZES = {4: (1, 130), 32: (1, 130)}   # rne_vjp at n = 4 and n = 32 also runs at these N

HP = math.pi / 2


def _inertia(rng):
    A = rng.uniform(-1, 1, (3, 3))
    return 0.05 * (A @ A.T) + 0.02 * np.eye(3)


def _structured(name, mdh, rows, bare, seed, massless=()):
    """rows: (alpha, a, d) per link.  bare: B = Jm = 0, G = 1.  massless: links with m = 0, I = 0, r = 0.  Tc = 0 and offset = 0 everywhere"""
    rng = np.random.default_rng(seed)
    links = []
    for j, (alpha, a, d) in enumerate(rows):
        kw = dict(alpha=alpha, a=a, d=d, offset=0.0, m=rng.uniform(0.5, 3.0), r=rng.uniform(-0.2, 0.2, 3), I=_inertia(rng), Tc=[0.0, 0.0])
        kw.update(dict(Jm=0.0, G=1.0, B=0.0) if bare else dict(Jm=rng.uniform(1e-4, 5e-4), G=rng.uniform(-60, 60), B=rng.uniform(1e-4, 2e-3)))
        if j in massless:
            kw.update(m=0.0, r=np.zeros(3), I=np.zeros((3, 3)))
        links.append((RevoluteMDH if mdh else RevoluteDH)(**kw))
    return DHRobot(links, name=name)


STRUCTURED = {
    "planar4s": lambda: _structured("planar4s", 0, [(0.0, 0.4, 0.0), (0.0, 0.3, 0.0), (0.0, 0.25, 0.0), (0.0, 0.1, 0.0)], True, 501),
    "ortho4m": lambda: _structured("ortho4m", 1, [(0.0, 0.0, 0.3), (-HP, 0.25, 0.0), (HP, 0.0, 0.2), (0.0, 0.15, 0.0)], False, 502),
    "wrist6m": lambda: _structured("wrist6m", 1, [(0.0, 0.0, 0.35), (-HP, 0.0, 0.0), (0.0, 0.4, 0.1), (-HP, 0.03, 0.38), (HP, 0.0, 0.0), (-HP, 0.0, 0.0)],
                                   True, 503, massless=(4,)),
    "ortho7s": lambda: _structured("ortho7s", 0, [(HP, 0.0, 0.33), (-HP, 0.1, 0.0), (HP, 0.0, 0.0), (-HP, 0.05, 0.3), (HP, 0.0, 0.2), (-HP, 0.0, 0.0),
                                                  (HP, 0.08, 0.1)], False, 504),
}


def _generic(ns):
    return {"n%d%s" % (n, "m" if m else "s"): (lambda n=n, m=m: random_robot(n, m, 100 + 2 * n + m)) for n in ns for m in (0, 1)}


DH_ROBOTS = dict(_generic(DH_N + RNE_N))
DH_ROBOTS.update(STRUCTURED)
DH_ALL = sorted(_generic(DH_N)) + sorted(STRUCTURED)          # inertia_vjp and coriolis_vjp
RNE_ALL = sorted(_generic(DH_N + RNE_N)) + sorted(STRUCTURED)
# the sibling zoo's random tables, named here for their float32 run alone (f32 against rounded fp64 needs no oracle): tests/test_rne_vjp.py runs
# float32 on puma560, panda and n9m only
RNE_F32_ZOO = sorted(k for k in dh_cases.ROBOTS if k not in ("puma560", "panda"))

# name -> (seed, links drawn, joints = link groups, serial chain?): what the seed gives is asserted in tree_robot()
TREES = {"t2": (13, 3, 2, True), "t4": (1, 4, 4, False), "t10": (11, 10, 10, False), "t12": (11, 12, 12, False), "t20": (24, 21, 20, False),
         "t24": (24, 25, 24, False),
         # 20 groups again, for the tree inertia adjoint's tile alone: 230 doubles a row and 18 per branch slot against the 320 per lane a CU
         # holds.  t20 and t20b have five slots (the even stride, exactly 160 KiB), t20w has six and is refused
         "t20b": (17, 22, 20, False), "t20w": (2, 22, 20, False)}
TREE_RNE_ALL = ("t2", "t4", "t10", "t12", "t20", "t24")
TREE_INERTIA_ALL = ("t2", "t4", "t10", "t12", "t20", "t20b")
TREE_CORIOLIS_ALL = ("t2", "t4", "t10", "t12", "t20")
TREE_RNE_ROWS = {k: 4 for k in TREE_RNE_ALL}
TREE_INERTIA_ROWS = {"t2": 4, "t4": 4, "t10": 4, "t12": 4, "t20": 2, "t20b": 2}
TREE_CORIOLIS_ROWS = {"t2": 4, "t4": 4, "t10": 2, "t12": 2, "t20": None}          # None: no oracle, the composition on 65 distinct rows


@functools.lru_cache(maxsize=None)
def dh_robot(name):
    return DH_ROBOTS[name]()


@functools.lru_cache(maxsize=None)
def tree_robot(name):
    """(ERobot, the oracle's link list)"""
    seed, n_links, n, serial = TREES[name]
    prod, orc = random_tree(np.random.default_rng(seed), n_links)
    rob = ERobot(prod, name=name)
    p = _props(rob)
    assert rob.n == n and p["serial"] == serial and p["pris"] < rob.n and rob._in_group_order(), (name, rob.n, p)
    assert p["pris"] >= 1 and p["flip"] >= 1, (name, p)          # (t2 too: serial, one prismatic group, two flipped joints, a static link with mass)
    return rob, dfs(orc)


def _special(name, q, qd=None):
    """the structured robots' exact inputs, written into fresh draws (see the module's docstring)"""
    if name not in STRUCTURED:
        return q, qd
    rng = np.random.default_rng(900 + sum(map(ord, name)))
    q = np.array(q)
    rows = np.arange(q.shape[0])
    for r in rows[np.isin(rows % 65, (3, 40, 64))]:
        q[r] = HP * rng.integers(-2, 3, q.shape[1])
    q[rows[rows % 65 == 3][:1], 0] = 0.0
    q.setflags(write=False)
    if qd is not None:
        qd = np.array(qd)
        qd[rows % 65 == 17] = 0.0
        for r in rows[rows % 7 == 2]:
            qd[r, r % q.shape[1]] = 0.0
        qd.setflags(write=False)
    return q, qd


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ rne_vjp
def rne_inputs(name, n_rows=N):
    """(robot, q, qd, qdd, gtau), n_rows distinct rows, read-only.  The sibling's seed rule: 7000 + 13 N + sum(ord(name))"""
    rb = dh_robot(name) if name in DH_ROBOTS else dh_cases.robot(name)
    q, qd, qdd, g = dh_cases.draw(rb, n_rows, 7000 + 13 * n_rows + sum(map(ord, name)))
    q, qd = _special(name, q, qd)
    return rb, q, qd, qdd, g


@functools.lru_cache(maxsize=None)
def rne_case(name, n_rows=N, h=H):
    """(robot, q, qd, qdd, gtau, [gq, gqd, gqdd] of the oracle): computed once, shared, never written to"""
    rb, q, qd, qdd, g = rne_inputs(name, n_rows)
    ref = dh_cases.rne_oracle(rb, q, qd, qdd, g, h=h)
    _frozen(*ref)
    return rb, q, qd, qdd, g, ref


# ------------------------------------------------------------------------------------------------ tree_rne_vjp
@functools.lru_cache(maxsize=None)
def tree_rne_case(name, h=H):
    """(robot, link list, q, qd, qdd, gtau, gravity, [gq, gqd, gqdd] of the oracle) of TREE_RNE_ROWS[name] rows"""
    rob, orc = tree_robot(name)
    q, qd, qdd, g = tree_cases.draw(rob.n, 9000 + sum(map(ord, name)), rows=TREE_RNE_ROWS[name])
    gravity = tree_cases.gravity_of(rob, "plain")
    ref = tree_cases.rne_oracle(orc, q, qd, qdd, g, gravity, h=h)
    _frozen(*ref)
    return rob, orc, q, qd, qdd, g, gravity, ref


# ------------------------------------------------------------------------------------------------ inertia_vjp, tree_inertia_vjp
@functools.lru_cache(maxsize=None)
def inertia_dh_case(name, h=H):
    """(robot, q, gM, gq of the oracle), 65 distinct rows"""
    rb = dh_robot(name)
    q, g = inertia_cases.draw(rb.n, N, inertia_cases._seed(name, N))
    q, _ = _special(name, q)
    ref, = _frozen(inertia_cases.dh_oracle(rb, q, g, h=h))
    return rb, q, g, ref


@functools.lru_cache(maxsize=None)
def inertia_tree_case(name, h=H):
    """(robot, link list, q, gM, gq of the oracle) of TREE_INERTIA_ROWS[name] rows"""
    rob, orc = tree_robot(name)
    rows = TREE_INERTIA_ROWS[name]
    q, g = inertia_cases.draw(rob.n, rows, inertia_cases._seed(name, rows))
    ref, = _frozen(inertia_cases.tree_oracle(orc, q, g, h=h))
    return rob, orc, q, g, ref


# ------------------------------------------------------------------------------------------------ coriolis_vjp, tree_coriolis_vjp
def coriolis_dh_batched(rb):
    """oracle.coriolis_dh (Dynamics.coriolis, statement for statement) with its inverse-dynamics calls gathered: the reference's rne is evaluated
    row by row inside ONE call for the n unit velocities and ONE for the n (n - 1) / 2 pairs of every configuration, instead of one call each,
    and the sums are formed in the reference's order, a whole batch per statement.  The same numbers bit for bit
    (tests/test_vjp_census.py::test_the_batched_coriolis_reference_is_the_reference), about fifty times sooner: the stencil of a 15-joint table on
    65 rows asks for 60 Coriolis matrices of 120 inverse-dynamics evaluations each, per row"""
    from oracle import oracle
    L, mdh, n = oracle.nofriction_L24(rb.L24()), rb.mdh, rb.n
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    unit = np.eye(n)
    both = np.array([unit[i] + unit[j] for i, j in pairs]).reshape(len(pairs), n)

    def C(q, qd):
        q, qd = np.asarray(q, dtype=np.float64).reshape(-1, n), np.asarray(qd, dtype=np.float64).reshape(-1, n)
        rows = q.shape[0]
        rne = lambda QD: oracle.rne_dh(L, mdh, np.repeat(q, QD.shape[0], axis=0), np.tile(QD, (rows, 1)), np.zeros((rows * QD.shape[0], n)),
                                       [0, 0, 0]).reshape(rows, QD.shape[0], n)
        Cm = np.zeros((rows, n, n))
        Csq = np.zeros((rows, n, n)) + rne(unit).transpose(0, 2, 1)          # Csq[k, :, i] = tau(q_k, e_i)
        tau = rne(both) if pairs else None
        for p, (i, j) in enumerate(pairs):
            Cm[:, :, j] = Cm[:, :, j] + (tau[:, p] - Csq[:, :, j] - Csq[:, :, i]) * qd[:, i, None] / 2
            Cm[:, :, i] = Cm[:, :, i] + (tau[:, p] - Csq[:, :, j] - Csq[:, :, i]) * qd[:, j, None] / 2
        for k in range(rows):
            Cm[k] = Cm[k] + Csq[k] @ np.diag(qd[k])
        return Cm
    return C


@functools.lru_cache(maxsize=None)
def coriolis_dh_case(name, h=H):
    """(robot, q, qd, gC, gq and gqd of the oracle), 65 distinct rows.  coriolis_vjp_cases.dh_oracle with the batched reference in place of
    oracle.coriolis_dh: the stencil for gq, the exact linearity in qd for gqd"""
    rb = dh_robot(name)
    q, qd, g = coriolis_cases.draw(rb.n, N, coriolis_cases._seed(name))
    q, qd = _special(name, q, qd)
    Cref = coriolis_dh_batched(rb)
    rq, rd = _frozen(coriolis_cases._gq(Cref, q, qd, g, h), coriolis_cases._gqd(Cref, q, g))
    return rb, q, qd, g, rq, rd


@functools.lru_cache(maxsize=None)
def coriolis_tree_case(name, h=H):
    """(robot, link list, q, qd, gC, gq and gqd of the oracle) of TREE_CORIOLIS_ROWS[name] rows"""
    rob, orc = tree_robot(name)
    q, qd, g = coriolis_cases.draw(rob.n, TREE_CORIOLIS_ROWS[name], coriolis_cases._seed(name))
    rq, rd = _frozen(*coriolis_cases.tree_oracle(orc, q, qd, g, h=h))
    return rob, orc, q, qd, g, rq, rd


def coriolis_tree_distinct(name, n_rows=N):
    """(robot, q, qd, gC) of n_rows DISTINCT rows from the same distribution, no oracle: for the comparison with the composition"""
    rob, _ = tree_robot(name)
    return (rob,) + coriolis_cases.draw(rob.n, n_rows, coriolis_cases._seed(name) + 1)


# ------------------------------------------------------------------------------------------------ what is named, for the census
# The largest joint / group count with a register form of its own, as it stood when the robots were filed: a robot beyond it is filed under the
# run-time-n form.  tests/test_vjp_census.py holds this against the `case` labels of the six launchers -- a label added there needs a robot here.
FILED_REGISTER_MAX = {"rne_vjp": 8, "inertia_vjp": 8, "coriolis_vjp": 7, "tree_rne_vjp": 8, "tree_inertia_vjp": 8, "tree_coriolis_vjp": 8}


def named():
    """{family: set of keys} over the sibling zoo and this table.  A key is (form, n) for the three tree families, (form, n, mdh) for inertia_vjp
    and coriolis_vjp, (form, n, mdh, "f64" | "f32") for rne_vjp; form is "reg" up to FILED_REGISTER_MAX, "rt" beyond.  hand4 is left out of the
    inertia and Coriolis families: their raw entry points refuse a hand-numbered tree.  A robot is built to read its n: no oracle runs"""
    form = lambda fam, n: "reg" if n <= FILED_REGISTER_MAX[fam] else "rt"
    dh = lambda fam, rb: (form(fam, rb.n), rb.n, int(bool(rb.mdh)))
    tree = lambda fam, n: (form(fam, n), n)
    out = {}
    f = "rne_vjp"
    out[f] = {dh(f, dh_cases.robot(k)) + ("f64",) for k in dh_cases.ROBOTS} | {dh(f, dh_cases.robot(k)) + ("f32",) for k in ("puma560", "panda", "n9m")}
    out[f] |= {dh(f, dh_robot(k)) + (s,) for k in RNE_ALL for s in ("f64", "f32")} | {dh(f, dh_cases.robot(k)) + ("f32",) for k in RNE_F32_ZOO}
    for f, zoo in (("inertia_vjp", inertia_cases), ("coriolis_vjp", coriolis_cases)):
        out[f] = {dh(f, zoo.dh_robot(k)) for k in zoo.DH_ROBOTS} | {dh(f, dh_robot(k)) for k in DH_ALL}
    for f, zoo, mine in (("tree_rne_vjp", tree_cases.ROBOTS, TREE_RNE_ALL), ("tree_inertia_vjp", inertia_cases.TREES, TREE_INERTIA_ALL),
                         ("tree_coriolis_vjp", coriolis_cases.TREES, TREE_CORIOLIS_ALL)):
        out[f] = {tree(f, tree_cases.robot(k)[0].n) for k in zoo} | {tree(f, TREES[k][2]) for k in mine}
    return out
