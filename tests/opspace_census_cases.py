"""Shared by tests/test_opspace_census.py and the flush-guard table (not a test module): the robots that take the operational-space kernels
(rtbhip_opspace / rtbhip_tree_opspace) through EVERY instantiation their launchers dispatch and through every launch class, which the zoo of
tests/opspace_cases.py (eight DH robots, three trees: ten of the 80 forms) leaves out.  The oracle, its formula, the input rule and the bound
are that module's; the rows are 97 and DISTINCT.

DH launcher, k_opspace<NJ, MDH, ALLREV>, NJ = 1..16, both conventions, all-revolute or not: 64 forms
    r<n>s / r<n>m   all-revolute: rne_vjp_cases.random_robot(n, mdh, 300 + 2 n + mdh)
    p<n>s / p<n>m   joint n // 2 prismatic: opspace_cases.with_prismatic(n, mdh, n // 2, 500 + 2 n + mdh).  Never the first joint for n >= 2, so M is
                    symmetric and Asada's ratio is compared; at n = 1 it is the only joint, and a 1 x 1 M is symmetric
Tree launcher, k_tree_opspace<NG>, NG = 1..16
    t<n>            tree_rne_vjp_cases.random_tree(default_rng(seed), links): what each seed gives (n groups, branched from 3 groups on, a prismatic
                    group and a flipped joint from 2 groups on, numbered in group order) is asserted in tree_robot()
    lad<n>_<k>      a ladder as the flush-guard table's _ladder8, with exactly k branch slots: group j hangs off group j - 2 for 2 <= j < k + 2 and
                    off group j - 1 beyond; one prismatic and two flipped joints.  The launch classes:
                        lad8_1    the first tree request above 48 KB (hipFuncSetAttribute): 93 + 18 = 111 doubles a row, 56832 bytes
                        lad16_2   265 + 36 = 301 doubles a row, tile 64, 154112 bytes
                        lad16_3   265 + 54 = 319 doubles a row: 163328 bytes, 512 bytes under a compute unit's 160 KB -- still tile 64, the largest
                                  request any robot can make
                        lad16_4   265 + 72 = 337 doubles a row: tile 32, 86272 bytes
                        lad14_6   217 + 108 = 325 doubles a row: a tile-32 tree of 14 groups, 83200 bytes
A tree's J is a seeded (6, n) matrix with entries ~ U(-1, 1): a tree has no single path through all its joints, and the entry point takes any
Jacobian (opspace_cases: tree7).

Inputs: q ~ U(-3, 3); a row is redrawn while cond(J) > 1e3 on the oracle's Jacobian alone, at most one third of the draws (asserted in inputs()).
97 rows: at tile 64 one full tile and 33 rows, at tile 32 three full tiles and one row.

ops_layout and ops_tile_rows of csrc/opspace_device.h are restated below (layout, tile_rows, launch_shape): the expected launch shapes of the device
test and of the CPU replay rest on this copy, and tests/test_opspace_census.py pins nine of its values and holds the replay's own to it.

Bound: K eps cond(J)^2 max|ref| per row (1 for the Asada ratio), K = 8 x the CPU replay's largest ratio.  The replay's largest ratio over the census
cases is K_CENSUS_MEASURED below; where it exceeds opspace_cases.K_MEASURED the census, and only the census, is held at 8 x K_CENSUS_MEASURED."""
import functools

import numpy as np

import opspace_cases as oc
import rne_vjp_cases as dhc
import tree_rne_vjp_cases as trc
from opspace_cases import EPS, COND_MAX, AXES, GRAVITY, formula, ratio
from oracle import oracle, chains, erobot as oer
from helpers import chain_from_ets

ROWS = 97
SIZES = (1, 31, 32, 33, 63, 64, 65, 96)          # every one returns the bits of the leading rows of the 97-row result
# the constants of the launch code as they stood when the robots were filed (tests/test_opspace_census.py reads them from the source text)
MAX_JOINTS, REG_MAX, SLOT_DOUBLES, OUT_W, WAVE, LDS_LIMIT = 16, 8, 18, 43, 64, 160 * 1024

# the largest err / (eps cond(J)^2 max|ref|) of the CPU replay over every census case and mask, against the oracle, per output (Mx, Gx, asada) with
# the case that set it (tests/test_opspace_census.py::test_replay_equals_the_oracle prints every figure and fails when one is exceeded):
#     Mx     30.36  p10m, every mask (the right Gram path; 27.73 on p7s, 27.24 on p11m: rows of cond(J) 16..30, where the allowance eps cond^2 is small)
#     Gx    132.19  r1s (one joint: its gravity torque nearly vanishes on row 28, |Gx| 0.005 against a median of 0.17; every other case stays below 10.1)
#     asada  10.46  p16m / rot
K_CENSUS_BY_OUTPUT = (30.36, 132.19, 10.46)
K_CENSUS_MEASURED = max(K_CENSUS_BY_OUTPUT)
K = 8.0 * max(K_CENSUS_MEASURED, oc.K_MEASURED)                                   # the census's bound
K_OUT = tuple(8.0 * max(k, oc.K_MEASURED) for k in K_CENSUS_BY_OUTPUT)            # and, finer and never wider, each output at 8 x its own figure


# ------------------------------------------------------------------------------------------------ the launch code, restated
def layout(n, packed, q_in_tile):
    """ops_layout -> (wm, q_off, j_off, g_off, stride): [M | q unless it lives in the M tile | J 6 n | g beyond REG_MAX joints], made odd, and never
    shorter than a finished row"""
    wm = n * (n + 1) // 2 if packed else n * n
    q_off = 0 if q_in_tile else wm
    j_off = wm + (0 if q_in_tile else n)
    g_off = j_off + 6 * n
    used = g_off + (n if n > REG_MAX else 0)
    return wm, q_off, j_off, g_off, max(used, OUT_W) | 1


def tile_rows(per_row, limit=LDS_LIMIT):
    """ops_tile_rows: 64 rows, halved while they exceed a compute unit's LDS (never below 8)"""
    t = WAVE
    while t > 8 and per_row * t * 8 > limit:
        t //= 2
    return t


def per_row(n, tree, allrev=True, slots=0):
    """doubles a lane owns: the row of k_opspace<n, ., allrev> (launch_opspace: ops_layout(n, allrev, allrev)) or of k_tree_opspace<n>
    (launch_tree_opspace: ops_layout(n, true, false) and kTreeSlotDoubles per branch slot behind the rows)"""
    if tree:
        return layout(n, True, False)[4] + SLOT_DOUBLES * slots
    return layout(n, allrev, allrev)[4]


def launch_shape(name, N, limit=LDS_LIMIT):
    """what rtbhip.last_launch() must show: (workgroups, threads, LDS bytes)"""
    w = row_doubles(name)
    t = tile_rows(w, limit)
    return (N + t - 1) // t, WAVE, t * w * 8


# ------------------------------------------------------------------------------------------------ the table
def _dh_table():
    out = {}
    for n in range(1, MAX_JOINTS + 1):
        for mdh in (0, 1):
            c = "m" if mdh else "s"
            out["r%d%s" % (n, c)] = (n, mdh, True)
            out["p%d%s" % (n, c)] = (n, mdh, False)
    return out


DH_ROBOTS = _dh_table()          # name -> (n, modified DH?, all-revolute?)
# name -> (seed, links drawn, groups): what the seed gives is asserted in tree_robot()
RANDOM_TREES = {"t1": (0, 1, 1), "t2": (1, 2, 2), "t3": (1, 3, 3), "t4": (3, 5, 4), "t5": (1, 6, 5), "t6": (1, 7, 6), "t7": (1, 8, 7), "t8": (1, 9, 8),
                "t9": (1, 10, 9), "t10": (1, 11, 10), "t11": (5, 12, 11), "t12": (5, 13, 12), "t13": (5, 14, 13), "t14": (17, 15, 14), "t15": (24, 16, 15),
                "t16": (24, 17, 16)}
LADDERS = {"lad8_1": (8, 1), "lad16_2": (16, 2), "lad16_3": (16, 3), "lad16_4": (16, 4), "lad14_6": (14, 6)}          # name -> (groups, branch slots)
# the launch classes a tree must be named for -> (robot, doubles per row, tile, LDS bytes)
TREE_CLASSES = {"8 groups, one slot: first request above 48 KB": ("lad8_1", 111, 64, 56832),
                "16 groups, two slots: tile 64": ("lad16_2", 301, 64, 154112),
                "16 groups, three slots: the largest request, tile 64": ("lad16_3", 319, 64, 163328),
                "16 groups, four slots: tile 32": ("lad16_4", 337, 32, 86272),
                "a tile-32 tree of at most 14 groups": ("lad14_6", 325, 32, 83200)}
DH = sorted(DH_ROBOTS, key=lambda k: (DH_ROBOTS[k][0], k))
TREES = sorted(RANDOM_TREES, key=lambda k: RANDOM_TREES[k][2]) + list(LADDERS)
ALL = DH + TREES


def is_tree(name):
    return name not in DH_ROBOTS


@functools.lru_cache(maxsize=None)
def dh_robot(name):
    n, mdh, allrev = DH_ROBOTS[name]
    rb = dhc.random_robot(n, mdh, 300 + 2 * n + mdh) if allrev else oc.with_prismatic(n, bool(mdh), n // 2, 500 + 2 * n + mdh)
    sigma = [int(l.sigma) for l in rb.links]
    assert rb.n == n and int(bool(rb.mdh)) == mdh and sigma == [0 if allrev or j != n // 2 else 1 for j in range(n)], (name, sigma)
    return rb


def slots_of(parents):
    """branch slots of a group table, restated from compile_tree (csrc/tree.cpp): one per parent that some group other than the next one hangs off"""
    return len({p for j, p in enumerate(parents) if p >= 0 and p != j - 1})


def _ladder(name):
    """(ERobot, the oracle's link list): n groups numbered by hand IN group order, group j off group j - 2 for 2 <= j < k + 2 (k branch slots) and off
    group j - 1 beyond"""
    from rtbhip import ET, ETS, Link, ERobot
    n, k = LADDERS[name]
    rng = np.random.default_rng(7100 + 20 * n + k)
    kinds = ("Rz", "Ry", "Rx", "tz", "Rz", "Ry", "Rx", "Rz")
    prod, orc = [], []
    for i in range(n):
        parent = None if i == 0 else (max(0, i - 2) if i < k + 2 else i - 1)
        a, fl = kinds[i % 8], i % 8 in (2, 6)
        T = chains.elementary("Rz", rng.uniform(-1, 1)) @ chains.elementary("tx", rng.uniform(-.3, .3)) @ chains.elementary("Rx", rng.uniform(-1, 1))
        m, r = float(rng.uniform(0.5, 3)), rng.uniform(-0.3, 0.3, 3)
        prod.append(Link(ets=ETS() * ET.SE3(T) * getattr(ET, a)(flip=fl), jindex=i, m=m, r=r, parent=None if parent is None else prod[parent], name="d%d" % i))
        orc.append(dict(name="d%d" % i, parent=None if parent is None else "d%d" % parent, ets=[T, (a, None, fl)], m=m, r=r, jindex=i))
    rob = ERobot(prod, name=name)
    parents = [r["parent"] for r in rob.group_table()]
    assert rob.n == n and rob._in_group_order() and slots_of(parents) == k, (name, parents)
    p = trc._props(rob)
    assert 1 <= p["pris"] < n and p["flip"] >= 1, (name, p)
    return rob, orc


@functools.lru_cache(maxsize=None)
def tree_robot(name):
    """(ERobot, the oracle's link list)"""
    if name in LADDERS:
        return _ladder(name)
    seed, n_links, n = RANDOM_TREES[name]
    prod, orc = trc.random_tree(np.random.default_rng(seed), n_links)
    from rtbhip import ERobot
    rob = ERobot(prod, name=name)
    p = trc._props(rob)
    assert rob.n == n and rob._in_group_order(), (name, rob.n, p)
    if n >= 2:          # (one group cannot be prismatic and leave a revolute one)
        assert 1 <= p["pris"] < n and p["flip"] >= 1, (name, p)
    if n >= 3:
        assert not p["serial"], (name, p)
    return rob, trc.dfs(orc)


def robot(name):
    return tree_robot(name)[0] if is_tree(name) else dh_robot(name)


def tree_slots(name):
    return slots_of([r["parent"] for r in tree_robot(name)[0].group_table()])


def row_doubles(name):
    if is_tree(name):
        return per_row(tree_robot(name)[0].n, True, slots=tree_slots(name))
    n, _, allrev = DH_ROBOTS[name]
    return per_row(n, False, allrev)


def tail_class(n):
    """the four forms of ops_tail: the left Gram path, the LU path, the static right Gram path, the run-time-n right Gram path"""
    return "n<6" if n < 6 else "n=6" if n == 6 else "7..8" if n <= REG_MAX else "9..16"


def named():
    """{form: [names]}: ("dh", n, mdh, all-revolute) / ("tree", n) / ("class", text of TREE_CLASSES).  The robots are built to read what they are: no oracle runs"""
    out = {}
    for name in DH:
        rb = dh_robot(name)
        out.setdefault(("dh", rb.n, int(bool(rb.mdh)), all(int(l.sigma) == 0 for l in rb.links)), []).append(name)
    for name in RANDOM_TREES:          # (a ladder is filed under its launch class alone: every robot of the table is then the only one of its form)
        out.setdefault(("tree", tree_robot(name)[0].n), []).append(name)
    for text, (name, w, tile, lds) in TREE_CLASSES.items():
        if name in TREES and (row_doubles(name), tile_rows(row_doubles(name)), launch_shape(name, 1)[2]) == (w, tile, lds):
            out.setdefault(("class", text), []).append(name)
    return out


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def gravity3(name):
    """what the raw entry point is handed as grav3"""
    return np.ascontiguousarray(GRAVITY) if is_tree(name) else dh_robot(name)._gravity_c(GRAVITY)


def inertia(name, q):
    if is_tree(name):
        return oer.erobot_inertia(tree_robot(name)[1], q)
    rb = dh_robot(name)
    return oracle.inertia_dh(rb.L24(), rb.mdh, q)


def gravload(name, q):
    z = np.zeros_like(q)
    if is_tree(name):
        return oer.erobot_rne(tree_robot(name)[1], q, z, z, GRAVITY)
    rb = dh_robot(name)
    return oracle.rne_dh(rb.L24(), rb.mdh, q, z, z, gravity3(name))


@functools.lru_cache(maxsize=None)
def _chain(name):
    return chain_from_ets(dh_robot(name).ets())


def _seed(name):
    return 8100 + sum(ord(c) for c in name)


def draw_rows(tag, n, rows, seed, jac=None):
    """(q (rows, n), J (rows, 6, n), draws, replaced): q ~ U(-3, 3), J = jac(q) -- or, without one, entries ~ U(-1, 1) -- a draw replaced while
    cond(J) > COND_MAX, at most one third of them; distinct rows, read-only"""
    rng = np.random.default_rng(seed)
    cand = rng.uniform(-3.0, 3.0, (2 * rows, n))
    Jc = rng.uniform(-1.0, 1.0, (2 * rows, 6, n)) if jac is None else jac(cand)
    keep, replaced = [], 0
    for i in range(cand.shape[0]):
        if np.linalg.cond(Jc[i]) > COND_MAX:
            replaced += 1
            continue
        keep.append(i)
        if len(keep) == rows:
            break
    assert len(keep) == rows, (tag, "too few well-conditioned draws")
    draws = rows + replaced
    assert 3 * replaced <= draws, (tag, "more than one third of the draws replaced", replaced, draws)
    q, J = np.ascontiguousarray(cand[keep]), np.ascontiguousarray(Jc[keep])
    assert len({q[r].tobytes() for r in range(rows)}) == rows
    q.setflags(write=False); J.setflags(write=False)
    return q, J, draws, replaced


@functools.lru_cache(maxsize=None)
def inputs(name, rows=ROWS):
    """(q (rows, n), J (rows, 6, n), draws, replaced) of a census case: fixed seed"""
    return draw_rows(name, robot(name).n, rows, _seed(name), None if is_tree(name) else (lambda q: oracle.jacob0(_chain(name), q)))


def reference_of(q, J, M, g):
    """{"Mx": (rows, 6, 6), "Gx": (rows, 6), "all" / "trans" / "rot": (rows,), "cond": (rows,)}: opspace_cases.formula on every row, read-only"""
    rows = q.shape[0]
    out = {"Mx": np.zeros((rows, 6, 6)), "Gx": np.zeros((rows, 6)), "cond": np.array([np.linalg.cond(Ji) for Ji in J])}
    for key in AXES:
        out[key] = np.zeros(rows)
    for i in range(rows):
        for key, mask in AXES.items():
            out["Mx"][i], out["Gx"][i], out[key][i] = formula(M[i], g[i], J[i], mask)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, rows=ROWS):
    """the oracle on every row of inputs(name, rows), computed once"""
    q, J, _, _ = inputs(name, rows)
    return reference_of(q, J, inertia(name, q), gravload(name, q))


def ratios(got, ref, key):
    """[Mx, Gx, asada] as err / (eps cond^2 max|ref|), the largest over the rows"""
    Mx, Gx, asada = got
    return [ratio(Mx, ref["Mx"], ref["cond"]), ratio(Gx, ref["Gx"], ref["cond"]), ratio(asada, ref[key], ref["cond"], unit=True)]


def within(r, bounds=None):
    """[Mx, Gx, asada] ratios within the census's bound, and each within its output's own"""
    return max(r) <= K and all(x <= b for x, b in zip(r, K_OUT if bounds is None else bounds))
