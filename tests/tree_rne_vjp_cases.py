"""Shared by tests/test_tree_rne_vjp.py and tests/test_tree_rne_vjp_emu.py (not a test module): the robots, the inputs and the ORACLE of the
adjoint of the link-tree inverse dynamics (rtbhip_tree_rne_vjp).

Oracle: five-point Richardson central differences of the restated reference (oracle.erobot.erobot_rne / erobot_accel), one input column at a
time, contracted with the incoming gradient -- the scheme of tests/rne_vjp_cases.py:

    D = (4 d(h) - d(2h)) / 3,   d(h) = (f(x + h e_k) - f(x - h e_k)) / 2h,   h = 1e-3

Its own error (h against h / 2) is <= 1e-11 max(1, |g|max) on these robots (test_tree_rne_vjp.py checks that), a hundred times inside the bound
the adjoint is held to: 1e-9 max(1, |ref|max) over the compared array, the DH adjoint's bound.
Inputs: q ~ U(-3, 3), qd, qdd ~ U(-2, 2), gtau ~ U(-1, 1).  The oracle is a per-sample Python loop, so a case draws ROWS = 16 distinct rows and
repeats them cyclically to N; the oracle runs once on the 16 and is tiled -- every lane and tile position is compared."""
import functools

import numpy as np

import rtbhip
from rtbhip import ET, ETS, Link, ERobot, urdf
from oracle import erobot as oer, chains
from rne_vjp_cases import richardson, rel_err, H, BOUND        # the same stencil, the same bound

ROWS = 16
GRAVITY = np.array([0.4, -1.1, -9.0])


def random_tree(rng, n_links=9):
    """tests/test_erobot_rne.py's recipe: a branched robot exercising every joint kind, flips, static links (with mass) and SE3 constants"""
    axes = ["Rx", "Ry", "Rz", "tx", "ty", "tz"]
    prod, orc = [], []
    for i in range(n_links):
        parent = None if i == 0 else int(rng.integers(max(0, i - 3), i))
        items, ets = [], ETS()
        T = chains.elementary("Rz", rng.uniform(-1, 1)) @ chains.elementary("tx", rng.uniform(-.3, .3)) @ chains.elementary("Rx", rng.uniform(-1, 1))
        items.append(T); ets = ets * ET.SE3(T)
        if rng.uniform() < 0.5:
            a, v = axes[int(rng.integers(0, 6))], float(rng.uniform(-0.5, 0.5))
            items.append((a, v)); ets = ets * getattr(ET, a)(v)
        if rng.uniform() < 0.75 or i == n_links - 1:
            a, fl = axes[int(rng.integers(0, 6))], bool(rng.uniform() < 0.3)
            items.append((a, None, fl)); ets = ets * getattr(ET, a)(flip=fl)
        m, r = float(rng.uniform(0, 3)), rng.uniform(-0.3, 0.3, 3)
        name = "k%d" % i
        prod.append(Link(ets=ets, m=m, r=r, parent=(prod[parent] if parent is not None else None), name=name))
        orc.append(dict(name=name, parent=(None if parent is None else "k%d" % parent), ets=items, m=m, r=r))
    return prod, orc


def dfs(orc):
    """links in the depth-first order the reference's _sort_links produces"""
    kids = {l["name"]: [] for l in orc}
    for l in orc:
        if l["parent"] is not None:
            kids[l["parent"]].append(l)
    out, stack = [], [orc[0]]
    while stack:
        l = stack.pop()
        out.append(l)
        stack.extend(reversed(kids[l["name"]]))
    return out


# name -> (seed, links drawn, joints, serial chain?): what the seed gives is asserted in _tree()
TREES = {"one_p": (0, 1, 1, True), "one_r": (5, 1, 1, True), "chain3": (7, 4, 3, True), "chain8": (216, 9, 8, True), "tree3": (1, 3, 3, False),
         "tree5": (1, 6, 5, False), "tree6": (3, 9, 6, False), "tree7": (2, 8, 7, False), "tree8": (2, 9, 8, False), "tree9": (1, 10, 9, False)}
BRANCHED = ("tree5", "tree6", "tree7", "tree8")          # each: a prismatic group, a flipped joint, a static link with mass
URDFS = {"UR5": (), "KinovaGen3": (), "YuMi": ("gripper_r_base", "gripper_l_base")}
ROBOTS = sorted(TREES) + sorted(URDFS) + ["hand4"]
AUTO = [n for n in ROBOTS if n != "hand4"]               # numbered in group order: M symmetric, the gqdd identity and accel apply


def _props(rob):
    recs = rob.group_table()
    par = [r["parent"] for r in recs]
    last = max(i for g in rob.link_groups() for i in g)
    return dict(serial=all(p == j - 1 for j, p in enumerate(par)), pris=sum(r["kind"] >= 3 for r in recs), flip=sum(r["flip"] for r in recs),
                static=sum((not l.isjoint) and l.m > 0 for l in rob.links[:last + 1]))


def _tree(name):
    seed, n_links, n, serial = TREES[name]
    prod, orc = random_tree(np.random.default_rng(seed), n_links)
    rob = ERobot(prod, name=name)
    p = _props(rob)
    assert rob.n == n and p["serial"] == serial, (name, rob.n, p)
    if name in BRANCHED:
        assert 5 <= rob.n <= 8 and p["pris"] >= 1 and p["flip"] >= 1 and p["static"] >= 1 and p["pris"] < rob.n, (name, p)
    if name == "tree9":
        assert 9 <= rob.n <= 12 and not p["serial"]
    return rob, dfs(orc)


def _urdf(name):
    r = urdf.load(name)
    exclude = tuple(e for e in URDFS[name] if e in r.linkdict)
    er = r.erobot(exclude)
    orc = []
    for l in er.links:                                        # er.links is already in depth-first order (tests/test_erobot_rne.py: _urdf_case)
        items = [(e.axis, None, e.isflip) if e.isjoint else np.array(e.T) for e in l.ets]
        orc.append(dict(name=l.name, parent=None if l.parent is None else l.parent.name, ets=items, m=l.m, r=l.r))
    return er, orc


def _hand4():
    """a branched 4-joint tree whose joints are numbered by hand, out of group order: q / qd / qdd and the gradients go by jindex, gtau by group"""
    prod, orc = random_tree(np.random.default_rng(4), 6)      # (hand-numbered links keep the order they were given in: no depth-first sort)
    order = [2, 0, 3, 1]
    by_name, k = {}, 0
    for l in orc:
        if len(l["ets"][-1]) == 3 and not isinstance(l["ets"][-1], np.ndarray):
            by_name[l["name"]] = order[k]
            l["jindex"] = order[k]
            k += 1
    assert k == 4
    made = {}
    for l in prod:
        made[l.name] = Link(l.ets, jindex=by_name.get(l.name), m=l.m, r=l.r, parent=None if l.parent is None else made[l.parent.name], name=l.name)
    rob = ERobot(list(made.values()), name="hand4")
    assert rob.n == 4 and [r["jindex"] for r in rob.group_table()] == order and not _props(rob)["serial"]
    return rob, orc


@functools.lru_cache(maxsize=None)
def robot(name):
    """(ERobot, the oracle's link list)"""
    if name in TREES:
        return _tree(name)
    if name in URDFS:
        return _urdf(name)
    assert name == "hand4"
    return _hand4()


def draw(n, seed, rows=ROWS):
    rng = np.random.default_rng(seed)
    q, qd, qdd, g = rng.uniform(-3, 3, (rows, n)), rng.uniform(-2, 2, (rows, n)), rng.uniform(-2, 2, (rows, n)), rng.uniform(-1, 1, (rows, n))
    for a in (q, qd, qdd, g):
        a.setflags(write=False)
    return q, qd, qdd, g


def rne_oracle(orc, q, qd, qdd, g, gravity, h=H, which=(0, 1, 2)):
    """[gq, gqd, gqdd] (None where not asked for) of the restated reference's rne; qd / qdd None = zeros"""
    z = np.zeros_like(q)
    xs = [q, z if qd is None else qd, z if qdd is None else qdd]
    f = lambda a, b, c: oer.erobot_rne(orc, a, b, c, gravity)
    return [richardson(f, xs, w, g, h) if w in which else None for w in range(3)]


def accel_oracle(orc, q, qd, tq, g, gravity, h=H):
    f = lambda a, b, c: oer.erobot_accel(orc, a, b, c, gravity)
    return [richardson(f, [q, qd, tq], w, g, h) for w in range(3)]


def inertia_gqdd(orc, q, g):
    """the exact identity  gqdd[i, k] = sum_j g[i, j] d tau_j / d qdd_k  from the reference's inertia rows (row k: tau for qdd = e_k)"""
    return np.einsum("nkj,nj->nk", oer.erobot_inertia(orc, q), g)


def gravity_of(rob, variant):
    return GRAVITY if variant == "gravity" else np.asarray(rob.gravity, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(name, variant="plain"):
    """inputs (ROWS rows) and the oracle's answers for one (robot, variant): computed once, shared, never written to.
    variant: plain | noqd (qd = None) | noqdd | gravity.  ref: [gq, gqd, gqdd], None for an absent input"""
    rob, orc = robot(name)
    q, qd, qdd, g = draw(rob.n, 9000 + sum(map(ord, name)))
    qd = None if variant == "noqd" else qd
    qdd = None if variant == "noqdd" else qdd
    gravity = gravity_of(rob, variant)
    ref = rne_oracle(orc, q, qd, qdd, g, gravity, which=tuple(w for w, x in enumerate((q, qd, qdd)) if x is not None))
    for a in ref:
        if a is not None:
            a.setflags(write=False)
    return rob, orc, q, qd, qdd, g, gravity, ref


def tiled(x, N):
    """the ROWS rows repeated cyclically to N rows (None stays None)"""
    return None if x is None else np.ascontiguousarray(x[np.arange(N) % x.shape[0]])
