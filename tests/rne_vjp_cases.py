"""Shared by tests/test_rne_vjp.py and tests/test_rne_vjp_emu.py (not a test module): the robots, the inputs and the ORACLE of the inverse-dynamics
adjoint.

Oracle: five-point Richardson central differences of the compiled reference (oracle.rne_dh / oracle.accel_dh), one input column at a time,
contracted with the incoming gradient:

    D = (4 d(h) - d(2h)) / 3,   d(h) = (f(x + h e_k) - f(x - h e_k)) / 2h,   h = 1e-3

Its own error (h against h / 2) is <= 1e-11 max(1, |g|max) for rne on the shipped DH Puma560 and DH Panda (test_rne_vjp.py checks that), a hundred
times inside the bound the adjoint is held to: rne's contract in this project, 1e-9 max(1, |ref|max) over the compared array.
Inputs: q ~ U(-3, 3), qd, qdd ~ U(-2, 2), gtau ~ U(-1, 1); for a table with Coulomb friction |qd_j| ~ U(0.1, 2) with a random sign -- no stencil
point may cross qd_j = 0, where tau jumps (at |qd| < 4e-3 the oracle itself is off by O(1))."""
import functools

import numpy as np

import rtbhip
from rtbhip.dh import DHRobot, RevoluteDH, RevoluteMDH

H = 1e-3
BOUND = 1e-9
BASE = np.array([[0.0, -1.0, 0.0, 0.1], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, -0.3], [0.0, 0.0, 0.0, 1.0]])
GRAVITY = np.array([0.4, -1.1, -9.0])
FEXT = np.array([1.5, -2.0, 0.7, 0.3, -0.4, 0.9])


def random_robot(n, mdh, seed):
    """an all-revolute table with nothing special about it: generic alpha, a, d, offset, full inertia tensors, r, Jm, B, Tc, G all non-zero"""
    rng = np.random.default_rng(seed)
    links = []
    for _ in range(n):
        A = rng.uniform(-1, 1, (3, 3))
        I = 0.05 * (A @ A.T) + 0.02 * np.eye(3)
        kw = dict(d=rng.uniform(-0.4, 0.4), a=rng.uniform(-0.4, 0.4), alpha=rng.uniform(-1.5, 1.5), offset=rng.uniform(-0.5, 0.5), m=rng.uniform(0.5, 3.0),
                  r=rng.uniform(-0.2, 0.2, 3), I=I, Jm=rng.uniform(1e-4, 5e-4), G=rng.uniform(-60, 60), B=rng.uniform(1e-4, 2e-3),
                  Tc=[rng.uniform(0.1, 0.5), -rng.uniform(0.1, 0.5)])
        links.append((RevoluteMDH if mdh else RevoluteDH)(**kw))
    return DHRobot(links, name="random%d%s" % (n, "m" if mdh else "s"))


ROBOTS = {"puma560": lambda: rtbhip.models.DH.Puma560(), "panda": lambda: rtbhip.models.DH.Panda()}
for _n in (1, 2, 3, 5, 8, 9, 12):
    for _m in (0, 1):
        ROBOTS["n%d%s" % (_n, "m" if _m else "s")] = (lambda n=_n, m=_m: random_robot(n, m, 100 + 2 * n + m))


@functools.lru_cache(maxsize=None)
def robot(name):
    return ROBOTS[name]()


def draw(rb, N, seed):
    """(q, qd, qdd, gtau), each (N, n), read-only"""
    rng = np.random.default_rng(seed)
    n = rb.n
    q, qdd, g = rng.uniform(-3, 3, (N, n)), rng.uniform(-2, 2, (N, n)), rng.uniform(-1, 1, (N, n))
    if any(np.any(np.asarray(l.Tc) != 0) for l in rb.links):
        qd = rng.uniform(0.1, 2, (N, n)) * rng.choice([-1.0, 1.0], (N, n))
    else:
        qd = rng.uniform(-2, 2, (N, n))
    for a in (q, qd, qdd, g):
        a.setflags(write=False)
    return q, qd, qdd, g


def richardson(f, xs, which, g, h=H):
    """sum_j g[:, j] d f_j / d xs[which][:, k] for every column k: (N, n)"""
    out = np.zeros_like(xs[which])
    for k in range(xs[which].shape[1]):
        def d(step):
            hi, lo = [np.array(x) for x in xs], [np.array(x) for x in xs]
            hi[which][:, k] += step
            lo[which][:, k] -= step
            return (f(*hi) - f(*lo)) / (2 * step)
        out[:, k] = (((4.0 * d(h) - d(2 * h)) / 3.0) * g).sum(axis=1)
    return out


def rne_oracle(rb, q, qd, qdd, g, gravity=None, fext=None, h=H, which=(0, 1, 2)):
    """[gq, gqd, gqdd] (None where not asked for) of the compiled reference's rne; qd / qdd None = zeros"""
    from oracle import oracle
    L, mdh, gc = rb.L24(), rb.mdh, rb._gravity_c(gravity)
    z = np.zeros_like(q)
    xs = [q, z if qd is None else qd, z if qdd is None else qdd]
    f = lambda a, b, c: oracle.rne_dh(L, mdh, a, b, c, gc, fext)
    return [richardson(f, xs, w, g, h) if w in which else None for w in range(3)]


def accel_oracle(rb, q, qd, tq, g, gravity=None, h=H):
    from oracle import oracle
    L, mdh, gc = rb.L24(), rb.mdh, rb._gravity_c(gravity)
    f = lambda a, b, c: oracle.accel_dh(L, mdh, a, b, c, gc)
    return [richardson(f, [q, qd, tq], w, g, h) for w in range(3)]


def inertia_gqdd(rb, q, g):
    """the exact identity  gqdd[i, k] = sum_j g[i, j] d tau_j / d qdd_k  from the reference's inertia rows (row k: tau for qdd = e_k)"""
    from oracle import oracle
    M = oracle.inertia_dh(rb.L24(), rb.mdh, q)
    return np.einsum("nkj,nj->nk", M, g)


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / max(1.0, np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def case(name, N, variant="plain"):
    """inputs and the oracle's answers for one (robot, N, variant): computed once, shared, never written to.
    variant: plain | noqd (qd = None) | noqdd | gravity | fext | base.  ref: [gq, gqd, gqdd], None for an absent input"""
    rb = robot(name)
    if variant == "base":
        rb = ROBOTS[name]()
        rb.base = BASE
    q, qd, qdd, g = draw(rb, N, 7000 + 13 * N + sum(map(ord, name)))
    qd = None if variant == "noqd" else qd
    qdd = None if variant == "noqdd" else qdd
    gravity = GRAVITY if variant == "gravity" else None
    fext = FEXT if variant == "fext" else None
    # (an absent input has no gradient to ask for -- and with Coulomb friction the differences in qd around qd = 0 would straddle the jump)
    ref = rne_oracle(rb, q, qd, qdd, g, gravity, fext, which=tuple(w for w, x in enumerate((q, qd, qdd)) if x is not None))
    for a in ref:
        if a is not None:
            a.setflags(write=False)
    return rb, q, qd, qdd, g, gravity, fext, ref
