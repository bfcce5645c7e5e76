"""Shared by tests/test_coriolis_vjp.py and tests/test_coriolis_vjp_emu.py (not a test module): the robots, the inputs and the ORACLE of the adjoint of
the Coriolis / centripetal matrix (rtbhip_coriolis_vjp, rtbhip_tree_coriolis_vjp).

Oracle for gq: the five-point Richardson central differences of tests/rne_vjp_cases.py on the reference's Coriolis matrix (oracle.coriolis_dh for DH
robots, oracle.erobot.erobot_coriolis on the link list tests/tree_rne_vjp_cases.py restates for link trees), one q column at a time, the (N, n, n)
difference contracted with the incoming gradient gC:

    D = (4 d(h) - d(2h)) / 3,   d(h) = (C(q + h e_k, qd) - C(q - h e_k, qd)) / 2h,   h = 1e-3

Oracle for gqd: no stencil.  C is linear in qd, so  gqd[:, m] = sum_jk gC[:, j, k] C(q, e_m)[:, j, k]  exactly.

The stencil's own error, measured on the CPU with these inputs (8 rows DH, 2 rows trees) as the largest difference between the stencil at h and at
h / 2 over max(1, |ref|max): Puma560 6.2e-13, Panda 9.6e-13, UR5 8.8e-13 -- inside 1e-11, a hundredth of the bound, so h = 1e-3 stays; the exact gqd
against its own stencil <= 2.0e-13 (test_coriolis_vjp.py::test_the_oracle_is_a_hundred_times_finer_than_the_bound).
Bound: the project's contract, 1e-9 max(1, |ref|max) over the compared array.
Inputs: q ~ U(-3, 3), qd ~ U(-2, 2), gC ~ U(-1, 1).  The reference's Coriolis matrix costs n + n (n - 1) / 2 inverse-dynamics calls per row and the
stencil 4 n of those, and the tree oracle is a Python loop (one erobot_coriolis row of YuMi: 0.12 s): a case draws a few distinct rows -- 8, or 2
for the big trees -- and repeats them cyclically to N (tree_rne_vjp_cases.tiled); the oracle runs once on the distinct rows.

What period-8 / period-2 inputs CANNOT see: row r and row r + 8 (r + 2) carry the same inputs and the same expected outputs, so a staging or flush
error that moves a row by a multiple of the period (the tile's f / n, f % n index arithmetic, the per-pass restaging of the run-time-n forms)
returns exactly the expected bits.  The cyclic cases serve test_gradients_equal_the_oracle and the guard-row test, where the oracle is needed on
every row; rows that are all distinct are covered by tests/test_flush_guard_all_gpu.py (129 distinct rows per robot at every size of its table)
and, in tests/test_coriolis_vjp.py, by test_rows_are_independent, test_fused_call_equals_the_composition and
test_nonfinite_and_huge_joint_values_stay_in_their_row (draw() with no oracle: bit comparisons and the composition)."""
import functools

import numpy as np

import rne_vjp_cases as dh_cases
import tree_rne_vjp_cases as tree_cases
from rne_vjp_cases import richardson, rel_err, H, BOUND        # the same stencil, the same bound
from tree_rne_vjp_cases import tiled

ROWS = 8
BIG_ROWS = 2

DH_ROBOTS = dict(dh_cases.ROBOTS)
for _m in (0, 1):
    DH_ROBOTS["n16%s" % ("m" if _m else "s")] = (lambda m=_m: dh_cases.random_robot(16, m, 100 + 2 * 16 + m))
DH_SMALL = sorted(k for k in DH_ROBOTS if k in ("puma560", "panda") or int(k[1:-1]) <= 8)      # up to 8 joints (1..7: the register forms; 8: run-time-n)
DH_BIG = sorted(k for k in DH_ROBOTS if k not in DH_SMALL)                                       # 9 joints and more: the run-time-n form
TREES = list(tree_cases.AUTO)                   # numbered in group order
TREE_BIG = ("tree9", "KinovaGen3", "YuMi")      # 9, 13 and 14 joints: the run-time-n form
HAND = "hand4"                                  # numbered by hand: refused by the raw call, the ordinary path in the front end


@functools.lru_cache(maxsize=None)
def dh_robot(name):
    return DH_ROBOTS[name]()


def tree_robot(name):
    """(ERobot, the oracle's link list)"""
    return tree_cases.robot(name)


def draw(n, rows, seed):
    """(q (rows, n), qd (rows, n), gC (rows, n, n)), read-only"""
    rng = np.random.default_rng(seed)
    q, qd, g = rng.uniform(-3, 3, (rows, n)), rng.uniform(-2, 2, (rows, n)), rng.uniform(-1, 1, (rows, n, n))
    for a in (q, qd, g):
        a.setflags(write=False)
    return q, qd, g


def _gq(C, q, qd, gC, h):
    n = q.shape[1]
    return richardson(lambda a: C(a, qd).reshape(-1, n * n), [q], 0, gC.reshape(-1, n * n), h)


def _gqd(C, q, gC):
    n = q.shape[1]
    out = np.zeros_like(q)
    for m in range(n):
        e = np.zeros_like(q)
        e[:, m] = 1.0
        out[:, m] = (C(q, e) * gC).sum(axis=(1, 2))
    return out


def dh_coriolis(rb):
    from oracle import oracle
    L, mdh = rb.L24(), rb.mdh
    return lambda q, qd: oracle.coriolis_dh(L, mdh, q, qd)


def tree_coriolis(orc):
    from oracle import erobot as oer
    return lambda q, qd: oer.erobot_coriolis(orc, q, qd)


def dh_oracle(rb, q, qd, gC, h=H):
    """(gq, gqd)"""
    C = dh_coriolis(rb)
    return _gq(C, q, qd, gC, h), _gqd(C, q, gC)


def tree_oracle(orc, q, qd, gC, h=H):
    """(gq, gqd)"""
    C = tree_coriolis(orc)
    return _gq(C, q, qd, gC, h), _gqd(C, q, gC)


def gqd_stencil(C, q, qd, gC, h=H):
    """gqd from the same stencil on qd: what the exact form is checked against"""
    n = q.shape[1]
    return richardson(lambda a, b: C(a, b).reshape(-1, n * n), [q, qd], 1, gC.reshape(-1, n * n), h)


def _seed(name):
    return 17000 + sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def dh_case(name):
    """(robot, q, qd, gC, ref_gq, ref_gqd) of ROWS rows for one DH robot: computed once, shared, never written to"""
    rb = dh_robot(name)
    q, qd, g = draw(rb.n, ROWS, _seed(name))
    rq, rd = dh_oracle(rb, q, qd, g)
    rq.setflags(write=False)
    rd.setflags(write=False)
    return rb, q, qd, g, rq, rd


@functools.lru_cache(maxsize=None)
def tree_case(name):
    """(robot, the oracle's link list, q, qd, gC, ref_gq, ref_gqd) of ROWS (BIG_ROWS for the big trees) rows for one link tree"""
    rob, orc = tree_robot(name)
    q, qd, g = draw(rob.n, BIG_ROWS if name in TREE_BIG else ROWS, _seed(name))
    rq, rd = tree_oracle(orc, q, qd, g)
    rq.setflags(write=False)
    rd.setflags(write=False)
    return rob, orc, q, qd, g, rq, rd


def case(name, N):
    """(robot, q (N, n), qd (N, n), gC (N, n, n), ref_gq (N, n), ref_gqd (N, n)) of a DH robot or a link tree, its distinct rows repeated to N"""
    if name in DH_ROBOTS:
        rb, q, qd, g, rq, rd = dh_case(name)
    else:
        rb, _, q, qd, g, rq, rd = tree_case(name)
    return (rb,) + tuple(tiled(x, N) for x in (q, qd, g, rq, rd))
