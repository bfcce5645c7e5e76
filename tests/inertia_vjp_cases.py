"""Shared by tests/test_inertia_vjp.py and tests/test_inertia_vjp_emu.py (not a test module): the robots, the inputs and the ORACLE of the adjoint of
the joint-space inertia matrix (rtbhip_inertia_vjp, rtbhip_tree_inertia_vjp).

Oracle: the five-point Richardson central differences of tests/rne_vjp_cases.py on the reference's inertia matrix (oracle.inertia_dh for DH robots,
oracle.erobot.erobot_inertia on the link list tests/tree_rne_vjp_cases.py restates for link trees), one q column at a time, the (N, n, n) difference
contracted with the incoming gradient gM:

    D = (4 d(h) - d(2h)) / 3,   d(h) = (M(q + h e_k) - M(q - h e_k)) / 2h,   h = 1e-3

Its own error, measured on the CPU at 24 rows (DH) / 8 rows (trees) as the largest difference between the stencil at h and at h / 2 over
max(1, |ref|max): Puma560 7.1e-13, Panda 8.1e-13, UR5 6.2e-13 at h = 1e-3 -- inside 1e-11 max(1, |ref|max), a hundredth of the bound, so h = 1e-3
stays (test_inertia_vjp.py::test_the_oracle_is_a_hundred_times_finer_than_the_bound holds it there).
Bound: the project's contract, 1e-9 max(1, |ref|max) over the compared array.
Inputs: q ~ U(-3, 3), gM ~ U(-1, 1), NOT symmetric: every entry of M is an output in its own right.  The tree oracle is a per-sample Python loop,
so a tree case draws ROWS distinct rows and repeats them cyclically to N (tree_rne_vjp_cases.tiled); the oracle runs once on the ROWS rows.

What period-8 inputs CANNOT see: row r and row r + 8 carry the same inputs and the same expected outputs, so a staging or flush error that moves a
row by a multiple of 8 (the tile's f / n, f % n index arithmetic, the per-pass restaging of the run-time-n forms) returns exactly the expected
bits.  The cyclic tree cases serve test_gradient_equals_the_oracle and the guard-row test, where the oracle is needed on every row; rows that are
all distinct are covered by tests/test_flush_guard_all_gpu.py (129 distinct rows per robot at every size of its table) and, in
tests/test_inertia_vjp.py, by test_rows_are_independent, test_fused_call_equals_the_composition and
test_nonfinite_and_huge_joint_values_stay_in_their_row (draw() with no oracle: bit comparisons and the composition)."""
import functools

import numpy as np

import rne_vjp_cases as dh_cases
import tree_rne_vjp_cases as tree_cases
from rne_vjp_cases import richardson, rel_err, H, BOUND        # the same stencil, the same bound
from tree_rne_vjp_cases import tiled

ROWS = 8

DH_ROBOTS = dict(dh_cases.ROBOTS)
for _m in (0, 1):
    DH_ROBOTS["n16%s" % ("m" if _m else "s")] = (lambda m=_m: dh_cases.random_robot(16, m, 100 + 2 * 16 + m))
DH_SMALL = sorted(k for k in DH_ROBOTS if k in ("puma560", "panda") or int(k[1:-1]) <= 8)      # the register forms
DH_BIG = sorted(k for k in DH_ROBOTS if k not in DH_SMALL)                                       # the run-time-n form
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
    """(q (rows, n), gM (rows, n, n)), read-only"""
    rng = np.random.default_rng(seed)
    q, g = rng.uniform(-3, 3, (rows, n)), rng.uniform(-1, 1, (rows, n, n))
    q.setflags(write=False)
    g.setflags(write=False)
    return q, g


def dh_oracle(rb, q, gM, h=H):
    from oracle import oracle
    L, mdh, n = rb.L24(), rb.mdh, rb.n
    f = lambda a: oracle.inertia_dh(L, mdh, a).reshape(-1, n * n)
    return richardson(f, [q], 0, gM.reshape(-1, n * n), h)


def tree_oracle(orc, q, gM, h=H):
    from oracle import erobot as oer
    n = q.shape[1]
    f = lambda a: oer.erobot_inertia(orc, a).reshape(-1, n * n)
    return richardson(f, [q], 0, gM.reshape(-1, n * n), h)


def _seed(name, N):
    return 11000 + 13 * N + sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def dh_case(name, N):
    """(robot, q, gM, ref) for one (DH robot, N): computed once, shared, never written to"""
    rb = dh_robot(name)
    q, g = draw(rb.n, N, _seed(name, N))
    ref = dh_oracle(rb, q, g)
    ref.setflags(write=False)
    return rb, q, g, ref


@functools.lru_cache(maxsize=None)
def tree_case(name):
    """(robot, the oracle's link list, q, gM, ref) of ROWS rows for one link tree: computed once, shared, never written to"""
    rob, orc = tree_robot(name)
    q, g = draw(rob.n, ROWS, _seed(name, ROWS))
    ref = tree_oracle(orc, q, g)
    ref.setflags(write=False)
    return rob, orc, q, g, ref
