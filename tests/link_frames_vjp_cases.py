"""Shared by tests/test_link_frames_vjp.py and tests/test_link_frames_vjp_emu.py (not a test module): the chains, the marks, the inputs and the
ORACLE of the all-frame adjoint (rtbhip_link_frames_vjp).

Oracle: for each mark m the PREFIX chain of the first marks[m] transforms, its pose and Jacobian from the compiled reference restated in oracle/
(oracle.fkine, oracle.jacob0), contracted as tests/test_kin_vjp.py's docstring contracts them with gJ = 0 and the base folded in:

    gq[i, col(k)] += sum (B_R^T G[i, m])[:3, :3] * ([w_k]x R)  +  (B_R^T G[i, m])[:3, 3] . v_k

with R the rotation of the prefix chain's T (no base) and (v_k ; w_k) column k of its J.  A prefix without joints contributes nothing.  It shares
nothing with the kernel: no suffix sums, no frame table, one reference call per mark.  G ~ U(-1, 1), q ~ U(-3, 3); bound: the project's kinematics
criterion, 1e-10 absolute.  Every case draws ROWS distinct rows once; the device tests repeat them cyclically to N."""
import functools

import numpy as np

from oracle import oracle, chains
from helpers import product_ets, mixed_spec, tool_base

BOUND = 1e-10
ROWS = 24
PANDA_MARKS = [0, 2, 4, 7, 10, 14, 16, 20, 22]          # models.Panda().fkine_all: the base and one frame per link of the 22-transform ETS


def random_spec(n, seed):
    """n joints of all six kinds with random flips, constants of every kind (an SE3 among them) between and after them -- helpers.mixed_spec's mix"""
    rng = np.random.default_rng(seed)
    axes = ["Rx", "Ry", "Rz", "tx", "ty", "tz"]
    spec = []
    for j in range(n):
        for _ in range(int(rng.integers(0, 3))):
            a = axes[int(rng.integers(0, 6))]
            spec.append((a, float(rng.uniform(-1.2, 1.2) if a[0] == "R" else rng.uniform(-0.4, 0.4))))
        if j % 5 == 2:
            spec.append(chains.elementary("Rz", float(rng.uniform(-1, 1))) @ chains.elementary("tx", 0.2) @ chains.elementary("Rx", float(rng.uniform(-1, 1))))
        # mostly revolute: a long run of prismatic joints only adds up translations
        a = axes[int(rng.integers(0, 3))] if rng.uniform() < 0.75 else axes[int(rng.integers(3, 6))]
        spec.append((a, None, bool(rng.integers(0, 2))))
    spec.append(("tz", 0.25))
    return spec


def _spread_marks(m, count, seed):
    """`count` nondecreasing marks in 0..m: both ends, repeats where count exceeds m + 1"""
    rng = np.random.default_rng(seed)
    inner = sorted(int(x) for x in rng.integers(0, m + 1, count - 2))
    return [0] + inner + [m]


def _all_marks(spec):
    return list(range(len(spec) + 1))


_RXRY = [("tz", 0.3), ("Rx", None), ("tx", 0.2), ("Ry", 0.4), ("Ry", None, True), ("ty", -0.1), ("Rz", 0.7), ("Rz", None), ("tx", 0.15)]
_TWO = [("tx", 0.3), ("tz", None), ("Rx", 0.5), ("Rz", None, True), ("ty", 0.2)]
_COLS = [("tz", 0.2), ("Rz", None), ("tx", 0.3), ("Ry", None, True), ("tz", 0.1)]

# name -> (spec, marks, with base?, q columns of the joints (None: 0..n-1), q width (None: n))
CASES = {
    "one": ([("tx", 0.2), ("Rz", None), ("ty", 0.3)], [0, 1, 2, 3], False, None, None),
    "two": (_TWO, _all_marks(_TWO), False, None, None),                                   # one prismatic, one flipped
    "rxry": (_RXRY, [0, 2, 3, 3, 5, 6, 7, 8, 9], False, None, None),                      # marks inside the constant run after an Rx and after an Ry joint
    "panda": (chains.PANDA_ETS, PANDA_MARKS, False, None, None),
    "panda_base": (chains.PANDA_ETS, PANDA_MARKS, True, None, None),
    "repeat": (mixed_spec(), [1, 1, 1, 5, 5, 12, 12], True, None, None),
    "zeros": (mixed_spec(), [0, 0, 0], True, None, None),                                 # every frame is the base: gq == 0
    "cols": (_COLS, _all_marks(_COLS), False, [1, 3], 5),
    "wide": (_COLS, _all_marks(_COLS), True, [1, 117], 120),                              # a q / gq tile beyond the default dynamic LDS allocation
    "n4": (random_spec(4, 41), None, True, None, None),
    "n5": (random_spec(5, 51), None, False, None, None),
    "n6": (random_spec(6, 61), None, True, None, None),
    "n8": (random_spec(8, 81), None, False, None, None),
    "n9": (random_spec(9, 91), None, True, None, None),
    "n12": (random_spec(12, 121), None, False, None, None),
    "n32": (random_spec(32, 321), None, True, None, None),
}
EMU_CASES = ["one", "two", "rxry", "panda", "panda_base", "repeat", "zeros", "n12", "n32", "cols"]


def marks_of(name):
    spec, marks = CASES[name][:2]
    return list(marks) if marks is not None else _spread_marks(len(spec), 33, 7 + len(spec))


def base_of(name):
    return tool_base()[1] if CASES[name][2] else None


@functools.lru_cache(maxsize=None)
def ets_of(name):
    """the product's ETS of a case (kept alive: its handle is reused)"""
    import rtbhip
    spec, _, _, cols, width = CASES[name]
    if cols is None:
        return product_ets(spec)
    ets, it = rtbhip.ETS(), iter(cols)
    for item in spec:
        axis, eta = item[0], item[1] if len(item) > 1 else None
        flip = bool(item[2]) if len(item) > 2 else False
        ctor = getattr(rtbhip.ET, axis)
        ets = ets * (ctor(eta) if eta is not None else ctor(flip=flip, jindex=next(it)))
    ets.q_width = width
    return ets


def spec_from_ets(ets):
    """(oracle spec, q columns of its joints) of a product ETS, from its op-table (helpers.chain_from_ets's reading of it)"""
    spec, cols = [], []
    for kind, flip, jindex, T in ets.optable():
        if kind == 6:
            spec.append(np.array(T, dtype=np.float64))
        else:
            spec.append((("Rx", "Ry", "Rz", "tx", "ty", "tz")[kind], None, bool(flip)))
            cols.append(int(jindex))
    return spec, cols


def oracle_fkine_all(er, q, G):
    """the oracle for ERobot.fkine_all (slot 0 the base, slot link.number that link): one prefix chain per link -- the path from the root to it"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, er.n)
    out = np.zeros(q.shape)
    for l in er.links:
        e = er.ets(end=l)
        if e.n == 0:
            continue
        spec, cols = spec_from_ets(e)
        out += oracle_gq(spec, [len(spec)], q, G[:, [l.number]], None, cols, er.n)
    return out


def oracle_gq(spec, marks, q, G, base=None, cols=None, width=None):
    """(N, width): the contraction of the module docstring; q (N, width), G (N, nmarks, 4, 4)"""
    n = sum(1 for it in spec if not isinstance(it, np.ndarray) and (len(it) < 2 or it[1] is None))
    cols = list(range(n)) if cols is None else list(cols)
    width = n if width is None else width
    q = np.asarray(q, dtype=np.float64).reshape(-1, width)
    out = np.zeros((q.shape[0], width))
    BR = np.eye(3) if base is None else np.asarray(base, dtype=np.float64)[:3, :3]
    for m, k in enumerate(marks):
        ch = chains.Chain(list(spec[:k]))
        if ch.n == 0:
            continue
        qm = np.ascontiguousarray(q[:, cols[:ch.n]])
        T, J = oracle.fkine(ch, qm), oracle.jacob0(ch, qm)
        Gp = np.einsum("ab,iac->ibc", BR, G[:, m, :3, :])                # B_R^T G[:3, :]
        R = T[:, :3, :3]
        for j in range(ch.n):
            v, w = J[:, :3, j], J[:, 3:, j]
            wR = np.cross(w[:, None, :], np.swapaxes(R, 1, 2)).swapaxes(1, 2)      # [w]x R, column by column
            out[:, cols[j]] += (Gp[:, :, :3] * wR).sum(axis=(1, 2)) + (Gp[:, :, 3] * v).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(ets, marks, base, q (ROWS, width), G (ROWS, nmarks, 4, 4), reference gq (ROWS, width)); the arrays are read-only"""
    spec, _, _, cols, width = CASES[name]
    marks, base = marks_of(name), base_of(name)
    ets = ets_of(name)
    w = ets.q_width
    rng = np.random.default_rng(1000 + len(spec) + 17 * len(marks))
    q = rng.uniform(-3, 3, (ROWS, w))
    G = rng.uniform(-1, 1, (ROWS, len(marks), 4, 4))
    ref = oracle_gq(spec, marks, q, G, base, cols, width)
    for a in (q, G, ref):
        a.setflags(write=False)
    return ets, marks, base, q, G, ref


def tiled(a, N):
    """the rows of a repeated cyclically to N rows"""
    return np.ascontiguousarray(a[np.arange(N) % a.shape[0]])
