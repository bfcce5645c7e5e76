"""Every output flush outside the fkine / Jacobian tile writes its rows and nothing else: guard rows, every live row against the oracle, row
independence bit for bit, and the launch shape -- one table row per (compute entry point of include/rtbhip.h, form), through the raw C ABI.

What a row does, at every N in SIZES (one lane; the 8-configuration line groups of k_frames; the 16-row rounds of the Hessian tile; the 32- and
64-row seams, one row either side of each; two tiles ending full, ragged by one or empty), on the first N rows of inputs drawn ONCE at N = 129
(q ~ U(-pi, pi)):

1. guard rows.  Every input and every output is a flush_guard.Guarded buffer: 64 rows of a fixed NaN bit pattern in front and behind, one
   allocation.  After the call the guard rows of every output hold the pattern, every input buffer is unchanged bit for bit (guards included), and an
   output that was not asked for (a NULL gradient) holds the pattern everywhere.
2. every live row against the oracle, with the oracle and the bound of the family's own device test (restated next to each builder with a
   file:line pointer): all N rows at every N, for the compiled oracles and for the Python-loop ones alike (oracle/erobot.py, the Richardson
   stencils over it, the momentum balance, the Python IK solvers), each computed once on the 129 rows.  The only rows left out are those the
   family's own test leaves out: a singular J J^T for jacobm_from_jacobian, a sum on the p_servo threshold, an IK target the oracle does not solve.
   The fused adjoints of the Coriolis matrix of a link tree (and of the inertia matrix of the 9-joint tree) are the exception in cost: their oracle
   is a Python loop of n + n (n - 1) / 2 inverse-dynamics evaluations per matrix and 5 n matrices per row.  It runs on ORACLE_ROWS_24 / _14 (the
   seams, every residue mod 8, three classes twice in one tile), and EVERY row is held at 2e-9 max(1, |ref|max) to the composition the fused call
   replaces -- launches of rtbhip_tree_rne_vjp, another kernel, itself held to its oracle on all 129 rows here -- at N = 129; every smaller N must
   return the bits of the leading rows of that result (Case.second).  No row of any table row is left out of both.
   Outputs are finite everywhere (a read past the last input row would bring in a NaN of the input guards); IK: wherever it reports success.
3. row independence.  Every row of SEAM_ROWS below N -- the first row, the last row of every size and the rows either side of every multiple of
   8 -- has the bits of the same row computed alone (N = 1).
4. launch shape.  rtbhip.last_launch() shows ceil(N / 64) workgroups and, where the table row names one, the LDS request of the path the row is
   filed under, restated from the launch code: hess_mode 0 / 2 -> k_kin_hess_tile<NJ, 4 / 8>, 1 -> k_kin_hess<NJ>, the run-time-n tile k_kin;
   hessian_from_jacobian, the from-Jacobian consumers, the pose errors, the differential-kinematics kernel, link_frames and its adjoint, rne and
   its adjoint, the kinematics adjoints (register tile and k_vjp_from_jac_any).  The requests of inertia / coriolis / accel, of the tree kernels
   and of rne_base_wrench depend on per-robot tables (slots, aliasing and strides chosen by structure): there the grid alone is asserted.
   IK is left out: its grid is the scheduler's (waves per CU), not the batch's.

The Hessian family in depth: frames 0 and 1, with and without a tool, n in {1, 2, 3, 6, 7, 9, 10} on the register tile (hess_mode 0, 1, 2; the
requests above 48 KB at n = 9, 10 go through hipFuncSetAttribute), n in {11, 12} and reg = 0 on the run-time-n tile with coalesced 1 and 0,
tiles_per_wave = 2 (grid-stride k_kin: at N = 129 three tiles on two waves, one ends on a lone tile), hessian_from_jacobian at the same n and
n = 14 (k_hess_from_jac_any).  Bit-equal by construction and asserted: tiles_per_wave 2 against 1 (the same kernel on another grid).  NOT asserted:
hess_mode 0 / 1 / 2, reg 0 / 1, coalesced 0 / 1 against each other -- different instantiations whose contraction into fused multiply-adds the
compiler chooses per kernel; each is held to the oracle bound on its own.

Ad-hoc chains are created and run under rtbhip.tune("jit", 0): no case waits for, or leaves behind, a run-time compile.  A fixture restores every
knob.

The fused adjoints of the inertia and Coriolis matrices (rtbhip_inertia_vjp, rtbhip_coriolis_vjp and their tree forms): the register forms, the
last register size, the first run-time-n size and a long one of each; for the Coriolis pair gq alone and gqd alone return the bits of the call that
asks for both and leave the other buffer untouched (Case.same_as).  A tree of at most 8 groups that launch_tree_coriolis_vjp cannot serve with
the register form exists only with hand numbering: the register form's request 64 * 8 * (((2 n + n^2) | 1) + 24 nslots + 18 nkept) exceeds
160 KB = 320 doubles per lane only at n = 8 (row 81) with 24 nslots + 18 nkept > 239; nslots <= n - 2 = 6 (a slot needs a parent with a child
two or more groups on), nkept <= n - 1 = 7.  A depth-first numbering keeps only leaves and has a slot per branching group, at most 162.  _ladder8
(group j off group j - 2: 6 slots, 7 kept, 179712 bytes) is such a table; its row asserts the run-time-n request, 86528 bytes.

The set of entry points is read from include/rtbhip.h (header_census): every `int rtbhip_*(..., int32_t mem, void *stream)`, and every
`int rtbhip_*(... int64_t N ..., void *stream)` without a mem -- rtbhip_ik_vjp, rtbhip_opspace and rtbhip_tree_opspace, exactly.  The ctypes table's
stream types (_sp, _si, _sc, ...) serve the families' refusal censuses and decide nothing here.

Row-independence exceptions: none.  Every entry point of the table, IK included (q0 supplied, one search), returns for a row of a batch the bits
of that row computed alone.

The Panda URDF carries no masses (every torque of its link tree is zero), so the tree rows take UR5, KinovaGen3 and the random trees of
tests/tree_rne_vjp_cases.py; a row whose oracle is zero everywhere fails as vacuous unless it says why (the one-joint Hessian without a tool).
tests/test_flush_guard_engine.py shows without a GPU that each kind of wrong flush fails the check named for it.

RESULTS of the device run with every row compared (MI355X; every row prints "flush_guard_all <id>: <entry point> <output> max deviation ... (... of its bound)"):
all rows green, no guard row written, no row depending on its tile mates.  Worst deviation from the oracle per entry point, absolute, and as a
fraction of the bound it is held to:

    hessian                        1.8e-15  (1.8e-05)     rne                      4.3e-13  (1.9e-06)     ik_lm                    6.0e-12  (6.0e-06)
    hessian_from_jacobian          2.2e-16  (2.2e-06)     rne_f32                  7.2e-06  (0.96)        ik_lm_nullspace          2.2e-10  (2.2e-04)
    manipulability_from_jacobian   1.7e-14  (1.6e-04)     rne_base_wrench          2.6e-06  (7.7e-04)     ik_qp                    2.5e-13  (2.5e-06)
    jacobm_from_jacobian           3.4e-14  (2.9e-05)     inertia                  1.8e-15  (3.0e-04)     fkine_jacob_vjp          4.2e-15  (4.2e-05)
    angle_axis                     8.4e-15  (0.20)        coriolis                 2.2e-15  (7.6e-05)     kin_vjp_from_jacobian    1.8e-15  (1.8e-05)
    p_servo_error                  8.4e-15  (0.20)        accel                    5.7e-13  (8.5e-07)     fkine_jacob_vjp_f32      2.3e-07  (0.99)
    p_servo                        2.8e-14  (0.20)        tree_rne                 3.6e-14  (7.7e-06)     rne_vjp                  1.8e-10  (7.6e-03)
    jacob_dot                      1.6e-15  (1.6e-05)     tree_inertia             3.6e-15  (6.4e-04)     rne_vjp_f32              6.5e-06  (0.93)
    jacob0_analytical              9.6e-15  (9.6e-06)     tree_coriolis            1.8e-15  (7.1e-04)     tree_rne_vjp             4.5e-11  (4.9e-03)
    jacob0_dot_analytical          5.4e-06  (0.12)        tree_accel               4.8e-12  (5.8e-06)     link_frames_vjp          1.1e-14  (1.1e-04)
    manipulability                 1.2e-14  (4.8e-04)     link_frames              5.6e-16  (5.6e-06)
    jacobm                         2.4e-14  (1.8e-05)

    inertia_vjp            gq      3.4e-11  (8.1e-04)     tree_inertia_vjp    gq   7.0e-12  (1.9e-03)   against the composition  5.3e-15  (1.2e-07)
    coriolis_vjp           gq      9.3e-11  (1.4e-03)     tree_coriolis_vjp   gq   1.2e-11  (9.3e-04)   against the composition  3.6e-14  (1.1e-06)
                           gqd     3.2e-14  (1.6e-06)                         gqd  4.9e-15  (1.6e-06)   against the composition  1.4e-14  (8.5e-07)

    opspace                Mx      3.0e-06  (0.43)        tree_opspace        Mx   5.8e-11  (0.035)       ik_vjp    gTep     7.2e-12  (2.7e-04)
                           Gx      1.1e-08  (0.020)                           Gx   3.0e-12  (6.7e-03)                 gtwist   7.2e-12  (2.7e-04)
                           asada   1.7e-14  (0.014)                           asada 5.8e-16 (4.6e-03)

(the three entry points without a mem argument: puma560, panda, n9s, the general 16-joint chain p16s in tiles of 32 rows, UR5 and the ladder tree
lad16_4 in tiles of 32 rows; the bound is K eps cond(J)^2 max|ref| per row, so the absolute figures are those of rows with cond(J) near 1e3;
rows whose `success` is 0 return exact zeros.)

(gq is held to a finite-difference stencil whose own error is some 1e-12 of the scale; gqd of the Coriolis pair to the exact linearity in qd, and
the fused call agrees with the composition it replaces to a few ulp.)

(The float32 rows sit at their bound by construction: it is 1e-9 of the scale plus half a float32 ulp of the value, and the rounding error of a
float32 result reaches half an ulp.)  The whole module takes 85 s on the device, 21 s of it the rows that were here before the inertia / Coriolis adjoints joined (slowest of those
3.7 s, the Richardson stencil of a 9-joint tree on all 129 rows).  The 26 adjoint rows cost 64 s, nearly all of it their CPU oracles, each computed
once per robot: tree_coriolis_vjp tree8 11.3 s and tree9 10.5 s (the Python Coriolis stencil on 24 / 14 oracle rows, the fewest the row
conditions allow), coriolis_vjp n12m 8.5 s (600 000 calls of the compiled inverse dynamics), tree_inertia_vjp tree8 7.9 s (all 129 rows)."""
import functools
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib, urdf
from helpers import replaying, chain_from_ets, tool_base, angle_axis_tolerance, DEV
from flush_guard import Guarded
from oracle import oracle, chains, erobot as oer, poe

# raw device pointers into guarded buffers: not served by the CPU replay of the GPU suite
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(replaying(), reason="raw device pointers into guarded buffers: not served by the CPU replay")]

SIZES = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129)
NMAX = max(SIZES)
SEAM_ROWS = np.array(sorted({0} | {N - 1 for N in SIZES} | {k + d for k in range(8, NMAX, 8) for d in (-1, 0)}))
ALL_ROWS = np.arange(NMAX)
KNOBS = {"jit": 1, "hess_mode": 0, "reg": 1, "coalesced": 1, "tiles_per_wave": 1}          # the defaults (csrc/kin_kernels.hip:537-540, csrc/jit.cpp:203)
JIT0 = {"jit": 0}
MEM = _lib.MEM_DEVICE
TOOL, BASE = tool_base()
WORST = {}


@pytest.fixture(autouse=True)
def _knobs():
    yield
    for k, v in KNOBS.items():
        rtbhip.tune(k, v)


# ------------------------------------------------------------------------------------------------ the engine
class In:
    """an input array: (NMAX, ...) rows of which a batch takes the first N -- or, fixed=True, an operand passed whole at every N (a broadcast pose)"""

    def __init__(self, a, dtype="float64", fixed=False):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.a, self.dtype, self.fixed = a.reshape(a.shape[0], -1), dtype, fixed
        assert fixed or a.shape[0] == NMAX


class O:
    """an output array: name, values per row, dtype"""

    def __init__(self, name, width, dtype="float64"):
        self.name, self.width, self.dtype = name, int(width), dtype


class Case:
    """fn: entry point; ins: name -> In; outs: [O]; args(N, p, stream) -> the argument tuple, p(name) the device address of that buffer's first live
    row (an output whose p() is never asked for must stay untouched); ref: output name -> (NMAX, width) oracle rows; rows: None (all rows carry an
    oracle value) | index array | name -> either; tol(name, ref rows, their indices) -> absolute bound per entry; err(name, got, ref) -> deviation per entry
    (default |got - ref|); launch(N) -> (grid, LDS bytes | None); check(res, N): a comparison of its own instead (IK); twin: knobs under which the
    N = NMAX call must return the same bits; zero_ok: the oracle may be zero everywhere (else that is a vacuous row and fails);
    second() -> output name -> (NMAX, width): a second reference that has a value on EVERY row (where the oracle is affordable on a few rows only),
    evaluated once after the N = NMAX call and compared with it on all rows at tol2(name, second rows) -- and then every smaller N must have
    returned the bits of the leading rows of the N = NMAX result, which ties their rows to that comparison; same_as() -> another Case on the same
    inputs (the call with every output asked for) whose N = NMAX call must return the same bits for the outputs this one asks for"""

    def __init__(self, fn, ins, outs, args, ref=None, tol=None, rows=None, err=None, launch=None, check=None, twin=None, keep=None, zero_ok=False,
                 second=None, tol2=None, same_as=None):
        self.fn, self.ins, self.outs, self.args, self.ref, self.tol, self.rows = fn, ins, outs, args, ref or {}, tol, rows
        self.err, self.launch, self.check, self.twin, self.keep, self.zero_ok = err, launch, check, twin, keep, zero_ok
        self.second, self.tol2, self.same_as = second, tol2, same_as
        assert (second is None) == (tol2 is None)

    def rows_of(self, name, N):
        r = self.rows.get(name) if isinstance(self.rows, dict) else self.rows
        return np.arange(N) if r is None else r[r < N]


def _call(torch, case, rows, what):
    """one raw call on the rows `rows` of the inputs, everything in guarded buffers -> ({output name: (len(rows), width) array}, last_launch())"""
    N = len(rows)
    bufs, snap, asked = {}, {}, set()
    for name, i in case.ins.items():
        a = i.a if i.fixed else i.a[rows]
        bufs[name] = Guarded(torch, a.shape[0], a.shape[1], i.dtype, DEV()).load(torch, a)
        snap[name] = bufs[name].bits.clone()
    for o in case.outs:
        bufs[o.name] = Guarded(torch, N, o.width, o.dtype, DEV())

    def p(name):
        if name is None:
            return None
        asked.add(name)
        return bufs[name].ptr
    p.address_of = lambda name: bufs[name].ptr          # without asking for it (tests/test_flush_guard_engine.py: a stand-in that writes where it was not told to)
    _lib.check(getattr(_lib.lib(), case.fn)(*case.args(N, p, _lib.current_stream_ptr())))
    launch = _lib.last_launch()
    torch.cuda.synchronize()
    for name in case.ins:
        assert torch.equal(bufs[name].bits, snap[name]), what + (name, "an input buffer was written")
    res = {}
    for o in case.outs:
        g = bufs[o.name]
        assert g.guards_intact(), what + (o.name, "guard rows written")
        if o.name not in asked:
            assert bool((g.bits == g.pattern).all()), what + (o.name, "an output that was not asked for was written")
            continue
        res[o.name] = g.live().cpu().numpy().copy()
    return res, launch


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _compare(case, rid, res, N):
    for name, ref in case.ref.items():
        rows = case.rows_of(name, N)
        if not len(rows):
            continue
        got, want = res[name][rows].astype(np.float64), ref[rows]
        assert np.isfinite(want).all(), (rid, N, name, "the oracle has no value on a row it is compared on")
        assert N < NMAX or case.zero_ok or np.abs(want).max() > 0, (rid, name, "the oracle is zero everywhere: nothing is compared")
        e = case.err(name, got, want) if case.err else np.abs(got - want)
        t = np.broadcast_to(np.asarray(case.tol(name, want, rows), dtype=np.float64), e.shape)
        key = (case.fn, name)
        w = WORST.setdefault(rid, {}).setdefault(key, [0.0, 0.0])
        ratio = e / np.maximum(t, 1e-300)
        w[0], w[1] = max(w[0], float(e.max())), max(w[1], float(ratio.max()))
        assert bool((e <= t).all()), (rid, N, name, "max deviation %.3e, %.3g of its bound, row %d" % (e.max(), ratio.max(), rows[int(np.argmax(ratio.reshape(len(rows), -1).max(axis=1)))]))


def _compare_second(case, rid, by_size):
    """every row of the N = NMAX result against the second reference, then every smaller N against the leading rows of that result, bit for bit"""
    full = by_size[NMAX]
    for name, want in case.second().items():
        got = full[name].astype(np.float64)
        assert want.shape == got.shape and np.isfinite(want).all(), (rid, name, "the second reference has no value on some row")
        e = np.abs(got - want)
        t = np.broadcast_to(np.asarray(case.tol2(name, want), dtype=np.float64), e.shape)
        ratio = e / np.maximum(t, 1e-300)
        w = WORST.setdefault(rid, {}).setdefault((case.fn, name + " (second reference, all rows)"), [0.0, 0.0])
        w[0], w[1] = max(w[0], float(e.max())), max(w[1], float(ratio.max()))
        assert bool((e <= t).all()), (rid, name, "second reference: max deviation %.3e, %.3g of its bound, row %d" % (
            e.max(), ratio.max(), int(np.argmax(ratio.reshape(NMAX, -1).max(axis=1)))))
    for N, res in by_size.items():
        for name, got in res.items():
            assert _same_bits(got, full[name][:N]), (rid, N, name, "differs from the leading rows of the N = %d result" % NMAX)


ROWS = []          # (id, entry point, knobs, builder of the Case)


def row(rid, fn, knobs, build):
    assert rid not in {r[0] for r in ROWS}, rid
    ROWS.append((rid, fn, dict(knobs or {}), build))


def _run(rid):
    _, fn, knobs, build = next(r for r in ROWS if r[0] == rid)
    _run_row(rid, fn, knobs, build)


def _run_row(rid, fn, knobs, build):
    import torch
    for k, v in knobs.items():
        rtbhip.tune(k, v)
    case = build()
    assert case.fn == fn
    alone = {int(r): _call(torch, case, np.array([r]), (rid, "row %d alone" % r))[0] for r in SEAM_ROWS}
    by_size = {}
    for N in SIZES:
        res, launch = _call(torch, case, np.arange(N), (rid, N))
        by_size[N] = res
        if case.launch is not None and not replaying():
            grid, lds = case.launch(N)
            assert launch[0] == grid and launch[1] == 64, (rid, N, "launch", launch, "expected grid", grid)
            assert lds is None or launch[2] == lds, (rid, N, "launch", launch, "expected LDS bytes", lds)
        for name, got in res.items():
            assert got.shape[0] == N
            if got.dtype.kind == "f" and case.check is None:
                assert np.isfinite(got).all(), (rid, N, name, "a row that is not finite", np.argwhere(~np.isfinite(got))[:4].tolist())
            for r in SEAM_ROWS[SEAM_ROWS < N]:
                assert _same_bits(got[r:r + 1], alone[int(r)][name]), (rid, N, name, "row %d differs from the same row computed alone" % r)
        if case.check is not None:
            case.check(rid, res, N)
        else:
            _compare(case, rid, res, N)
        if N == NMAX and case.twin:
            for k, v in case.twin.items():
                rtbhip.tune(k, v)
            other, _ = _call(torch, case, np.arange(N), (rid, N, "twin"))
            for k, v in knobs.items():
                rtbhip.tune(k, v)
            for name in res:
                assert _same_bits(res[name], other[name]), (rid, name, "bits differ under", case.twin)
        if N == NMAX and case.same_as is not None:
            other, _ = _call(torch, case.same_as(), np.arange(N), (rid, N, "every output asked for"))
            for name in res:
                assert _same_bits(res[name], other[name]), (rid, name, "bits differ from the call with every output asked for")
    if case.second is not None:
        _compare_second(case, rid, by_size)
    for (f, name), (e, ratio) in sorted(WORST.get(rid, {}).items()):
        print("flush_guard_all %s: %s %s max deviation %.3e (%.3g of its bound)" % (rid, f, name, e, ratio))


def _tiles(N):
    return (N + 63) // 64


def _grid_only(N):
    return _tiles(N), None


def _sparse(rows, out):
    """(NMAX, ...) with `out` on `rows`, NaN elsewhere"""
    out = np.asarray(out, dtype=np.float64)
    full = np.full((NMAX,) + out.shape[1:], np.nan)
    full[rows] = out
    return full.reshape(NMAX, -1)


def _flat(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(a.shape[0], -1)


def _rng(*key):
    return np.random.default_rng([sum(map(ord, k)) if isinstance(k, str) else int(k) for k in key])


# ------------------------------------------------------------------------------------------------ chains
def _serial(n, seed):
    from test_kin_flush_guard_gpu import _serial as serial          # the all-revolute chains of the fkine / Jacobian flush-guard test
    return serial(n, seed)


@functools.lru_cache(maxsize=None)
def _chain(name):
    """(product ETS, oracle Chain).  panda: the ETS model; ur5: the URDF; sN: _serial(N, N), ad hoc -- every row on one runs under jit = 0"""
    if name == "panda":
        return rtbhip.models.Panda().ets(), chains.panda_ets()
    if name == "ur5":
        e = urdf.load("UR5").ets()
        return e, chain_from_ets(e)
    return _serial(int(name[1:]), int(name[1:]))


def _kn(chain, **extra):
    return dict(JIT0 if chain.startswith("s") else {}, **extra)


@functools.lru_cache(maxsize=None)
def _q(chain):
    n = _chain(chain)[0].n
    rng = _rng("q", chain)
    return rng.uniform(-np.pi, np.pi, (NMAX, n)), rng.uniform(-1.0, 1.0, (NMAX, n))


def _tool(with_tool):
    return TOOL if with_tool else None


ABS10 = lambda name, w, rows: 1e-10          # the project's kinematics criterion, 1e-10 absolute (README rows a1-a6; tests/test_kin_flush_guard_gpu.py)


# ------------------------------------------------------------------------------------------------ the Hessian family
@functools.lru_cache(maxsize=None)
def _hess_ref(chain, with_tool, frame):
    return _flat(oracle.hessian(_chain(chain)[1], _q(chain)[0], _tool(with_tool), frame))


# one revolute joint followed by a slide along its own axis: w x v = 0, the Hessian is zero until a tool moves the end point off the axis
ZERO_H = lambda chain, with_tool: chain == "s1" and not with_tool


def _hess_lds(path, n):
    hw = (6 * n * n) | 1
    if path == "tile4":                 # csrc/kin_kernels.hip launch_hess_tile<NJ, 4>: (64 / R) rows of 6 n^2 | 1 doubles
        return 16 * hw * 8
    if path == "tile8":
        return 8 * hw * 8
    if path == "run":                   # k_kin_hess<NJ>: 64 Jacobians of 6 n + 1 doubles
        return 64 * (6 * n + 1) * 8
    assert path == "rt"                 # k_kin: csrc/kin_tile.h kin_lds_bytes(n, q_width)
    return 64 * (max(6 * n, 16) + 1 + n) * 8


def _hessian(chain, frame, with_tool, path, tpw=1):
    def build():
        ets, _ = _chain(chain)
        n = ets.n
        t = _lib.small(_tool(with_tool), 16)
        grid = (lambda N: _tiles(N)) if path != "rt" else (lambda N: (_tiles(N) + tpw - 1) // tpw)
        return Case("rtbhip_hessian", {"q": In(_q(chain)[0])}, [O("H", 6 * n * n)],
                    lambda N, p, s: (ets._handle(), p("q"), N, _lib.host_ptr(t), frame, p("H"), MEM, s),
                    ref={"H": _hess_ref(chain, with_tool, frame)}, tol=ABS10, launch=lambda N: (grid(N), _hess_lds(path, n)),
                    twin={"tiles_per_wave": 1} if tpw > 1 else None, keep=(ets, t), zero_ok=ZERO_H(chain, with_tool))
    return build


REG_N = {"s1": 1, "s2": 2, "s3": 3, "ur5": 6, "panda": 7, "s9": 9, "s10": 10}
for _c in REG_N:
    for _mode, _path in ((0, "tile4"), (1, "run"), (2, "tile8")):
        for _frame, _wt in ((0, False), (1, True)) + (((0, True), (1, False)) if _mode == 0 else ()):
            row("hessian %s mode%d f%d%s" % (_c, _mode, _frame, " tool" if _wt else ""), "rtbhip_hessian", _kn(_c, hess_mode=_mode),
                _hessian(_c, _frame, _wt, _path))
for _c in ("s11", "s12"):
    for _co in (1, 0):
        for _frame, _wt in ((0, False), (1, True)):
            row("hessian %s rt coalesced%d f%d%s" % (_c, _co, _frame, " tool" if _wt else ""), "rtbhip_hessian", _kn(_c, coalesced=_co),
                _hessian(_c, _frame, _wt, "rt"))
for _c in ("s3", "panda", "s10"):
    for _co in (1, 0):
        for _frame, _wt in ((0, True), (1, False)):
            row("hessian %s reg0 coalesced%d f%d%s" % (_c, _co, _frame, " tool" if _wt else ""), "rtbhip_hessian", _kn(_c, reg=0, coalesced=_co),
                _hessian(_c, _frame, _wt, "rt"))
for _c, _kw in (("s12", {}), ("panda", {"reg": 0})):
    for _frame in (0, 1):
        row("hessian %s rt tiles_per_wave2 f%d" % (_c, _frame), "rtbhip_hessian", _kn(_c, tiles_per_wave=2, **_kw), _hessian(_c, _frame, False, "rt", tpw=2))


def _hess_from_jac(chain, frame, with_tool):
    def build():
        _, ch = _chain(chain)
        n = ch.n
        J = oracle.jacob(ch, _q(chain)[0], _tool(with_tool), frame)          # J0 gives hessian0, Je hessiane (include/rtbhip.h)
        # csrc/kin_kernels.hip launch_hess_from_jac_nj: the larger of the Jacobian tile and the R = 4 Hessian tile; k_hess_from_jac_any: none
        lds = max(16 * ((6 * n * n) | 1), 64 * (6 * n + 1)) * 8 if n <= 10 else 0
        return Case("rtbhip_hessian_from_jacobian", {"J": In(J)}, [O("H", 6 * n * n)], lambda N, p, s: (p("J"), N, n, p("H"), MEM, s),
                    ref={"H": _hess_ref(chain, with_tool, frame)}, tol=ABS10, launch=lambda N: (_tiles(N), lds), zero_ok=ZERO_H(chain, with_tool))
    return build


for _c in list(REG_N) + ["s11", "s12", "s14"]:
    for _frame, _wt in ((0, False), (1, True)):
        row("hessian_from_jacobian %s f%d%s" % (_c, _frame, " tool" if _wt else ""), "rtbhip_hessian_from_jacobian", _kn(_c), _hess_from_jac(_c, _frame, _wt))


# ------------------------------------------------------------------------------------------------ pure functions of a supplied Jacobian
METHODS = ("yoshikawa", "minsingular", "invcondition")          # method codes 0, 1, 2 of include/rtbhip.h


def _from_jac_lds(n):
    return 64 * (6 * n + 1) * 8          # csrc/diffjac_kernels.hip: the tile's 64 Jacobians, rows of 6 n + 1 doubles


def _manip_from_jac(chain, method):
    def build():
        from test_diff_kinematics import _reference_manipulability
        _, ch = _chain(chain)
        J = oracle.jacob0(ch, _q(chain)[0])
        want = np.array([_reference_manipulability(J[i], METHODS[method], [1] * 6) for i in range(NMAX)])
        return Case("rtbhip_manipulability_from_jacobian", {"J": In(J)}, [O("m", 1)], lambda N, p, s: (p("J"), N, ch.n, 63, method, p("m"), MEM, s),
                    ref={"m": _flat(want)}, tol=lambda name, w, rows: 1e-10 + 1e-8 * np.abs(w),          # tests/test_diff_kinematics.py:369
                    launch=lambda N: (_tiles(N), _from_jac_lds(ch.n)))
    return build


def _jacobm_from_jac(chain, with_H):
    def build():
        from test_diff_kinematics import _reference_jacobm
        _, ch = _chain(chain)
        q = _q(chain)[0]
        J, H = oracle.jacob0(ch, q), oracle.hessian0(ch, q)
        want = np.array([_reference_jacobm(J[i], H[i], [1] * 6) for i in range(NMAX)])
        ok = np.array([np.linalg.cond(J[i] @ J[i].T) < 1e8 for i in range(NMAX)])          # tests/test_diff_kinematics.py:377-380: away from singular J J^T
        assert ok.sum() > NMAX // 2 and all(ok[N - 1] for N in SIZES)
        scale = np.abs(want[ok]).max()
        ins = {"J": In(J)}
        if with_H:
            ins["Hin"] = In(H)
        return Case("rtbhip_jacobm_from_jacobian", ins, [O("Jm", ch.n)],
                    lambda N, p, s: (p("J"), p("Hin") if with_H else None, N, ch.n, 63, p("Jm"), MEM, s),
                    ref={"Jm": _flat(want)}, rows=np.flatnonzero(ok), tol=lambda name, w, rows: 1e-8 * scale, launch=lambda N: (_tiles(N), _from_jac_lds(ch.n)))
    return build


for _c in ("panda", "ur5"):
    for _m in (0, 1, 2):
        row("manipulability_from_jacobian %s %s" % (_c, METHODS[_m]), "rtbhip_manipulability_from_jacobian", {}, _manip_from_jac(_c, _m))
    for _h in (False, True):
        row("jacobm_from_jacobian %s%s" % (_c, " H supplied" if _h else ""), "rtbhip_jacobm_from_jacobian", {}, _jacobm_from_jac(_c, _h))


# ------------------------------------------------------------------------------------------------ pose errors and p_servo
@functools.lru_cache(maxsize=None)
def _poses():
    ch = chains.panda_ets()
    rng = _rng("poses")
    return oracle.fkine(ch, rng.uniform(-np.pi, np.pi, (NMAX, 7))), oracle.fkine(ch, rng.uniform(-np.pi, np.pi, (NMAX, 7)))


def _rpy_error(Te, Tep):
    """tools/p_servo.py:88-97 restated: eTep = inv(wTe) wTep, e = [eTep.t ; tr2rpy(eTep, "zyx")] (oracle/poe.py restates tr2rpy)"""
    out = np.empty((len(Te), 6))
    for i, (a, b) in enumerate(zip(Te, Tep)):
        E = np.linalg.inv(a) @ b
        out[i, :3], out[i, 3:] = E[:3, 3], poe.tr2rpy_zyx(E[:3, :3])
    return out


def _circle(name, got, want):
    """|got - want| with the three roll-pitch-yaw angles compared on the circle (tests/test_p_servo.py:87-92); method 1 only -- an angle-axis vector
    is no angle on a circle and is compared as it stands (tests/test_03_python_ik_pins.py:94,125)"""
    d = got - want
    if name != "arrived":
        d[:, 3:] = (d[:, 3:] + np.pi) % (2 * np.pi) - np.pi
    return np.abs(d)


GAIN = np.array([1.0, 2.0, 3.0, 0.5, 0.25, 4.0])
THRESHOLD = 2.5
AA_LDS = 2 * 64 * 17 * 8          # csrc/kin_kernels.hip:432,449: two operand tiles of kAaStride = 17 doubles


def _pose_error(fn, form, method):
    def build():
        Te, Tep = _poses()
        if form == "Te once":
            Te = np.repeat(Te[:1], NMAX, axis=0)
        if form == "Tep once":
            Tep = np.repeat(Tep[:1], NMAX, axis=0)
        ins = {"Te": In(Te[:1] if form == "Te once" else Te, fixed=form == "Te once"), "Tep": In(Tep[:1] if form == "Tep once" else Tep, fixed=form == "Tep once")}
        na = (lambda N: 1) if form == "Te once" else (lambda N: N)
        nb = (lambda N: 1) if form == "Tep once" else (lambda N: N)
        if method == 0:
            e = np.array([oracle.angle_axis(a, b) for a, b in zip(Te, Tep)])
            te = angle_axis_tolerance(Te, Tep)[:, None] * np.ones(6)          # tests/helpers.py: per pair, by the distance from a half turn
        else:
            e, te = _rpy_error(Te, Tep), np.full((NMAX, 6), 1e-11)                 # tests/test_p_servo.py:95-97, away from the pitch singularity
            assert np.abs(np.abs(e[:, 4]) - np.pi / 2).min() > 1e-3
        tol_of = {}
        if fn == "rtbhip_angle_axis":
            outs, ref = [O("e", 6)], {"e": e}
            args = lambda N, p, s: (p("Te"), na(N), p("Tep"), nb(N), p("e"), MEM, s)
            tol_of["e"] = te
        elif fn == "rtbhip_p_servo_error":
            outs, ref = [O("e", 6)], {"e": e}
            args = lambda N, p, s: (p("Te"), na(N), p("Tep"), nb(N), method, p("e"), MEM, s)
            tol_of["e"] = te
        else:
            total = np.abs(e).sum(axis=1)
            outs, ref = [O("v", 6), O("arrived", 1, "uint8")], {"v": e * GAIN, "arrived": _flat((total < THRESHOLD).astype(np.float64))}
            args = lambda N, p, s: (p("Te"), na(N), p("Tep"), nb(N), method, GAIN.ctypes.data, THRESHOLD, p("v"), p("arrived"), MEM, s)
            tol_of["v"], tol_of["arrived"] = te * GAIN, np.zeros((NMAX, 1))
            rows = {"arrived": np.flatnonzero(np.abs(total - THRESHOLD) > 1e-5)}          # tests/test_p_servo.py:133: off the threshold itself
        return Case(fn, ins, outs, args, ref=ref, err=_circle if method == 1 else None, launch=lambda N: (_tiles(N), AA_LDS), rows=rows if fn == "rtbhip_p_servo" else None,
                    tol=lambda name, w, rows: tol_of[name][rows])          # (the bound is per pair)
    return build


for _form in ("equal counts", "Te once", "Tep once"):
    row("angle_axis %s" % _form, "rtbhip_angle_axis", {}, _pose_error("rtbhip_angle_axis", _form, 0))
    for _m in (0, 1):
        row("p_servo_error %s method%d" % (_form, _m), "rtbhip_p_servo_error", {}, _pose_error("rtbhip_p_servo_error", _form, _m))
        row("p_servo %s method%d" % (_form, _m), "rtbhip_p_servo", {}, _pose_error("rtbhip_p_servo", _form, _m))


# ------------------------------------------------------------------------------------------------ differential kinematics of a chain
REPS = ("rpy/xyz", "rpy/zyx", "eul", "exp")          # representation codes 0..3 of include/rtbhip.h


def _reg_lds(n):
    return max(32 * (6 * n + 1), 64 * 17) * 8          # csrc/kin_reg.h reg_lds_doubles: the larger of a 32-row Jacobian round and the 64 x 17 pose tile


def _diff(fn, chain, **kw):
    def build():
        ets, ch = _chain(chain)
        n, h = ets.n, ets._handle()
        q, qd = _q(chain)
        ins, rows = {"q": In(q)}, None
        if fn == "rtbhip_jacob_dot":                                   # tests/test_diff_kinematics.py:211-212
            frame = kw["frame"]
            ins["qd"] = In(qd)
            outs, ref, tol = [O("Jd", 6 * n)], {"Jd": _flat(oracle.jacob_dot(ch, q, qd, None, frame))}, ABS10
            args = lambda N, p, s: (h, p("q"), p("qd"), N, None, frame, p("Jd"), MEM, s)
        elif fn == "rtbhip_jacob0_analytical":                         # tests/test_diff_kinematics.py:198
            rep = kw["rep"]
            outs, ref, tol = [O("Ja", 6 * n)], {"Ja": _flat(oracle.jacob0_analytical(ch, q, REPS[rep]))}, lambda name, w, rows: 1e-9
            args = lambda N, p, s: (h, p("q"), N, None, rep, p("Ja"), MEM, s)
        elif fn == "rtbhip_jacob0_dot_analytical":                     # tests/test_diff_kinematics.py:124-126: 2e-5 max(1, |ref|max)
            rep = kw["rep"]
            ins["qd"] = In(qd)
            rows = ALL_ROWS
            outs, ref = [O("Jd", 6 * n)], {"Jd": _sparse(rows, oracle.jacob0_dot_analytical(ch, q[rows], qd[rows], REPS[rep]))}
            tol = lambda name, w, rows: 2e-5 * max(1.0, np.abs(w).max())
            args = lambda N, p, s: (h, p("q"), p("qd"), N, None, rep, p("Jd"), MEM, s)
        elif fn == "rtbhip_manipulability":                            # tests/test_diff_kinematics.py:218-221
            m = kw["method"]
            outs, ref = [O("m", 1)], {"m": _flat(oracle.manipulability(ch, q, "all", method=METHODS[m]))}
            tol = (lambda name, w, rows: 1e-12 + 1e-9 * np.abs(w)) if m == 0 else (lambda name, w, rows: 1e-9 + 1e-7 * np.abs(w))
            args = lambda N, p, s: (h, p("q"), N, None, 63, m, p("m"), MEM, s)
        else:                                                          # tests/test_diff_kinematics.py:223-224
            assert fn == "rtbhip_jacobm"
            outs, ref = [O("Jm", n)], {"Jm": _flat(oracle.jacobm(ch, q, "all"))}
            tol = lambda name, w, rows: 1e-9 * max(1.0, np.abs(w).max()) + 1e-7 * np.abs(w)
            args = lambda N, p, s: (h, p("q"), N, None, 63, p("Jm"), MEM, s)
        return Case(fn, ins, outs, args, ref=ref, tol=tol, rows=rows, launch=lambda N: (_tiles(N), _reg_lds(n)), keep=ets)
    return build


for _c in ("panda", "ur5"):
    for _f in (0, 1):
        row("jacob_dot %s f%d" % (_c, _f), "rtbhip_jacob_dot", {}, _diff("rtbhip_jacob_dot", _c, frame=_f))
    for _r in (0, 3):
        row("jacob0_analytical %s %s" % (_c, REPS[_r]), "rtbhip_jacob0_analytical", {}, _diff("rtbhip_jacob0_analytical", _c, rep=_r))
        row("jacob0_dot_analytical %s %s" % (_c, REPS[_r]), "rtbhip_jacob0_dot_analytical", {}, _diff("rtbhip_jacob0_dot_analytical", _c, rep=_r))
    for _m in (0, 1, 2):
        row("manipulability %s %s" % (_c, METHODS[_m]), "rtbhip_manipulability", {}, _diff("rtbhip_manipulability", _c, method=_m))
    row("jacobm %s" % _c, "rtbhip_jacobm", {}, _diff("rtbhip_jacobm", _c))


# ------------------------------------------------------------------------------------------------ link frames
def _link_frames(chain, marks, with_base):
    def build():
        ets, ch = _chain(chain)
        mk = np.ascontiguousarray(marks if marks is not None else [0, 3, len(ets.optable())], dtype=np.int32)
        b = _lib.small(BASE if with_base else None, 16)
        ref = oracle.link_frames(ch, _q(chain)[0], [int(m) for m in mk], base=BASE if with_base else None)          # tests/test_fkine_all.py:73
        return Case("rtbhip_link_frames", {"q": In(_q(chain)[0])}, [O("F", 16 * len(mk))],
                    lambda N, p, s: (ets._handle(), p("q"), N, _lib.host_ptr(b), _lib.host_ptr(mk), len(mk), p("F"), MEM, s),
                    ref={"F": _flat(ref)}, tol=ABS10, launch=lambda N: (_tiles(N), 64 * 17 * 8), keep=(ets, b, mk))          # csrc/frames_kernels.hip:57
    return build


row("link_frames panda 9 marks base", "rtbhip_link_frames", {}, _link_frames("panda", [0, 2, 4, 7, 10, 14, 16, 20, 22], True))
row("link_frames ur5 3 marks", "rtbhip_link_frames", {}, _link_frames("ur5", None, False))
row("link_frames s12 4 marks", "rtbhip_link_frames", JIT0, _link_frames("s12", [0, 5, 5, 17], False))


# ------------------------------------------------------------------------------------------------ DH dynamics
@functools.lru_cache(maxsize=None)
def _dh(name):
    import rne_vjp_cases
    return rne_vjp_cases.robot(name)          # puma560 (6, standard DH), panda (7, modified DH), n9s, n12m: the robots of tests/rne_vjp_cases.py


@functools.lru_cache(maxsize=None)
def _dyn_inputs(name, n, f32=False):
    rng = _rng("dyn", name)
    a = [rng.uniform(-np.pi, np.pi, (NMAX, n)), rng.uniform(-2, 2, (NMAX, n)), rng.uniform(-2, 2, (NMAX, n)), rng.uniform(-1, 1, (NMAX, n))]
    if f32:
        a = [x.astype(np.float32).astype(np.float64) for x in a]
    return a


FEXT = np.array([1.5, -2.0, 0.7, 0.3, -0.4, 0.9])
RNE_TOL = lambda name, w, rows: 1e-9 * max(1.0, np.abs(w).max())                                     # rne's contract: tests/test_erobot_rne.py:311, tests/rne_vjp_cases.py:10
RNE_TOL32 = lambda name, w, rows: 1e-9 * max(1.0, np.abs(w).max()) + 2.0 ** -24 * np.abs(w)          # ... and one rounding to float32 (tests/test_kin_flush_guard_gpu.py)


def _rne(name, form):
    def build():
        rb = _dh(name)
        n, h, L, mdh = rb.n, rb._dyn_handle(), rb.L24(), rb.mdh
        f32 = form == "f32"
        q, qd, qdd, _ = _dyn_inputs(name, n, f32)
        gc = np.ascontiguousarray(rb._gravity_c(None), dtype=np.float64)
        fext = FEXT if form == "fext" else None
        dt = "float32" if f32 else "float64"
        ins = {"q": In(q, dt), "qd": In(qd, dt), "qdd": In(qdd, dt)}
        tau = oracle.rne_dh(L, mdh, q, qd, qdd, gc, fext)
        if form == "base_wrench":
            from test_base_wrench_balance import balance_wrench, frame0_gravity          # the momentum balance that test holds wbase to, 2e-5 of its scale (:135-143)
            rows = ALL_ROWS
            W = np.array([np.concatenate(balance_wrench(rb, q[r], qd[r], qdd[r], frame0_gravity(rb))) for r in rows])
            scale = _sparse(rows, np.maximum(1.0, np.abs(W).max(axis=1))[:, None] * np.ones(6))
            return Case("rtbhip_rne_base_wrench", ins, [O("tau", n), O("wbase", 6)],
                        lambda N, p, s: (h, p("q"), p("qd"), p("qdd"), N, _lib.host_ptr(gc), None, p("tau"), p("wbase"), MEM, s),
                        ref={"tau": tau, "wbase": _sparse(rows, W)}, rows={"wbase": rows},
                        tol=lambda nm, w, rows: RNE_TOL(nm, w, rows) if nm == "tau" else 2e-5 * scale[rows], launch=_grid_only, keep=(rb, gc))
        return Case("rtbhip_rne_f32" if f32 else "rtbhip_rne", ins, [O("tau", n, dt)],
                    lambda N, p, s: (h, p("q"), p("qd"), p("qdd"), N, _lib.host_ptr(gc), _lib.host_ptr(fext), p("tau"), MEM, s),
                    ref={"tau": tau}, tol=RNE_TOL32 if f32 else RNE_TOL, keep=(rb, gc, fext),
                    launch=lambda N: (_tiles(N), 64 * ((3 * n) | 1) * 8))          # csrc/rne_kernels.hip: q, qd, qdd rows of 3 n doubles, made odd (fp64 tile in both forms)
    return build


def _dyn(name, fn):
    def build():
        rb = _dh(name)
        n, h, L, mdh = rb.n, rb._dyn_handle(), rb.L24(), rb.mdh
        q, qd, tq, _ = _dyn_inputs(name, n)
        gc = np.ascontiguousarray(rb._gravity_c(None), dtype=np.float64)
        if fn == "rtbhip_inertia":          # tests/test_dynamics_terms.py:184
            return Case(fn, {"q": In(q)}, [O("M", n * n)], lambda N, p, s: (h, p("q"), N, p("M"), MEM, s), ref={"M": _flat(oracle.inertia_dh(L, mdh, q))},
                        tol=lambda nm, w, rows: 1e-12 + 1e-11 * np.abs(w), launch=_grid_only, keep=rb)
        if fn == "rtbhip_coriolis":         # tests/test_dynamics_terms.py:186
            return Case(fn, {"q": In(q), "qd": In(qd)}, [O("C", n * n)], lambda N, p, s: (h, p("q"), p("qd"), N, p("C"), MEM, s),
                        ref={"C": _flat(oracle.coriolis_dh(L, mdh, q, qd))}, tol=lambda nm, w, rows: 1e-11 + 1e-10 * np.abs(w), launch=_grid_only, keep=rb)
        ref = oracle.accel_dh(L, mdh, q, qd, tq, gc)          # tests/test_dynamics_terms.py:188-189
        scale = np.abs(ref).max()
        return Case(fn, {"q": In(q), "qd": In(qd), "tq": In(tq)}, [O("qdd", n)],
                    lambda N, p, s: (h, p("q"), p("qd"), p("tq"), N, _lib.host_ptr(gc), p("qdd"), MEM, s),
                    ref={"qdd": ref}, tol=lambda nm, w, rows: 1e-9 * scale + 1e-9 * np.abs(w), launch=_grid_only, keep=(rb, gc))
    return build


for _r in ("panda", "puma560"):
    for _form in ("plain", "fext"):
        row("rne %s %s" % (_r, _form), "rtbhip_rne", {}, _rne(_r, _form))
    row("rne_f32 %s" % _r, "rtbhip_rne_f32", {}, _rne(_r, "f32"))
    row("rne_base_wrench %s" % _r, "rtbhip_rne_base_wrench", {}, _rne(_r, "base_wrench"))
    for _fn in ("rtbhip_inertia", "rtbhip_coriolis", "rtbhip_accel"):
        row("%s %s" % (_fn[7:], _r), _fn, {}, _dyn(_r, _fn))
for _r in ("n9s", "n12m"):                      # (N n float32 torques: with n = 7, 9 every residue of the four-float piece over SIZES)
    row("rne %s plain" % _r, "rtbhip_rne", JIT0, _rne(_r, "plain"))
    row("rne_f32 %s" % _r, "rtbhip_rne_f32", JIT0, _rne(_r, "f32"))


# ------------------------------------------------------------------------------------------------ link trees
@functools.lru_cache(maxsize=None)
def _tree(name):
    """(ERobot, the oracle's link list), all of tests/tree_rne_vjp_cases.py: UR5 (6 joints) and KinovaGen3 (13) from their URDF files; tree7
    (branched, a prismatic and a flipped joint), chain8 and tree9 ad hoc -- under jit = 0.  (The Panda URDF carries no masses: every torque is zero.)"""
    import tree_rne_vjp_cases as tc
    return tc.robot(name)


TREE_KN = {"UR5": {}, "KinovaGen3": {}, "tree7": JIT0, "chain8": JIT0, "tree9": JIT0}


def _tree_case(name, fn, null_rates=False):
    def build():
        rob, orc = _tree(name)
        n, h = rob.n, rob._handle()
        q, qd, tq, _ = _dyn_inputs("tree " + name, n)
        g = np.ascontiguousarray(rob.gravity, dtype=np.float64).reshape(3)
        scaled = lambda k: (lambda nm, w, rows: k * max(1.0, np.abs(w).max()))
        if fn == "rtbhip_tree_rne":              # tests/test_erobot_rne.py:222
            z = np.zeros_like(q)
            ref = oer.erobot_rne(orc, q, z if null_rates else qd, z if null_rates else tq, g)
            ins = {"q": In(q)} if null_rates else {"q": In(q), "qd": In(qd), "qdd": In(tq)}
            return Case(fn, ins, [O("tau", n)], lambda N, p, s: (h, p("q"), None if null_rates else p("qd"), None if null_rates else p("qdd"), N, _lib.host_ptr(g),
                                                                 p("tau"), MEM, s),
                        ref={"tau": ref}, tol=lambda nm, w, rows: 1e-10 * max(1.0, np.abs(w).max()) + 1e-10 * np.abs(w), launch=_grid_only, keep=(rob, g))
        if fn == "rtbhip_tree_inertia":          # tests/test_erobot_dynamics.py:220
            return Case(fn, {"q": In(q)}, [O("M", n * n)], lambda N, p, s: (h, p("q"), N, p("M"), MEM, s), ref={"M": _flat(oer.erobot_inertia(orc, q))},
                        tol=scaled(1e-12), launch=_grid_only, keep=rob)
        rows = ALL_ROWS
        if fn == "rtbhip_tree_coriolis":         # tests/test_erobot_dynamics.py:223
            return Case(fn, {"q": In(q), "qd": In(qd)}, [O("C", n * n)], lambda N, p, s: (h, p("q"), p("qd"), N, p("C"), MEM, s),
                        ref={"C": _sparse(rows, oer.erobot_coriolis(orc, q[rows], qd[rows]))}, rows=rows, tol=scaled(1e-12), launch=_grid_only, keep=rob)
        assert np.linalg.cond(oer.erobot_inertia(orc, q[rows])).max() < 1e8          # tests/test_erobot_dynamics.py:230-233
        want = oer.erobot_accel(orc, q[rows], qd[rows], tq[rows], g)
        return Case(fn, {"q": In(q), "qd": In(qd), "tq": In(tq)}, [O("qdd", n)],
                    lambda N, p, s: (h, p("q"), p("qd"), p("tq"), N, _lib.host_ptr(g), p("qdd"), MEM, s),
                    ref={"qdd": _sparse(rows, want)}, rows=rows, tol=lambda nm, w, rows: 1e-8 * max(1.0, np.abs(w).max()) + 1e-8 * np.abs(w), launch=_grid_only,
                    keep=(rob, g))
    return build


for _r in ("UR5", "KinovaGen3", "tree7"):
    row("tree_rne %s" % _r, "rtbhip_tree_rne", TREE_KN[_r], _tree_case(_r, "rtbhip_tree_rne"))
    row("tree_rne %s NULL qd qdd" % _r, "rtbhip_tree_rne", TREE_KN[_r], _tree_case(_r, "rtbhip_tree_rne", True))
for _r in ("UR5", "tree7"):
    row("tree_inertia %s" % _r, "rtbhip_tree_inertia", TREE_KN[_r], _tree_case(_r, "rtbhip_tree_inertia"))
    row("tree_coriolis %s" % _r, "rtbhip_tree_coriolis", TREE_KN[_r], _tree_case(_r, "rtbhip_tree_coriolis"))
for _r in ("tree7", "chain8"):
    row("tree_accel %s" % _r, "rtbhip_tree_accel", TREE_KN[_r], _tree_case(_r, "rtbhip_tree_accel"))


# ------------------------------------------------------------------------------------------------ inverse kinematics
@functools.lru_cache(maxsize=None)
def _ik_problem(chain):
    """targets reached from inside the limits and starts near their solutions: q0 supplied and slimit = 1, so no restart is drawn
    (tests/test_staged_host_path.py:125, tests/test_00_gpu_parity.py:776-790)"""
    if chain == "panda":
        ets = rtbhip.models.Panda().ets()
        ets.qlim = chains.PANDA_QLIM
        ch = chains.panda_ets(with_limits=True)
    else:
        ets = urdf.load("UR5").ets()
        ets.qlim = np.clip(ets.qlim, -np.pi, np.pi)
        ch = chain_from_ets(ets)
    rng = _rng("ik", chain)
    qs = rng.uniform(ch.qlim[0] * 0.8, ch.qlim[1] * 0.8, (NMAX, ch.n))
    q0 = np.clip(qs + 0.15 * rng.normal(size=qs.shape), ch.qlim[0] + 0.02, ch.qlim[1] - 0.02)
    return ets, ch, oracle.fkine(ch, qs), q0


def _ik(chain, solver):
    def build():
        ets, ch, Tep, q0 = _ik_problem(chain)
        n, h = ets.n, ets._handle()
        outs = [O("q", n), O("success", 1, "int32"), O("iters", 1, "int32"), O("searches", 1, "int32"), O("residual", 1)]
        po = lambda p: (p("q"), p("success"), p("iters"), p("searches"), p("residual"))
        pi = np.full(n, 0.5)
        if solver == "lm":               # flavour 0, the C loop: the compiled oracle, every row (tests/test_00_gpu_parity.py:785-789)
            fn, rows, atol = "rtbhip_ik_lm", np.arange(NMAX), 1e-6
            args = lambda N, p, s: (h, p("Tep"), N, p("q0"), 30, 1, 1e-6, 1, None, 1.0, 0, 0, 0) + po(p) + (MEM, s)
            solve = lambda i: oracle.ik_lm(ch, Tep[i], q0=q0[i], restarts=np.zeros((2, n)), slimit=1)
        elif solver == "nullspace":      # flavour 1 with the null-space terms: the Python restatement (tests/test_00_gpu_parity.py:462-466)
            fn, rows, atol = "rtbhip_ik_lm_nullspace", ALL_ROWS, 1e-6
            args = lambda N, p, s: (h, p("Tep"), N, p("q0"), 30, 1, 1e-6, 1, None, 1.0, 0, 1, 0, 0.1, 0.1, 0.0, None) + po(p) + (MEM, s)
            solve = lambda i: oracle.ikine_py(ch, Tep[i], np.array([q0[i]]), step="lm", slimit=1, k=1.0, kq=0.1, km=0.1, ps=0.0, pi=0.3, method="chan")
        else:                            # the QP step with inequality rows (tests/test_00_gpu_parity.py:817-824)
            fn, rows, atol = "rtbhip_ik_qp", ALL_ROWS, 1e-7
            args = lambda N, p, s: (h, p("Tep"), N, p("q0"), 30, 1, 1e-6, 1, None, 0, 0.01, 1.0, 1.0, 0.0, 0.0, _lib.host_ptr(pi)) + po(p) + (MEM, s)
            solve = lambda i: oracle.ikine_py(ch, Tep[i], np.array([q0[i]]), step="qp", slimit=1, ks=1.0, kj=0.01, kq=1.0, ps=0.0, pi=0.5)
        want = {int(i): solve(int(i)) for i in rows}
        assert sum(1 for o in want.values() if o[1]) >= len(rows) // 3          # the comparison below is on the targets the oracle solves

        def check(rid, res, N):
            """(success, iterations, searches) and q where the oracle converges, as the family's tests compare them; success in {0, 1}, one search, at most
            ilimit iterations on every row"""
            ok, it, se = res["success"][:, 0], res["iters"][:, 0], res["searches"][:, 0]
            assert set(np.unique(ok)) <= {0, 1} and it.min() >= 1 and it.max() <= 30 and set(np.unique(se)) <= {1}, (rid, N)
            # (a search that fails may end on NaN: the restated reference's own loop does on such a target, oracle.ikine_py)
            assert np.isfinite(res["q"][ok == 1]).all() and np.isfinite(res["residual"][ok == 1]).all() and (ok == 1).sum() >= N // 3, (rid, N)
            for i in rows[rows < N]:
                o = want[int(i)]
                if o[1]:
                    assert (o[1], o[2], o[3]) == (ok[i], it[i], se[i]), (rid, N, int(i), (o[1], o[2], o[3]), (ok[i], it[i], se[i]))
                    e = float(np.abs(res["q"][i] - o[0]).max())
                    w = WORST.setdefault(rid, {}).setdefault((fn, "q"), [0.0, 0.0])
                    w[0], w[1] = max(w[0], e), max(w[1], e / atol)
                    assert e <= atol, (rid, N, int(i), e)
        return Case(fn, {"Tep": In(Tep), "q0": In(q0)}, outs, args, check=check, keep=(ets, pi))
    return build


row("ik_lm panda", "rtbhip_ik_lm", {}, _ik("panda", "lm"))
row("ik_lm ur5", "rtbhip_ik_lm", {}, _ik("ur5", "lm"))
row("ik_lm_nullspace panda", "rtbhip_ik_lm_nullspace", {}, _ik("panda", "nullspace"))
row("ik_qp ur5", "rtbhip_ik_qp", {}, _ik("ur5", "qp"))


# ------------------------------------------------------------------------------------------------ the adjoints
SUBSETS = {"all": (True, True, True), "gq": (True, False, False), "gqd": (False, True, False), "gqdd": (False, False, True)}          # tests/test_rne_vjp.py:241-261
VJP_TOL = lambda name, w, rows: 1e-9 * max(1.0, np.abs(w).max())                                  # tests/rne_vjp_cases.py: BOUND on rel_err
VJP_TOL32 = lambda name, w, rows: 1e-9 * max(1.0, np.abs(w).max()) + 2.0 ** -24 * np.abs(w)       # ... and one rounding to float32 (tests/test_rne_vjp.py:292-299)
GNAMES = ("gq", "gqd", "gqdd")


def _kin_vjp(chain, mode, form):
    """tests/test_kin_vjp.py: the oracle's T, J and H contracted in NumPy (_oracle_gq), 1e-10 absolute; modes gT / gJ / both (:264-273)"""
    def build():
        from test_kin_vjp import _oracle_gq
        ets, ch = _chain(chain)
        n = ets.n
        f32 = form == "f32"
        rng = _rng("kin_vjp", chain)
        q, gT, gJ = _q(chain)[0], rng.uniform(-1, 1, (NMAX, 4, 4)), rng.uniform(-1, 1, (NMAX, 6, n))
        if f32:
            q, gT, gJ = [x.astype(np.float32).astype(np.float64) for x in (q, gT, gJ)]
        with_tb = form != "from_jacobian" and chain != "ur5"
        tool, base = (TOOL, BASE) if with_tb else (None, None)
        pose, jac = _oracle_gq(ets, q, tool, base, gT, gJ)
        ref = (pose if mode != "gJ" else 0.0) + (jac if mode != "gT" else 0.0)
        dt = "float32" if f32 else "float64"
        ins = {"q": In(q, dt), "gT": In(gT, dt), "gJ": In(gJ, dt)}
        a, b = ("gT" if mode != "gJ" else None), ("gJ" if mode != "gT" else None)
        t, bs = _lib.small(tool, 16), _lib.small(base, 16)
        tol = (lambda nm, w, rows: 1e-10 + 2.0 ** -24 * np.abs(w)) if f32 else ABS10
        if form == "from_jacobian":
            del ins["q"]
            ins["T"], ins["J"] = In(oracle.fkine(ch, q)), In(oracle.jacob0(ch, q))
            args = lambda N, p, s: (p("T") if a else None, p("J"), p(a), p(b), N, n, p("gq"), MEM, s)
            fn = "rtbhip_kin_vjp_from_jacobian"
            if not a:
                del ins["T"]
        else:
            fn = "rtbhip_fkine_jacob_vjp_f32" if f32 else "rtbhip_fkine_jacob_vjp"
            args = lambda N, p, s: (ets._handle(), p("q"), N, _lib.host_ptr(bs), _lib.host_ptr(t), p(a), p(b), p("gq"), MEM, s)
        for k in ("gT", "gJ"):
            if k not in (a, b):
                del ins[k]
        if form == "from_jacobian" or n > 10:          # csrc/kin_kernels.hip k_vjp_from_jac_any: as many rows of (32 + 12 n + q_width) | 1 doubles as fit 48 KB
            stride = (32 + 12 * n + n) | 1
            lds = min(64, 6144 // stride) * stride * 8
        else:                                          # k_kin_vjp<NJ>: the Jacobian rounds when gJ is given, the pose tile alone otherwise
            lds = (_reg_lds(n) if b else 64 * 17 * 8)
        return Case(fn, ins, [O("gq", n, dt)], args, ref={"gq": ref}, tol=tol, launch=lambda N: (_tiles(N), lds), keep=(ets, t, bs))
    return build


for _c in ("panda", "ur5", "s12"):
    for _mode in ("gT", "gJ", "both"):
        row("fkine_jacob_vjp %s %s" % (_c, _mode), "rtbhip_fkine_jacob_vjp", _kn(_c), _kin_vjp(_c, _mode, "f64"))
        row("kin_vjp_from_jacobian %s %s" % (_c, _mode), "rtbhip_kin_vjp_from_jacobian", _kn(_c), _kin_vjp(_c, _mode, "from_jacobian"))
    row("fkine_jacob_vjp_f32 %s both" % _c, "rtbhip_fkine_jacob_vjp_f32", _kn(_c), _kin_vjp(_c, "both", "f32"))


def _rne_vjp(name, subset, f32=False):
    """tests/test_rne_vjp.py, tests/rne_vjp_cases.py: five-point Richardson differences of the compiled reference, 1e-9 max(1, |ref|max)"""
    def build():
        import rne_vjp_cases as rc
        rb = _dh(name)
        n, h = rb.n, rb._dyn_handle()
        q, qd, qdd, g = rc.draw(rb, NMAX, 4242)          # (keeps |qd| away from the Coulomb jump)
        if f32:
            q, qd, qdd, g = [np.asarray(x).astype(np.float32).astype(np.float64) for x in (q, qd, qdd, g)]
        want = SUBSETS[subset]
        ref = rc.rne_oracle(rb, q, qd, qdd, g, which=tuple(i for i in range(3) if want[i]))
        gc = np.ascontiguousarray(rb._gravity_c(None), dtype=np.float64)
        dt = "float32" if f32 else "float64"
        return Case("rtbhip_rne_vjp_f32" if f32 else "rtbhip_rne_vjp", {"q": In(q, dt), "qd": In(qd, dt), "qdd": In(qdd, dt), "gtau": In(g, dt)},
                    [O(k, n, dt) for k in GNAMES],
                    lambda N, p, s: (h, p("q"), p("qd"), p("qdd"), N, _lib.host_ptr(gc), None, p("gtau")) + tuple(p(k) if w else None for k, w in zip(GNAMES, want)) + (MEM, s),
                    ref={k: ref[i] for i, k in enumerate(GNAMES) if want[i]}, tol=VJP_TOL32 if f32 else VJP_TOL, keep=(rb, gc),
                    launch=lambda N: (_tiles(N), 64 * (4 * n + 1) * 8))          # csrc/rne_vjp_kernels.hip rne_vjp_stride: q, qd, qdd, gtau rows, 4 n + 1 doubles while that fits 64 KB
    return build


for _r in ("puma560", "panda", "n9s", "n12m"):
    _k = {} if _r in ("puma560", "panda") else JIT0
    for _s in SUBSETS:
        row("rne_vjp %s %s" % (_r, _s), "rtbhip_rne_vjp", _k, _rne_vjp(_r, _s))
    row("rne_vjp_f32 %s all" % _r, "rtbhip_rne_vjp_f32", _k, _rne_vjp(_r, "all", True))


@functools.lru_cache(maxsize=None)
def _tree_vjp_ref(name):
    """[gq, gqd, gqdd] on every row: one evaluation of the stencil per robot, shared by its subsets"""
    import tree_rne_vjp_cases as tc
    rob, orc = _tree(name)
    q, qd, qdd, g = _dyn_inputs("tree vjp " + name, rob.n)
    r = ALL_ROWS
    return tc.rne_oracle(orc, q[r], qd[r], qdd[r], g[r], np.ascontiguousarray(rob.gravity, dtype=np.float64).reshape(3))


def _tree_rne_vjp(name, subset):
    """tests/test_tree_rne_vjp.py, tests/tree_rne_vjp_cases.py: the same stencil over oracle/erobot.py on every row, the same bound"""
    def build():
        rob, orc = _tree(name)
        n, h = rob.n, rob._handle()
        q, qd, qdd, g = _dyn_inputs("tree vjp " + name, n)
        want, rows = SUBSETS[subset], ALL_ROWS
        gravity = np.ascontiguousarray(rob.gravity, dtype=np.float64).reshape(3)
        ref = _tree_vjp_ref(name)
        return Case("rtbhip_tree_rne_vjp", {"q": In(q), "qd": In(qd), "qdd": In(qdd), "gtau": In(g)}, [O(k, n) for k in GNAMES],
                    lambda N, p, s: (h, p("q"), p("qd"), p("qdd"), N, _lib.host_ptr(gravity), p("gtau")) + tuple(p(k) if w else None for k, w in zip(GNAMES, want)) + (MEM, s),
                    ref={k: _sparse(rows, ref[i]) for i, k in enumerate(GNAMES) if want[i]}, rows=rows, tol=VJP_TOL, launch=_grid_only, keep=(rob, gravity))
    return build


for _r in ("UR5", "tree7", "tree9"):          # (tree9: the run-time-n kernel of 9..24 groups)
    for _s in SUBSETS if _r != "tree9" else ("all",):
        row("tree_rne_vjp %s %s" % (_r, _s), "rtbhip_tree_rne_vjp", TREE_KN[_r], _tree_rne_vjp(_r, _s))


def _link_frames_vjp(name):
    """tests/test_link_frames_vjp.py, tests/link_frames_vjp_cases.py: one compiled reference call per mark (oracle_gq), 1e-10 absolute"""
    def build():
        import link_frames_vjp_cases as lc
        spec, _, _, cols, width = lc.CASES[name]
        ets, marks, base = lc.ets_of(name), lc.marks_of(name), lc.base_of(name)
        w = ets.q_width
        rng = _rng("frames vjp", name)
        q, G = rng.uniform(-np.pi, np.pi, (NMAX, w)), rng.uniform(-1, 1, (NMAX, len(marks), 4, 4))
        mk, b = np.ascontiguousarray(marks, dtype=np.int32), _lib.small(base, 16)
        return Case("rtbhip_link_frames_vjp", {"q": In(q), "gF": In(G)}, [O("gq", w)],
                    lambda N, p, s: (ets._handle(), p("q"), N, _lib.host_ptr(b), _lib.host_ptr(mk), len(mk), p("gF"), p("gq"), MEM, s),
                    ref={"gq": lc.oracle_gq(spec, marks, q, G, base, cols, width)}, tol=ABS10, keep=(ets, mk, b),
                    launch=lambda N: (_tiles(N), 64 * (2 * 16 + 1 + (w | 1)) * 8))          # csrc/frames_vjp_kernels.hip frames_vjp_lds: two frames of G + 1, and a q row made odd
    return build


for _r in ("panda", "panda_base", "n6", "n9", "n12", "cols"):
    row("link_frames_vjp %s" % _r, "rtbhip_link_frames_vjp", {} if _r.startswith("panda") else JIT0, _link_frames_vjp(_r))


# ------------------------------------------------------------------------------------------------ the adjoints of the inertia and Coriolis matrices
# Inputs as tests/inertia_vjp_cases.py:54-60 and tests/coriolis_vjp_cases.py:58-64 draw them -- q ~ U(-3, 3), qd ~ U(-2, 2), gM / gC ~ U(-1, 1), NOT
# symmetric -- but NMAX DISTINCT rows, drawn once per robot: the family's own cases repeat 8 (or 2) rows cyclically, and a staging or flush error
# that moves a row by a multiple of that period returns exactly the expected bits there.
CSUBSETS = {"both": (True, True), "gq": (True, False), "gqd": (False, True)}          # tests/test_coriolis_vjp.py:334-337
# The rows on which the Python-loop oracle of the tree Coriolis adjoint runs (n + n (n - 1) / 2 inverse-dynamics evaluations per matrix, 5 n matrices
# per row): the first and last row, both sides of the 8-row and 64-row seams, every residue class mod 8, and three classes (0, 7, 1) with two rows
# in one tile.  Every row, these included, is ALSO held to the composition the fused call replaces (Case.second).
ORACLE_ROWS_14 = np.array([0, 2, 7, 8, 11, 20, 29, 38, 63, 64, 65, 73, 127, 128])
ORACLE_ROWS_24 = np.array(sorted(set(ORACLE_ROWS_14.tolist()) | {16, 33, 47, 48, 70, 86, 95, 100, 109, 118}))
for _rows, _least in ((ORACLE_ROWS_14, 12), (ORACLE_ROWS_24, 24)):
    assert len(_rows) >= _least and len(set(_rows.tolist())) == len(_rows) and _rows.max() < NMAX
    assert {0, 7, 8, 63, 64, 65, 127, 128} <= set(_rows.tolist()) and {int(r) % 8 for r in _rows} == set(range(8))
    _pairs = {(int(r) % 8, int(r) // 64) for r in _rows if sum(1 for x in _rows if x % 8 == r % 8 and x // 64 == r // 64) >= 2}
    assert len({c for c, _ in _pairs}) >= 3, _pairs


@functools.lru_cache(maxsize=None)
def _mat_vjp_inputs(kind, name, n):
    rng = _rng(kind, name)
    return rng.uniform(-3, 3, (NMAX, n)), rng.uniform(-2, 2, (NMAX, n)), rng.uniform(-1, 1, (NMAX, n, n))


def _tree_slots_kept(parents):
    """(branch slots, kept groups) of a group table, restated: a group whose parent is not the group in front of it reads the parent's state through a
    slot, one slot per such parent (csrc/tree.cpp:94-101); the adjoint keeps the state of group j unless group j + 1 hangs directly off it
    (csrc/tree_coriolis_vjp_kernels.hip: `kept` in tree_coriolis_vjp_lane, `nkept` in launch_tree_coriolis_vjp)"""
    n = len(parents)
    return len({p for j, p in enumerate(parents) if p >= 0 and p != j - 1}), sum(1 for j in range(n) if j + 1 >= n or parents[j + 1] != j)


def _tree_coriolis_vjp_lds(n, nslots, nkept, rt):
    """csrc/tree_coriolis_vjp_kernels.hip: tree_coriolis_vjp_stride, `lds_of` in launch_tree_coriolis_vjp: q | qd | gC (one row of it in the run-time-n form) at an odd stride, 24 doubles per branch
    slot, and in the register form 18 per kept group"""
    return 64 * 8 * (((2 * n + (n if rt else n * n)) | 1) + 24 * nslots + (0 if rt else 18 * nkept))


@functools.lru_cache(maxsize=None)
def _ladder8():
    """(ERobot, the oracle's link list): 8 groups, group j hanging off group j - 2 (group 1 off group 0), numbered by hand IN group order, which
    keeps the links in the order given (a depth-first numbering cannot produce this table: there a group that does not hang off the one in front of
    it follows a leaf).  6 branch slots and 7 kept groups: the register form of rtbhip_tree_coriolis_vjp would ask for
    64 * 8 * (81 + 24 * 6 + 18 * 7) = 179712 bytes > 160 KB, so launch_tree_coriolis_vjp serves it with the run-time-n form,
    64 * 8 * (25 + 24 * 6) = 86528 bytes (csrc/tree_coriolis_vjp_kernels.hip: `rt` in launch_tree_coriolis_vjp).  One prismatic and one flipped joint."""
    from rtbhip import ET, ETS, Link, ERobot
    rng = _rng("ladder8")
    axes, flips = ("Rz", "Ry", "Rx", "tz", "Rz", "Ry", "Rx", "Rz"), (False, False, True, False, False, False, True, False)
    prod, orc = [], []
    for i, (a, fl) in enumerate(zip(axes, flips)):
        parent = None if i == 0 else max(0, i - 2)
        T = chains.elementary("Rz", rng.uniform(-1, 1)) @ chains.elementary("tx", rng.uniform(-.3, .3)) @ chains.elementary("Rx", rng.uniform(-1, 1))
        m, r = float(rng.uniform(0.5, 3)), rng.uniform(-0.3, 0.3, 3)
        prod.append(Link(ets=ETS() * ET.SE3(T) * getattr(ET, a)(flip=fl), jindex=i, m=m, r=r, parent=None if parent is None else prod[parent], name="d%d" % i))
        orc.append(dict(name="d%d" % i, parent=None if parent is None else "d%d" % parent, ets=[T, (a, None, fl)], m=m, r=r, jindex=i))
    rob = ERobot(prod, name="ladder8")
    parents = [r["parent"] for r in rob.group_table()]
    assert rob.n == 8 and rob._in_group_order() and parents == [-1, 0, 0, 1, 2, 3, 4, 5] and _tree_slots_kept(parents) == (6, 7)
    return rob, orc


# Which trees of at most 8 groups the register form cannot serve: 64 * 8 * (((2 n + n^2) | 1) + 24 nslots + 18 nkept) > 160 * 1024 means more than
# 320 doubles per lane; at n = 8 the row is 81, so 24 nslots + 18 nkept > 239.  A slot needs a parent p with a child j >= p + 2, so nslots <= n - 2 = 6;
# nkept <= n - 1 = 7 with one base link (group 1 hangs off group 0).  (6, 7) gives 270 and (5, 7) 246: both over, (4, 7) 222 is not; n = 7 has a row of
# (14 + 49) | 1 = 63 doubles, at most 5 slots and 6 kept groups: 291 <= 320, the register form.  So only 8-group tables numbered by hand reach the fallback -- _ladder8 is one.
assert _tree_coriolis_vjp_lds(8, 6, 7, False) == 179712 > 160 * 1024 >= _tree_coriolis_vjp_lds(7, 5, 6, False) and _tree_coriolis_vjp_lds(8, 6, 7, True) == 86528
assert _tree_coriolis_vjp_lds(8, 5, 7, False) > 160 * 1024 >= _tree_coriolis_vjp_lds(8, 4, 7, False)


def _mtree(name):
    return _ladder8() if name == "ladder8" else _tree(name)


MAT_DH_KN = lambda name: {} if name in ("puma560", "panda") else JIT0
MAT_TREE_KN = lambda name: {} if name == "UR5" else JIT0


def _mat_dh_robot(name):
    import inertia_vjp_cases as ic
    return ic.dh_robot(name)          # puma560, panda and the random all-revolute tables nNs / nNm of tests/rne_vjp_cases.py, N up to 16


@functools.lru_cache(maxsize=None)
def _inertia_vjp_ref(name, tree):
    """tests/inertia_vjp_cases.py:63-74: five-point Richardson differences, h = 1e-3 (tests/rne_vjp_cases.py:20, 66-76), of the reference's inertia
    matrix, one q column at a time, contracted with gM -- on every one of the NMAX rows, once per robot"""
    import inertia_vjp_cases as ic
    if tree:
        rob, orc = _mtree(name)
        q, _, g = _mat_vjp_inputs("tree inertia vjp", name, rob.n)
        r = _inertia_oracle_rows(name)
        return ic.tree_oracle(orc, q, g) if r is None else _sparse(r, ic.tree_oracle(orc, q[r], g[r]))
    rb = _mat_dh_robot(name)
    q, _, g = _mat_vjp_inputs("inertia vjp", name, rb.n)
    return ic.dh_oracle(rb, q, g)


def _inertia_oracle_rows(name):
    """every row (None) -- but the stencil of the 9-joint tree on 129 rows is 42 000 evaluations of the Python inverse dynamics, three times the
    slowest row this table had: tree9 takes the oracle rows and the composition on every row, as the tree Coriolis rows below do"""
    return ORACLE_ROWS_14 if name == "tree9" else None


@functools.lru_cache(maxsize=None)
def _tree_inertia_composition(name):
    """tests/test_inertia_vjp.py:262-280 (_composition): what the fused call replaces -- n launches of rtbhip_tree_rne_vjp at qd = 0, qdd = e_i,
    gtau = gM[:, i, :], no gravity, summed -- on all NMAX rows"""
    import torch
    from test_inertia_vjp import _composition
    rob, _ = _mtree(name)
    q, _, g = _mat_vjp_inputs("tree inertia vjp", name, rob.n)
    return _composition(rob, *(torch.from_numpy(np.ascontiguousarray(x)).to(DEV()) for x in (q, g))).cpu().numpy()


def _inertia_vjp(name, tree):
    """tests/test_inertia_vjp.py:319-328: the oracle above, bound 1e-9 max(1, |ref|max) (tests/inertia_vjp_cases.py:13; VJP_TOL); where the
    oracle runs on the oracle rows only, every row is also within 2e-9 max(1, |ref|max) of the composition (tests/test_inertia_vjp.py:333-344)"""
    def build():
        rows, second, tol2 = None, None, None
        ref = _inertia_vjp_ref(name, tree)
        if tree:
            rob, _ = _mtree(name)
            n, h, fn, launch = rob.n, rob._handle(), "rtbhip_tree_inertia_vjp", _grid_only          # (its LDS request counts the robot's branch slots)
            q, _, g = _mat_vjp_inputs("tree inertia vjp", name, n)
            rows = _inertia_oracle_rows(name)
            if rows is not None:
                scale = max(1.0, float(np.abs(ref[rows]).max()))
                second, tol2 = (lambda: {"gq": _tree_inertia_composition(name)}), (lambda nm, w: 2e-9 * scale)
        else:
            rob = _mat_dh_robot(name)
            n, h, fn = rob.n, rob._dyn_handle(), "rtbhip_inertia_vjp"
            q, _, g = _mat_vjp_inputs("inertia vjp", name, n)
            # csrc/inertia_vjp_kernels.hip: inertia_vjp_stride, `lds` in launch_inertia_vjp: q (n) | the folded gM (n (n + 1) / 2) at an odd stride, the register and the run-time-n form alike
            launch = lambda N: (_tiles(N), 64 * 8 * ((n + n * (n + 1) // 2) | 1))
        return Case(fn, {"q": In(q), "gM": In(g)}, [O("gq", n)], lambda N, p, s: (h, p("q"), N, p("gM"), p("gq"), MEM, s),
                    ref={"gq": ref}, rows=rows, tol=VJP_TOL, launch=launch, keep=rob, second=second, tol2=tol2)
    return build


for _r in ("puma560", "panda", "n8s", "n9s", "n16m"):          # 6 standard DH, 7 modified DH; 8: the last register size; 9: the first run-time-n size; 16: the limit
    row("inertia_vjp %s" % _r, "rtbhip_inertia_vjp", MAT_DH_KN(_r), _inertia_vjp(_r, False))
for _r in ("UR5", "tree7", "tree8", "tree9"):                  # tree7: branch slots in use; tree8: the last register size; tree9: run-time-n
    row("tree_inertia_vjp %s" % _r, "rtbhip_tree_inertia_vjp", MAT_TREE_KN(_r), _inertia_vjp(_r, True))


def _coriolis_oracle_rows(name):
    return ORACLE_ROWS_14 if name in ("tree9", "ladder8") else ORACLE_ROWS_24          # (the two that the run-time-n form serves)


@functools.lru_cache(maxsize=None)
def _coriolis_vjp_ref(name, tree):
    """tests/coriolis_vjp_cases.py:67-102: gq by the same stencil, h = 1e-3, on the reference's Coriolis matrix; gqd exactly, from the linearity of C
    in qd (gqd[:, m] = sum_jk gC[:, j, k] C(q, e_m)[:, j, k]).  DH: the compiled reference, all NMAX rows.  Trees: the Python loop, on the robot's
    oracle rows only -> (gq, gqd) as (NMAX, n) with NaN on the other rows"""
    import coriolis_vjp_cases as cc
    if tree:
        rob, orc = _mtree(name)
        q, qd, g = _mat_vjp_inputs("tree coriolis vjp", name, rob.n)
        r = _coriolis_oracle_rows(name)
        return tuple(_sparse(r, x) for x in cc.tree_oracle(orc, q[r], qd[r], g[r]))
    rb = _mat_dh_robot(name)
    q, qd, g = _mat_vjp_inputs("coriolis vjp", name, rb.n)
    return cc.dh_oracle(rb, q, qd, g)


@functools.lru_cache(maxsize=None)
def _tree_coriolis_composition(name):
    """tests/test_coriolis_vjp.py:272-291 (_composition): what the fused call replaces -- 2 n launches of rtbhip_tree_rne_vjp at qd +- e_k with
    gtau = +-1/4 gC[:, :, k], summed -- on all NMAX rows, once per robot.  rtbhip_tree_rne_vjp is another kernel, held to the oracle on all 129
    distinct rows by the tree_rne_vjp rows above."""
    import torch
    from test_coriolis_vjp import _composition
    rob, _ = _mtree(name)
    dq, dqd, dg = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV()) for x in _mat_vjp_inputs("tree coriolis vjp", name, rob.n))
    return tuple(x.cpu().numpy() for x in _composition(rob, dq, dqd, dg))


def _coriolis_vjp(name, subset, tree, lds=None):
    """tests/test_coriolis_vjp.py:321-337: both gradients at 1e-9 max(1, |ref|max) (VJP_TOL); gq alone and gqd alone return the bits of the call
    that asks for both (Case.same_as) and leave the other buffer alone.  Trees: the oracle on the oracle rows, and EVERY row within
    2e-9 max(1, |ref|max) of the composition (tests/test_coriolis_vjp.py:342-352: each side is within 1e-9 of the oracle; the scale is the
    oracle rows')"""
    def build():
        want = CSUBSETS[subset]
        names = [k for k, w in zip(("gq", "gqd"), want) if w]
        if tree:
            rob, _ = _mtree(name)
            n, h, fn = rob.n, rob._handle(), "rtbhip_tree_coriolis_vjp"
            q, qd, g = _mat_vjp_inputs("tree coriolis vjp", name, n)
            rows = _coriolis_oracle_rows(name)
            launch = _grid_only if lds is None else (lambda N: (_tiles(N), lds))
            ref = dict(zip(("gq", "gqd"), _coriolis_vjp_ref(name, True)))
            scale = {k: max(1.0, float(np.abs(ref[k][rows]).max())) for k in names}
            second = lambda: {k: v for k, v in zip(("gq", "gqd"), _tree_coriolis_composition(name)) if k in names}
            tol2 = lambda nm, w: 2e-9 * scale[nm]
        else:
            rob = _mat_dh_robot(name)
            n, h, fn = rob.n, rob._dyn_handle(), "rtbhip_coriolis_vjp"
            q, qd, g = _mat_vjp_inputs("coriolis vjp", name, n)
            rows, second, tol2 = None, None, None
            rt = n > 7          # csrc/coriolis_vjp_kernels.hip: kCoriolisVjpRegMax, coriolis_vjp_stride, `rt` and `lds` in launch_coriolis_vjp: q | qd | gC at an odd stride; beyond kCoriolisVjpRegMax one row of gC per pass
            launch = lambda N: (_tiles(N), 64 * 8 * ((2 * n + (n if rt else n * n)) | 1))
            ref = dict(zip(("gq", "gqd"), _coriolis_vjp_ref(name, False)))
        return Case(fn, {"q": In(q), "qd": In(qd), "gC": In(g)}, [O("gq", n), O("gqd", n)],
                    lambda N, p, s: (h, p("q"), p("qd"), N, p("gC")) + tuple(p(k) if w else None for k, w in zip(("gq", "gqd"), want)) + (MEM, s),
                    ref={k: ref[k] for k in names}, rows=rows, tol=VJP_TOL, launch=launch, keep=rob, second=second, tol2=tol2,
                    same_as=None if subset == "both" else _coriolis_vjp(name, "both", tree, lds))
    return build


# 6 and 7 = kCoriolisVjpRegMax: the register forms; 8: the first run-time-n size; 12: run-time-n with a longer pass loop.  (The limit size, 16, is
# 1.4e6 inverse-dynamics calls of the compiled reference on 129 rows -- half a minute; it runs in tests/test_coriolis_vjp.py.)
for _r in ("puma560", "panda", "n8m", "n12m"):
    for _s in CSUBSETS if _r in ("panda", "n8m") else ("both",):
        row("coriolis_vjp %s %s" % (_r, _s), "rtbhip_coriolis_vjp", MAT_DH_KN(_r), _coriolis_vjp(_r, _s, False))
for _r in ("UR5", "tree7", "tree8", "tree9"):
    for _s in CSUBSETS if _r in ("UR5", "tree9") else ("both",):
        row("tree_coriolis_vjp %s %s" % (_r, _s), "rtbhip_tree_coriolis_vjp", MAT_TREE_KN(_r), _coriolis_vjp(_r, _s, True))
# 8 groups whose register-form request does not fit a CU's LDS: the run-time-n form at n = 8, its request asserted (see _ladder8)
row("tree_coriolis_vjp ladder8 both", "rtbhip_tree_coriolis_vjp", JIT0, _coriolis_vjp("ladder8", "both", True, lds=_tree_coriolis_vjp_lds(8, 6, 7, True)))


# ------------------------------------------------------------------------------------------------ the entry points without a mem argument
# rtbhip_opspace, rtbhip_tree_opspace and rtbhip_ik_vjp take device pointers only: (..., void *stream), no mem.  Inputs at NMAX DISTINCT rows (the
# families' own cases repeat 16 or 24 rows cyclically).
def _ops_zoo(name):
    """(robot, tree?, gravity3, inertia, gravload, Jacobian of the robot's own path, bound factors (Mx, Gx, asada)) of a robot of tests/opspace_cases.py
    or of tests/opspace_census_cases.py: the oracle and the bound K eps cond(J)^2 max|ref| per row of the module that names it"""
    import opspace_cases as oc
    import opspace_census_cases as occ
    if name in occ.ALL:
        jac = None if occ.is_tree(name) else (lambda q: oracle.jacob0(occ._chain(name), q))
        return (occ.robot(name), occ.is_tree(name), occ.gravity3(name), lambda q: occ.inertia(name, q), lambda q: occ.gravload(name, q), jac, occ.K_OUT)
    return (oc.robot(name), oc.is_tree(name), oc.gravity3(name), lambda q: oc.inertia(name, q), lambda q: oc.gravload(name, q), lambda q: oc.jacob0(name, q), (oc.K,) * 3)


@functools.lru_cache(maxsize=None)
def _ops_ref(name):
    """(q, J, the oracle's rows): opspace_census_cases.draw_rows -- q ~ U(-3, 3), a draw replaced while cond(J) > 1e3, at most a third of them --
    and opspace_cases.formula on all NMAX rows, once per robot"""
    import opspace_census_cases as occ
    rb, tree, g3, inertia, gravload, jac, k = _ops_zoo(name)
    q, J, draws, replaced = occ.draw_rows("flush guard " + name, rb.n, NMAX, 8300 + sum(map(ord, name)), jac)
    return q, J, occ.reference_of(q, J, inertia(q), gravload(q))


def _opspace(name, want=("Mx", "Gx", "asada")):
    """tests/test_opspace.py:153-166, tests/test_opspace_census.py: oracle.inertia_dh / erobot_inertia, oracle.rne_dh / erobot_rne and
    numpy.linalg.inv / pinv / eig (opspace_cases.formula), per row K eps cond(J)^2 max|ref| (1 for the Asada ratio), mask 63.  The launch shape is
    the restatement of ops_layout / ops_tile_rows in tests/opspace_census_cases.py: a tile of 32 rows means ceil(N / 32) workgroups"""
    def build():
        import opspace_cases as oc
        import opspace_census_cases as occ
        rb, tree, g3, _, _, _, kout = _ops_zoo(name)
        q, J, ref = _ops_ref(name)
        n = rb.n
        fn, h = ("rtbhip_tree_opspace", rb._handle()) if tree else ("rtbhip_opspace", rb._dyn_handle())
        g3 = np.ascontiguousarray(g3, dtype=np.float64)
        w = occ.per_row(n, True, slots=occ.slots_of([r["parent"] for r in rb.group_table()])) if tree else occ.per_row(n, False, all(int(l.sigma) == 0 for l in rb.links))
        tile = occ.tile_rows(w)
        k = dict(zip(("Mx", "Gx", "asada"), kout))
        cond2 = oc.EPS * ref["cond"] ** 2

        def tol(nm, rows_ref, rows):
            scale = np.ones(len(rows)) if nm == "asada" else np.abs(rows_ref).max(axis=1)
            return (k[nm] * cond2[rows] * scale)[:, None]
        return Case(fn, {"q": In(q), "J": In(J)}, [O("Mx", 36), O("Gx", 6), O("asada", 1)],
                    lambda N, p, s: (h, p("q"), p("J"), N, _lib.host_ptr(g3), 63) + tuple(p(nm) if nm in want else None for nm in ("Mx", "Gx", "asada")) + (s,),
                    ref={nm: _flat({"Mx": ref["Mx"], "Gx": ref["Gx"], "asada": ref["all"]}[nm]) for nm in want}, tol=tol,
                    launch=lambda N: ((N + tile - 1) // tile, tile * w * 8), keep=(rb, g3),
                    same_as=None if len(want) == 3 else _opspace(name))
    return build


# puma560: the LU path; panda: the static right Gram path; n9s: the run-time-n tail; p16s (general DH, 16 joints, joint 8 prismatic): a tile of 32
# rows, ceil(N / 32) workgroups of 98560 bytes; UR5; lad16_4 (16 groups, four branch slots): a tile of 32 rows, 86272 bytes
OPS_KN = {"puma560": {}, "panda": {}, "n9s": JIT0, "p16s": JIT0, "UR5": {}, "lad16_4": JIT0}
for _r in OPS_KN:
    _fn = "rtbhip_tree_opspace" if _r in ("UR5", "lad16_4") else "rtbhip_opspace"
    row("%s %s" % (_fn[7:], _r), _fn, OPS_KN[_r], _opspace(_r))
    row("%s %s Mx alone" % (_fn[7:], _r), _fn, OPS_KN[_r], _opspace(_r, ("Mx",)))


@functools.lru_cache(maxsize=None)
def _ik_vjp_inputs(name):
    """tests/ik_vjp_cases.py:139-163 (inputs) at NMAX distinct rows: q ~ U(-3, 3), Tep = fkine(q) of the oracle, gq ~ U(-1, 1); a draw whose
    cond(J_a J_a^T) exceeds 1e4 for the full or the translation mask is replaced, at most one third of them.  success: zeros on some seam rows"""
    import ik_vjp_cases as kc
    m = kc.model(name)
    rng = _rng("ik_vjp", name)
    cand = rng.uniform(-3.0, 3.0, (2 * NMAX, m.n))
    Jc = m.jacob0(cand)
    ok = np.array([max(kc._cond(Jc[i], None), kc._cond(Jc[i], kc.TRANS)) <= kc.COND_MAX for i in range(len(cand))])
    keep = np.flatnonzero(ok)[:NMAX]
    assert len(keep) == NMAX and 3 * int((~ok[:keep[-1] + 1]).sum()) <= keep[-1] + 1, (name, "more than one third of the draws replaced")
    q, J = np.ascontiguousarray(cand[keep]), np.ascontiguousarray(Jc[keep])
    Tep, gq = np.ascontiguousarray(m.fkine(q)), rng.uniform(-1.0, 1.0, (NMAX, m.n))
    success = np.ones((NMAX, 1))
    success[[0, 7, 8, 33, 63, 64, 100, 127]] = 0.0
    assert {0, 7, 8, 63, 64, 127} <= set(SEAM_ROWS.tolist()) and success[128, 0] == 1.0
    tw, gT = kc.reference(J, Tep, gq, None, 0.0)
    tw[success[:, 0] == 0.0], gT[success[:, 0] == 0.0] = 0.0, 0.0          # a row that was not solved gets a zero gradient (tests/test_ik_vjp.py:424-436)
    return m, q, Tep, gq, success, tw, gT


def _ik_vjp(name, want=("gTep", "gtwist")):
    """tests/test_ik_vjp.py:303-313, tests/ik_vjp_cases.py: oracle.jacob0 and numpy.linalg.solve restating the definition, all six rows used, no
    damping; BOUND = 1e-9 of the row's largest reference magnitude.  we6 (NULL) is a host array and is not guarded"""
    def build():
        import ik_vjp_cases as kc
        m, q, Tep, gq, success, tw, gT = _ik_vjp_inputs(name)
        ets = m.ets
        ref = {"gTep": _flat(gT), "gtwist": _flat(tw)}
        return Case("rtbhip_ik_vjp", {"q": In(q), "Tep": In(Tep), "success": In(success, "int32"), "gq": In(gq)}, [O("gTep", 16), O("gtwist", 6)],
                    lambda N, p, s: (ets._handle(), p("q"), N, p("Tep"), p("success"), None, 0.0, p("gq")) + tuple(p(nm) if nm in want else None for nm in ("gTep", "gtwist")) + (s,),
                    ref={nm: ref[nm] for nm in want}, tol=lambda nm, w, rows: kc.BOUND * np.abs(w).max(axis=1)[:, None], launch=_grid_only, keep=(m, ets),
                    same_as=None if len(want) == 2 else _ik_vjp(name))
    return build


for _r in ("panda", "n11"):          # panda: k_ik_vjp<7>, the register form; n11: k_ik_vjp_any, the run-time-n form on a Jacobian in stream-ordered scratch
    for _w in (("gTep", "gtwist"), ("gTep",), ("gtwist",)):
        row("ik_vjp %s %s" % (_r, "both" if len(_w) == 2 else _w[0] + " alone"), "rtbhip_ik_vjp", {} if _r == "panda" else JIT0, _ik_vjp(_r, _w))


# ------------------------------------------------------------------------------------------------ the tests
# entry points whose flush already has guard rows (or poisoned buffers) around every output, every row against the oracle: entry point -> that test
ELSEWHERE = dict([(n, "test_kin_flush_guard_gpu.py::test_flush_writes_its_rows_and_leaves_the_guard_rows") for n in (
    "rtbhip_fkine", "rtbhip_jacob", "rtbhip_fkine_jacob", "rtbhip_fkine_jacob_packed", "rtbhip_fkine_jacob_f32", "rtbhip_fkine_jacob_packed_f32")] + [
    (n, "test_kin_flush_guard_gpu.py::test_fleet_launch_leaves_the_guard_rows") for n in ("rtbhip_fleet_fkine_jacob", "rtbhip_fleet_fkine_jacob_packed")] + [
    ("rtbhip_partial_fkine0", "test_partial_fkine0.py::test_gpu_writes_its_rows_and_nothing_else")])


NOT_COMPUTE = ("rtbhip_device_copy", "rtbhip_ik_restart")          # (..., mem / kind, stream) by shape, but no batch of rows is computed


MEMLESS = {"rtbhip_ik_vjp", "rtbhip_opspace", "rtbhip_tree_opspace"}          # compute entry points on device pointers only: (..., void *stream), no mem


def header_census(mem_only=False):
    """every compute entry point, from include/rtbhip.h itself: each `int rtbhip_*(` declaration whose parameter list ends in
    `int32_t mem, void *stream)`, and (unless mem_only) each one on a robot's handle that has an `int64_t N` and ends in `void *stream)` without a
    mem.  The ctypes
    table cannot opt an entry point out of this one by the type it gives the stream argument, nor the declaration by leaving out mem."""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    found = set()
    for name, params in re.findall(r"\bint\s+(rtbhip_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S):
        flat = " ".join(params.split())
        if re.search(r"\bint32_t\s+mem\s*,\s*void\s*\*\s*stream\s*$", flat):
            found.add(name)
        elif not mem_only and re.search(r"\bint64_t\s+N\b", flat) and re.search(r"\bvoid\s*\*\s*stream\s*$", flat) and re.match(r"rtbhip_(chain|dyn|tree)_t\b", flat):
            found.add(name)          # (a robot's handle first: rtbhip_shard_gather has an N and a stream too, and moves rows between ranks -- it computes none)
    return found - set(NOT_COMPUTE)


def census():
    """the rule by the types of rtbhip/_lib.py: (..., mem, stream) by shape as tests/test_api_refusals.py:924 builds the set, plus the vector-Jacobian
    products -- by the name, as include/rtbhip.h declares them; the stream types (_lib._sp and its subclasses _sq, _st, _sf; _si and _sc, which
    are none) claim rows for the families' own refusal censuses and decide nothing here"""
    S = _lib.SIGNATURES
    compute = {n for n, (_, a) in S.items() if len(a) >= 2 and a[-1] == _lib._vp and a[-2] == _lib._i32 and n not in NOT_COMPUTE}
    vjp = {n for n in header_census() if "_vjp" in n}
    return compute, vjp


def types_census():
    """what the census of this module found before it read the header: the shape rule, and the stream types _sp and its subclasses"""
    S = _lib.SIGNATURES
    compute = {n for n, (_, a) in S.items() if len(a) >= 2 and a[-1] == _lib._vp and a[-2] == _lib._i32 and n not in NOT_COMPUTE}
    return compute | {n for n, (_, a) in S.items() if a and (a[-1] is _lib._sp or (isinstance(a[-1], type) and issubclass(a[-1], _lib._sp)))}


def test_every_compute_entry_point_is_in_the_table_or_guard_checked_elsewhere():
    compute, vjp = census()
    assert len(compute) >= 35 and len(vjp) >= 11, (sorted(compute), sorted(vjp))
    tabled = {fn for _, fn, _, _ in ROWS}
    assert not tabled & set(ELSEWHERE)
    declared = header_census()
    assert declared == tabled | set(ELSEWHERE), sorted(declared ^ (tabled | set(ELSEWHERE)))
    assert declared >= types_census() and declared >= compute | vjp, sorted((types_census() | compute | vjp) - declared)
    assert declared <= set(_lib.SIGNATURES), sorted(declared - set(_lib.SIGNATURES))
    assert {"rtbhip_inertia_vjp", "rtbhip_tree_inertia_vjp", "rtbhip_coriolis_vjp", "rtbhip_tree_coriolis_vjp"} <= tabled
    # the wider rule adds exactly the three entry points without a mem argument, and each has rows
    with_mem = header_census(mem_only=True)
    assert declared - with_mem == MEMLESS and not MEMLESS & with_mem, sorted(declared - with_mem)
    assert MEMLESS <= tabled, "no table row for %s" % sorted(MEMLESS - tabled)
    for fn in MEMLESS:
        assert len({rid for rid, f, _, _ in ROWS if f == fn}) >= 4 and any("alone" in rid for rid, f, _, _ in ROWS if f == fn), fn
    here = os.path.dirname(os.path.abspath(__file__))
    for fn, where in ELSEWHERE.items():
        path, test = where.split("::")
        src = open(os.path.join(here, path)).read()
        assert "def %s(" % test in src and (fn[7:] in src), (fn, where)


def test_every_hessian_knob_is_exercised():
    seen = {}
    for rid, fn, knobs, _ in ROWS:
        if fn == "rtbhip_hessian":
            for k, v in knobs.items():
                seen.setdefault(k, set()).add(v)
    assert seen["hess_mode"] >= {0, 1, 2} and seen["reg"] >= {0} and seen["coalesced"] >= {0, 1} and seen["tiles_per_wave"] >= {2}
    assert set(KNOBS) >= set(seen)


@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_flush_guard_all(rid):
    try:
        _run(rid)
    except (_lib.RtbHipError, RuntimeError) as e:
        # a HIP error (RTBHIP_EHIP from the library, torch's own at the synchronize) is sticky: nothing more is launched on this device by this session.
        # A refusal of the arguments or a limit (RTBHIP_EINVAL, RTBHIP_ELIMIT) is an ordinary failure of this row.
        text = str(e)
        if "librtbhip error -2" in text or (not isinstance(e, _lib.RtbHipError) and ("HIP error" in text or "CUDA error" in text)):
            pytest.exit("flush_guard_all %s: device error, the session ends here: %r" % (rid, e), returncode=3)
        raise
