"""Differentiable ETS.ik_LM / ik_GN / ik_NR: rtbhip_ik_vjp and the Function of rtbhip/autograd.py.

The oracle and its bound are those of tests/ik_vjp_cases.py: oracle.jacob0 of the case's chain and numpy.linalg.solve restating
y_a = (J_a J_a^T + d^2 I)^-1 J_a gq, gTep = (y_v ; 1/2 [y_w]x R_p); bound 1e-9 of the row's largest reference magnitude.  Through autograd the rows
are the solver's own q, whose conditioning nobody filtered: there the bound of a row is 1e-9 max(1, cond(J_a J_a^T) / 1e4) -- the same
6 x 2.2e-16 x cond x 70 the cases' docstring reasons with.

No GPU is needed for the exports, the refusals of the raw ABI, the census against the header's comment, the front end's routing (a stand-in for a
CUDA tensor) and the solver's convergence on the autograd tests' inputs (the CPU replay of k_ik)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import replaying
import ik_vjp_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
BAD = 987654321
FN = "rtbhip_ik_vjp"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbol_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "rtbhip.h")).read()
    assert hasattr(_lib.lib(), FN) and FN in _lib.SIGNATURES and ("int %s(" % FN) in hdr
    res, args = _lib.SIGNATURES[FN]
    assert res is C.c_int and len(args) == 11 and args[0] is _lib._u64 and args[2] is _lib._i64 and args[6] is C.c_double
    assert args[-1] is _lib._vp                  # a plain void pointer: no mem argument in front of it, no stream type of its own


class _Ctx:
    def __init__(self):
        import link_frames_vjp_cases as fcases
        self._keep = (cases.model("panda").ets, rtbhip.ETS(rtbhip.ET.tx(0.2) * rtbhip.ET.Rx(0.3)), fcases.ets_of("cols"), cases.model("n4").ets)
        self.p, self.c0, self.cols, self.n4 = (e._handle() for e in self._keep)
        self._buf = np.zeros(8192)
        self.B = self._buf.ctypes.data
        self._we = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0])
        self.W5 = self._we.ctypes.data


_P = "ik_vjp: "
_WIDE = _P + "more used rows than joints: the solver's step is the least-squares one there, not differentiated here"
_DAMP = _P + "damping must be finite and >= 0"
# (handle, q, N, Tep, success, we6, damping, gq, gTep, gtwist, stream)
ROWS = [
    ("unknown", lambda x: (BAD, x.B, 4, x.B, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "unknown chain handle")),
    ("negN", lambda x: (x.p, x.B, -1, x.B, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "negative N")),
    ("nullq", lambda x: (x.p, None, 4, x.B, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullTep", lambda x: (x.p, x.B, 4, None, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgq", lambda x: (x.p, x.B, 4, x.B, None, None, 0.0, None, x.B, x.B, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullboth", lambda x: (x.p, x.B, 4, x.B, None, None, 0.0, x.B, None, None, None),
     (EINVAL, _P + "gTep and gtwist are both NULL: there is nothing to compute")),
    ("nojoints", lambda x: (x.c0, x.B, 4, x.B, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "chain has no joints")),
    ("jindex", lambda x: (x.cols, x.B, 4, x.B, None, None, 0.0, x.B, x.B, x.B, None),
     (EINVAL, _P + "chain must use jindex 0..n-1 (as rtbhip_ik_lm, whose q_out this reads)")),
    ("wide-null-mask", lambda x: (x.n4, x.B, 4, x.B, None, None, 0.1, x.B, x.B, x.B, None), (EINVAL, _WIDE)),
    ("wide-five-rows", lambda x: (x.n4, x.B, 4, x.B, None, x.W5, 0.1, x.B, x.B, x.B, None), (EINVAL, _WIDE)),
    ("damping-negative", lambda x: (x.p, x.B, 4, x.B, None, None, -0.1, x.B, x.B, x.B, None), (EINVAL, _DAMP)),
    ("damping-nan", lambda x: (x.p, x.B, 4, x.B, None, None, float("nan"), x.B, x.B, x.B, None), (EINVAL, _DAMP)),
    ("damping-inf", lambda x: (x.p, x.B, 4, x.B, None, None, float("inf"), x.B, x.B, x.B, None), (EINVAL, _DAMP)),
    ("too-many-tiles", lambda x: (x.p, x.B, 64 * 2 ** 31, x.B, None, None, 0.0, x.B, x.B, x.B, None), (ELIMIT, _P + "batch too large for one launch")),
    ("unknown+negN", lambda x: (BAD, x.B, -1, x.B, None, None, 0.0, x.B, x.B, x.B, None), (EINVAL, _P + "unknown chain handle")),
    ("negN+nullq", lambda x: (x.p, None, -1, None, None, None, 0.0, None, None, None, None), (EINVAL, _P + "negative N")),
    ("empty", lambda x: (x.p, x.B, 0, x.B, None, None, 0.0, x.B, x.B, x.B, None), (OK, None)),
    ("empty-null", lambda x: (x.p, None, 0, None, None, None, 0.0, None, None, None, None), (OK, None)),
    ("empty-success", lambda x: (x.p, x.B, 0, x.B, x.B, None, 0.0, x.B, x.B, x.B, None), (OK, None)),
]
# the refusals the header's comment names (parentheses dropped) -> the rows that hold them
HEADER = {
    "unknown chain handle": ["unknown"], "negative N": ["negN"], "a NULL input with N > 0": ["nullq", "nullTep", "nullgq"],
    "gTep and gtwist both NULL": ["nullboth"], "a chain without joints": ["nojoints"], "a chain whose jindex is not 0..n-1": ["jindex"],
    "more used rows than joints": ["wide-null-mask", "wide-five-rows"],
    "a negative or non-finite damping": ["damping-negative", "damping-nan", "damping-inf"],
    "a batch beyond one launch's tiles": ["too-many-tiles"],
}


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,make,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, make, want):
    ctx._buf[:] = 0.0
    rc = getattr(_lib.lib(), FN)(*make(ctx))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want
    assert not ctx._buf.any()                    # a refusal and the empty batch touch nothing


def test_every_refusal_the_header_names_has_a_row():
    hdr = open(os.path.join(ROOT, "include", "rtbhip.h")).read()
    end = hdr.index("int %s(" % FN)
    comment = " ".join(l.strip(" *") for l in hdr[hdr.rindex("/*", 0, end):end].splitlines())
    comment = re.sub(r"\([^)]*\)", "", comment)
    m = re.search(r"RTBHIP_EINVAL: (.*?)\.\s+RTBHIP_ELIMIT: (.*?)\.", comment)
    assert m, comment
    named = [re.sub(r"\s+", " ", x).strip() for part in m.groups() for x in part.split(",")]
    assert sorted(named) == sorted(HEADER), named
    ids = {r[0] for r in ROWS}
    assert len(ids) == len(ROWS) and all(set(v) <= ids for v in HEADER.values())
    refused = {r[0] for r in ROWS if r[2][0] != OK}
    assert refused - {"unknown+negN", "negN+nullq"} == {i for v in HEADER.values() for i in v}
    assert {r[2][0] for r in ROWS if r[0] in HEADER["a batch beyond one launch's tiles"]} == {ELIMIT}


# ------------------------------------------------------------------------------------------------ front-end routing (no GPU)
class _Ordinary(AssertionError):
    pass


def _fake_cuda(torch, shape, requires_grad, dtype=None):
    """what rtbhip takes for a CUDA tensor; the ordinary path stops at the first thing it asks of it"""
    class FakeCudaTensor:
        is_cuda = True

        def __init__(self):
            self.dtype, self.shape, self.requires_grad, self.device = dtype or torch.float64, tuple(shape), requires_grad, "cuda:0"

        def dim(self):
            return len(self.shape)

        def element_size(self):
            return 8

        def data_ptr(self):
            raise _Ordinary()

        def reshape(self, *a):
            raise _Ordinary()

        contiguous = detach = reshape

        def __getitem__(self, k):
            raise _Ordinary()

    FakeCudaTensor.__module__ = "torch"
    return FakeCudaTensor()


def test_routing_with_a_stand_in_tensor(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    seen = []

    def routed(ets, Tep, args, grad_damping):
        seen.append((ets.n, args[8], args[7], args[4], grad_damping))          # (n, flavour, method, mask, grad_damping)
        return (False, "q", "ok", "it", "se", "E")

    monkeypatch.setattr(rtbhip.autograd, "differentiable_ik", routed)
    panda, n4 = cases.model("panda").ets, cases.model("n4").ets
    t = lambda grad, **kw: _fake_cuda(torch, (5, 4, 4), grad, **kw)
    assert panda.ik_LM(t(True)) == ("q", "ok", "it", "se", "E")
    assert panda.ik_LM(t(True), method="sugihara", grad_damping=0.25)[0] == "q" and panda.ik_GN(t(True))[0] == "q" and panda.ik_NR(t(True), pinv_damping=0.5)[0] == "q"
    assert seen == [(7, 0, "chan", None, 0.0), (7, 0, "sugihara", None, 0.25), (7, 0, "gn", None, 0.0), (7, 0, "nr", None, 0.0)]
    del seen[:]
    # a mask of no more rows than joints routes on a short chain; the robot classes reach the same three methods
    assert n4.ik_LM(t(True), mask=[1, 1, 1, 0, 0, 1])[0] == "q" and n4.ik_GN(t(True), mask=[1, 0, 0, 0, 0, 0])[0] == "q"
    assert rtbhip.models.Panda().ik_LM(t(True), grad_damping=0.5)[0] == "q" and rtbhip.urdf.load("UR5").ik_NR(t(True), grad_damping=0.125)[0] == "q"
    assert cases.model("poe").robot.ik_GN(t(True))[0] == "q"
    assert [(s[0], s[4]) for s in seen] == [(4, 0.0), (4, 0.0), (7, 0.5), (6, 0.125), (6, 0.0)]
    del seen[:]
    # a plain Tep, disabled gradients, a wide mask on a 4-joint chain, ikine_LM and float32: the ordinary call, as before
    for call in (lambda: panda.ik_LM(t(False)), lambda: panda.ik_GN(t(False), grad_damping=0.5), lambda: panda.ik_NR(t(False)),
                 lambda: n4.ik_LM(t(True)), lambda: n4.ik_GN(t(True), mask=[1, 1, 1, 1, 1, 0]), lambda: n4.ik_NR(t(True), mask=[1, 2, 3, 4, 5, 6]),
                 lambda: panda.ikine_LM(t(True)), lambda: rtbhip.models.Panda().ikine_LM(t(True)),
                 lambda: panda.ik_LM(t(True, dtype=torch.float32)), lambda: panda.ik_NR(t(True, dtype=torch.float32))):
        with pytest.raises(_Ordinary):
            call()
    with torch.no_grad():
        for call in (lambda: panda.ik_LM(t(True)), lambda: panda.ik_GN(t(True)), lambda: panda.ik_NR(t(True))):
            with pytest.raises(_Ordinary):
                call()
    assert not seen
    # host arrays never come near it, with or without the new keyword
    assert not _lib.wants_grad(np.zeros((2, 4, 4)))
    with pytest.raises(TypeError):
        rtbhip.models.Panda().ik_LM(np.eye(4), grad_dampin=0.0)


# ------------------------------------------------------------------------------------------------ the autograd tests' inputs (no GPU)
# (Wampler's constant damping and Sugihara's E + k reach E < 1e-20 inside 30 iterations only when k is small: at the default k = 1 they crawl)
SOLVERS = [("ik_LM", dict(method="chan"), "chan", 1.0), ("ik_LM", dict(method="wampler", k=1e-8), "wampler", 1e-8),
           ("ik_LM", dict(method="sugihara", k=1e-8), "sugihara", 1e-8), ("ik_GN", {}, "gn", 0.0), ("ik_NR", {}, "nr", 0.0)]
SOLVER_IDS = ["LM-chan", "LM-wampler", "LM-sugihara", "GN", "NR"]
N_SOLVE = 65
TOL = 1e-20


def _solve_inputs(name):
    """(q_true (65, n) -- the cases' filter for conditioning --, Tep = fkine(q_true), q0 = q_true + 0.1 noise, W (65, n))"""
    m = cases.model(name)
    rng = np.random.default_rng(31 + sum(ord(c) for c in name))
    rows = []
    while len(rows) < N_SOLVE:
        cand = rng.uniform(-3.0, 3.0, (N_SOLVE, m.n))
        J = m.jacob0(cand)
        rows += [cand[i] for i in range(N_SOLVE) if max(cases._cond(J[i], None), cases._cond(J[i], cases.TRANS)) <= cases.COND_MAX]
    q = np.ascontiguousarray(rows[:N_SOLVE])
    return q, np.ascontiguousarray(m.fkine(q)), q + 0.1 * rng.normal(size=q.shape), rng.uniform(-1.0, 1.0, q.shape)


_CPU = {}


def _cpu_solve(name, k):
    """the replayed solver (tests/emu: k_ik's own lane functions on the CPU) on the inputs of the autograd tests -> (q, success)"""
    if (name, k) not in _CPU:
        import emu_harness
        _, _, method, kk = SOLVERS[k]
        q_true, Tep, q0, W = _solve_inputs(name)
        q, ok, it, se, E = emu_harness.ik(cases.model(name).ets, Tep, q0=q0, ilimit=30, slimit=100, tol=TOL, joint_limits=False, k=kk, method=method, flavour=0,
                                          seed=0)
        _CPU[(name, k)] = (q, ok)
    return _CPU[(name, k)]


@pytest.mark.parametrize("k", range(len(SOLVERS)), ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["panda", "UR5"])
def test_the_replayed_solver_converges_on_the_autograd_inputs(name, k):
    assert FN in _lib.SIGNATURES                 # (the inputs of test_backward_equals_the_oracle: nothing to prepare without the entry point)
    q, ok = _cpu_solve(name, k)
    print("ik_vjp autograd inputs %s/%s on the CPU: %d of %d rows solved at tol = %g" % (name, SOLVER_IDS[k], int(ok.sum()), N_SOLVE, TOL))
    assert 4 * int(ok.sum()) >= 3 * N_SOLVE


def _emit(y, Tep):
    """(N, 4, 4): the tangent-space gradient at Tep of the twist gradient y"""
    g = np.zeros((y.shape[0], 4, 4))
    for i in range(y.shape[0]):
        w = y[i, 3:]
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        g[i, :3, :3] = 0.5 * K @ Tep[i, :3, :3]
        g[i, :3, 3] = y[i, :3]
    return g


def _identity_discrepancy(name, q, ok, Tep, W16, got=None):
    """with T2 = fkine(q): the gradient of <W, T2> with respect to Tep through q = ik(Tep) against the tangent projection of W at Tep, the largest
    row-relative difference over the solved rows.  got None: the NumPy closed form at q (the reference for the bound); else the device's gradient"""
    m = cases.model(name)
    want = _emit(cases.pullback(Tep, W16), Tep)
    if got is None:
        J, T2 = m.jacob0(q), m.fkine(q)
        gq = np.einsum("irk,ir->ik", J, cases.pullback(T2, W16))
        got = cases.reference(J, Tep, gq, None, 0.0)[1]
    rows = np.flatnonzero(ok)
    return cases.row_error(got[rows], want[rows])


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the inverse-kinematics adjoint runs on the device only: not served by the CPU replay")(f))


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]          # (a copy: the cases are read-only)


def _mask(mask):
    return None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)


def _raw(ets, q, Tep, gq, mask, damping, success=None, want=(True, True)):
    """the entry point on device tensors (current stream) -> [gTep (N, 4, 4), gtwist (N, 6)], None for an output not asked for (handed over as NULL)"""
    torch = _torch()
    N = q.shape[0]
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device=q.device) if w else None for s, w in zip(((N, 4, 4), (N, 6)), want)]
    we = _mask(mask)
    _lib.check(getattr(_lib.lib(), FN)(ets._handle(), _ptr(q), N, _ptr(Tep), _ptr(success), _lib.host_ptr(we), float(damping), _ptr(gq), _ptr(outs[0]),
                                       _ptr(outs[1]), _stream(torch)))
    return outs


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


N_DEV = 130          # two full tiles and a partial one
SIZES = (1, 63, 64, 65, 130)


@gpu
@pytest.mark.parametrize("name,mask_name", cases.every_case())
def test_every_case_equals_the_oracle(name, mask_name):
    torch = _torch()
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mask_name)
    t = lambda a: cases.tiled(a, N_DEV)
    dq, dT, dg = _dev(torch, t(q), t(Tep), t(gq))
    got_T, got_tw = (x.cpu().numpy() for x in _raw(ets, dq, dT, dg, mask, damping))
    e_tw, e_T = cases.row_error(got_tw, t(tw)), cases.row_error(got_T, t(gT))
    print("ik_vjp device %s/%s (n = %d): gtwist %.3e, gTep %.3e of the row's |ref|max" % (name, mask_name, ets.n, e_tw, e_T))
    assert e_tw <= cases.BOUND and e_T <= cases.BOUND
    unused = [r for r in range(6) if r not in cases.used_rows(mask)]
    assert not got_tw[:, unused].any() and not got_T[:, 3, :].any()
    other = cases.same_answer(mask_name)
    if other:                                    # the positive weights drop out
        assert cases.row_error(got_tw, t(cases.case(name, other)[6])) <= cases.BOUND
        assert _bits(got_tw, _raw(ets, dq, dT, dg, cases.case(name, other)[4], damping)[1].cpu().numpy())


@gpu
@pytest.mark.parametrize("want", [(True, True), (True, False), (False, True)], ids=["both", "gTep", "gtwist"])
@pytest.mark.parametrize("name", ["n3", "panda", "n10", "n11", "n32"])
def test_guard_rows_and_inputs_unchanged(name, want):
    """every input and output between guard rows of one allocation (tests/flush_guard.py): the guards keep their bits, the inputs too, every live
    output row is written and equals the both-outputs call's bits"""
    torch = _torch()
    from flush_guard import Guarded
    mk = sorted(cases.masks_of(cases.model(name).n))[0]
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mk)
    n = ets.n
    for N in SIZES:
        t = lambda a: cases.tiled(a, N)
        ok = np.ones(N, dtype=np.int32)
        ins = [Guarded(torch, N, n, "float64").load(torch, t(q)), Guarded(torch, N, 16, "float64").load(torch, t(Tep).reshape(N, 16)),
               Guarded(torch, N, n, "float64").load(torch, t(gq)), Guarded(torch, N, 1, "int32").load(torch, ok.reshape(N, 1))]
        before = [g.bits.clone() for g in ins]
        outs = [Guarded(torch, N, 16, "float64"), Guarded(torch, N, 6, "float64")]
        _lib.check(getattr(_lib.lib(), FN)(ets._handle(), ins[0].ptr, N, ins[1].ptr, ins[3].ptr, _lib.host_ptr(_mask(mask)), float(damping), ins[2].ptr,
                                           outs[0].ptr if want[0] else None, outs[1].ptr if want[1] else None, _stream(torch)))
        torch.cuda.synchronize()
        assert all(torch.equal(g.bits, b) for g, b in zip(ins, before)), (name, N)
        ref = _raw(ets, *_dev(torch, t(q), t(Tep), t(gq)), mask, damping)
        for o, w, r in zip(outs, want, ref):
            assert o.guards_intact(), (name, N)
            if w:
                assert not bool((o.live_bits() == o.pattern).any()) and torch.equal(o.live(), r.reshape(N, -1)), (name, N)
            else:
                assert bool((o.live_bits() == o.pattern).all()), (name, N)


@gpu
@pytest.mark.parametrize("name", ["n2", "n5", "panda", "UR5", "n10", "n16"])
def test_rows_are_independent_bit_for_bit(name):
    torch = _torch()
    m = cases.model(name)
    masks = cases.masks_of(m.n)
    mask, damping = masks[sorted(masks)[0]]
    q, Tep, gq = cases.distinct(name, N_DEV)
    dq, dT, dg = _dev(torch, q, Tep, gq)
    a_T, a_tw = (x.cpu().numpy() for x in _raw(m.ets, dq, dT, dg, mask, damping))
    perm = np.random.default_rng(3).permutation(N_DEV)
    p_T, p_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q[perm], Tep[perm], gq[perm]), mask, damping))
    assert _bits(p_T, a_T[perm]) and _bits(p_tw, a_tw[perm])
    for k in (0, 63, 64, 129):                   # row k of the batch against the same row alone
        s_T, s_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q[k:k + 1], Tep[k:k + 1], gq[k:k + 1]), mask, damping))
        assert _bits(s_T[0], a_T[k]) and _bits(s_tw[0], a_tw[k]), (name, k)


def _ur5_with_a_singular_row():
    """UR5 rows of the cases with row 70 at q = 0: the arm stretched out, shoulder, elbow and wrist axes parallel -- J J^T singular"""
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case("UR5", "ones")
    m = cases.model("UR5")
    q = np.array(cases.tiled(q, N_DEV))
    q[70] = 0.0
    Tep = np.ascontiguousarray(m.fkine(q))
    J = m.jacob0(q)
    assert np.linalg.cond(J[70] @ J[70].T) > 1e12
    return m, q, Tep, cases.tiled(gq, N_DEV), J


@gpu
def test_a_nonfinite_q_and_a_singular_row_stay_in_their_row():
    torch = _torch()
    m, q, Tep, gq, J = _ur5_with_a_singular_row()
    tw, gT = cases.reference(np.delete(J, 70, axis=0), np.delete(Tep, 70, axis=0), np.delete(gq, 70, axis=0), None, 0.0)
    base_T, base_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q, Tep, gq), None, 0.0))
    others = np.delete(np.arange(N_DEV), 70)
    assert np.isfinite(base_tw[others]).all() and cases.row_error(base_tw[others], tw) <= cases.BOUND and cases.row_error(base_T[others], gT) <= cases.BOUND
    # a benign row in the singular row's place: every other row keeps its bits
    q2 = np.array(q)
    q2[70] = q2[71]
    T2 = np.array(Tep)
    T2[70] = T2[71]
    b_T, b_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q2, T2, gq), None, 0.0))
    assert _bits(b_T[others], base_T[others]) and _bits(b_tw[others], base_tw[others])
    # a NaN and an infinity among the joint values: their rows are not finite, every other row still meets the oracle (the wave of such a row takes
    # the library's sine and cosine: other bits, the same bound)
    for bad in (float("nan"), float("inf")):
        q3 = np.array(q)
        q3[3, 2] = bad
        n_T, n_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q3, Tep, gq), None, 0.0))
        assert not np.isfinite(n_tw[3]).any() and not np.isfinite(n_T[3, :3, :]).all()
        keep = np.delete(np.arange(N_DEV), [3, 70])
        ref_rows = np.delete(np.arange(N_DEV - 1), [3])          # (tw / gT have no row 70)
        assert np.isfinite(n_tw[keep]).all() and cases.row_error(n_tw[keep], tw[ref_rows]) <= cases.BOUND
        assert cases.row_error(n_T[keep], gT[ref_rows]) <= cases.BOUND


@gpu
def test_the_singular_row_with_damping_meets_the_oracle():
    torch = _torch()
    m, q, Tep, gq, J = _ur5_with_a_singular_row()
    tw, gT = cases.reference(J, Tep, gq, None, 0.1)
    got_T, got_tw = (x.cpu().numpy() for x in _raw(m.ets, *_dev(torch, q, Tep, gq), None, 0.1))
    e_tw, e_T = cases.row_error(got_tw, tw), cases.row_error(got_T, gT)
    print("ik_vjp device UR5 with a singular row, damping 0.1: gtwist %.3e, gTep %.3e; the singular row alone %.3e" % (e_tw, e_T, cases.row_error(got_tw[70:71], tw[70:71])))
    assert e_tw <= cases.BOUND and e_T <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["n2", "panda", "n11"])
def test_success_is_honoured(name):
    torch = _torch()
    mk = sorted(cases.masks_of(cases.model(name).n))[0]
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case(name, mk)
    t = lambda a: cases.tiled(a, N_DEV)
    ok = (np.arange(N_DEV) % 2).astype(np.int32)
    dq, dT, dg, dok = _dev(torch, t(q), t(Tep), t(gq), ok)
    all_T, all_tw = (x.cpu().numpy() for x in _raw(ets, dq, dT, dg, mask, damping))
    got_T, got_tw = (x.cpu().numpy() for x in _raw(ets, dq, dT, dg, mask, damping, success=dok))
    assert not got_T[ok == 0].any() and not got_tw[ok == 0].any()
    assert _bits(got_T[ok == 1], all_T[ok == 1]) and _bits(got_tw[ok == 1], all_tw[ok == 1])
    one_T, one_tw = (x.cpu().numpy() for x in _raw(ets, dq, dT, dg, mask, damping, success=torch.ones_like(dok)))
    assert _bits(one_T, all_T) and _bits(one_tw, all_tw)          # NULL success: every row counts as a solution


@gpu
def test_one_captured_graph_replayed_twice():
    """the launch a backward pass makes, under torch.cuda.graph: a single launch on the caller's stream, captured after one eager warm-up (the
    table's upload), replayed to the eager result and again on new inputs"""
    torch = _torch()
    ets, q, Tep, gq, mask, damping, tw, gT = cases.case("panda", "ones")
    t = lambda a: cases.tiled(a, N_DEV)
    dq, dT, dg = _dev(torch, t(q), t(Tep), t(gq))
    eager0 = [x.clone() for x in _raw(ets, dq, dT, dg, mask, damping)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _raw(ets, dq, dT, dg, mask, damping)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager0[0]) and torch.equal(outs[1], eager0[1])
    dq.copy_(dq.flip(0))
    dT.copy_(dT.flip(0))
    dg.copy_(dg * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager1 = _raw(ets, dq, dT, dg, mask, damping)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager1[0]) and torch.equal(outs[1], eager1[1]) and not torch.equal(outs[1], eager0[1])


# ------------------------------------------------------------------------------------------------ through autograd
def _solve(torch, name, k, Tep, q0, **kw):
    fn, extra, _, _ = SOLVERS[k]
    return getattr(cases.model(name).ets, fn)(Tep, q0=q0, joint_limits=False, tol=TOL, **extra, **kw)


@gpu
@pytest.mark.parametrize("k", range(len(SOLVERS)), ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["panda", "UR5"])
def test_backward_equals_the_oracle(name, k):
    torch = _torch()
    m = cases.model(name)
    assert 4 * int(_cpu_solve(name, k)[1].sum()) >= 3 * N_SOLVE          # first on the CPU: the inputs are solvable
    q_true, Tep, q0, W = _solve_inputs(name)
    dT, dq0, dW = _dev(torch, Tep, q0, W)
    dT.requires_grad_(True)
    q, ok, it, se, E = _solve(torch, name, k, dT, dq0)
    assert q.grad_fn is not None and tuple(q.shape) == (N_SOLVE, m.n)
    (q * dW).sum().backward()
    okh, qh, got = ok.cpu().numpy(), q.detach().cpu().numpy(), dT.grad.cpu().numpy()
    assert 4 * int(okh.sum()) >= 3 * N_SOLVE, int(okh.sum())
    assert got.shape == (N_SOLVE, 4, 4) and not got[okh == 0].any()
    rows = np.flatnonzero(okh)
    J = m.jacob0(qh[rows])
    ref = cases.reference(J, Tep[rows], W[rows], None, 0.0)[1]
    cond = np.array([np.linalg.cond(j @ j.T) for j in J])
    scale = np.abs(ref).reshape(len(rows), -1).max(axis=1)
    err = np.abs(got[rows] - ref).reshape(len(rows), -1).max(axis=1) / scale
    bound = cases.BOUND * np.maximum(1.0, cond / cases.COND_MAX)
    print("ik_vjp autograd %s/%s: %d of %d solved, largest error %.3e of the row's |ref|max (cond up to %.3g)" % (name, SOLVER_IDS[k], len(rows), N_SOLVE, err.max(), cond.max()))
    assert (err <= bound).all(), (err / bound).max()


@gpu
@pytest.mark.parametrize("name", ["panda", "UR5"])
def test_identity_through_two_functions(name):
    """q = ik_LM(Tep), T2 = fkine(q): the gradient of <W, T2> with respect to Tep is the tangent projection of W at Tep on the solved rows -- to the
    order of the residual the solver stopped at.  Bound: 100 times the same discrepancy from the replayed solver's q and the NumPy closed form,
    at least 1e-9."""
    torch = _torch()
    m = cases.model(name)
    q_true, Tep, q0, _ = _solve_inputs(name)
    W16 = np.random.default_rng(77).uniform(-1.0, 1.0, (N_SOLVE, 4, 4))
    q_cpu, ok_cpu = _cpu_solve(name, 0)
    d_cpu = _identity_discrepancy(name, q_cpu, ok_cpu, Tep, W16)
    dT, dq0, dW = _dev(torch, Tep, q0, W16)
    dT.requires_grad_(True)
    q, ok = _solve(torch, name, 0, dT, dq0)[:2]
    T2 = m.ets.eval(q)
    (T2 * dW).sum().backward()
    d_gpu = _identity_discrepancy(name, None, ok.cpu().numpy(), Tep, W16, got=dT.grad.cpu().numpy())
    print("ik_vjp identity %s: device %.3e, CPU reference %.3e (bound %.3e)" % (name, d_gpu, d_cpu, max(1e-9, 100.0 * d_cpu)))
    assert 4 * int(ok.sum()) >= 3 * N_SOLVE
    assert d_gpu <= max(1e-9, 100.0 * d_cpu)


@gpu
def test_launch_count_and_arguments(monkeypatch):
    torch = _torch()
    m = cases.model("panda")
    q_true, Tep, q0, W = _solve_inputs("panda")
    dT, dq0, dW = _dev(torch, Tep, q0, W)
    dT.requires_grad_(True)
    dq0.requires_grad_(True)
    q, ok, it, se, E = m.ets.ik_LM(dT, q0=dq0, joint_limits=False, tol=TOL)
    assert q.grad_fn is not None and all(x.grad_fn is None and not x.requires_grad for x in (ok, it, se, E))
    real, calls = getattr(_lib.lib(), FN), []
    monkeypatch.setattr(_lib.lib(), FN, lambda *a: calls.append(a) or real(*a))
    (q * dW).sum().backward()
    assert len(calls) == 1 and calls[0][2] == N_SOLVE and calls[0][9] is None and calls[0][8] is not None          # gTep asked for, gtwist not
    assert dq0.grad is None and dT.grad is not None and tuple(dT.grad.shape) == (N_SOLVE, 4, 4)
    batch = dT.grad.clone()
    # one (4, 4) target: the reference's 5-tuple, q attached to the graph, the gradient shaped like Tep
    one = dT.detach()[5].clone().requires_grad_(True)
    q1, ok1, it1, se1, E1 = m.ets.ik_LM(one, q0=dq0.detach()[5], joint_limits=False, tol=TOL)
    assert tuple(q1.shape) == (7,) and q1.grad_fn is not None and isinstance(ok1, int) and isinstance(it1, int) and isinstance(E1, float)
    (q1 * dW[5]).sum().backward()
    assert len(calls) == 2 and tuple(one.grad.shape) == (4, 4)
    assert ok1 == int(ok[5]) and torch.equal(one.grad, batch[5])
    # grad_damping reaches the launch; without a gradient it is ignored
    dT2 = dT.detach().clone().requires_grad_(True)
    m.ets.ik_LM(dT2, q0=dq0.detach(), joint_limits=False, tol=TOL, grad_damping=0.25)[0].sum().backward()
    assert len(calls) == 3 and calls[2][6] == 0.25
    with torch.no_grad():
        assert m.ets.ik_LM(dT2, q0=dq0.detach(), joint_limits=False, tol=TOL, grad_damping=0.25)[0].grad_fn is None


def _readme_line():
    text = open(os.path.join(ROOT, "README.md")).read()
    lines = [l for l in text.splitlines() if "ik_LM(Tep" in l and "backward()" in l]
    assert len(lines) == 1, lines
    return lines[0]


def test_readme_example_line_is_python():
    compile(_readme_line(), "README.md", "exec")
    assert "grad_damping" in open(os.path.join(ROOT, "README.md")).read()


@gpu
def test_readme_example_line_runs():
    torch = _torch()
    ns = {"torch": torch, "rtbhip": rtbhip, "panda": rtbhip.models.Panda(),
          "q": torch.rand(256, 7, device="cuda", dtype=torch.float64, requires_grad=True)}
    exec(compile(_readme_line(), "README.md", "exec"), ns)          # noqa: S102 -- our own README
    g = ns["Tep"].grad
    assert tuple(g.shape) == (256, 4, 4) and bool(torch.isfinite(g).all()) and bool((g != 0).any()) and not bool((g[:, 3, :] != 0).any())
