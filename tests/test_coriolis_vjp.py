"""Differentiable DHRobot.coriolis / ERobot.coriolis: rtbhip_coriolis_vjp, rtbhip_tree_coriolis_vjp and the two Functions of rtbhip/autograd.py.

The oracle and its bound are those of tests/coriolis_vjp_cases.py: for gq five-point Richardson differences (h = 1e-3) of the reference's Coriolis
matrix (oracle.coriolis_dh, oracle.erobot.erobot_coriolis), one q column at a time; for gqd the exact linearity of C in qd; both contracted with gC;
bound 1e-9 max(1, |ref|max) over the compared array.  The fused call against the composition it replaces -- 2 n launches of rtbhip_rne_vjp /
rtbhip_tree_rne_vjp at qd +- e_k, gtau = +-1/4 gC[:, :, k], summed (the polar identity C[:, k] = 1/4 (tau(qd + e_k) - tau(qd - e_k))) -- at
2e-9 max(1, |ref|max): each side is held to 1e-9 of the same oracle.  gradcheck: torch's default tolerances.

No GPU is needed for the exports, the refusals of the raw ABI, the census, the front end's routing (a stand-in for a CUDA tensor) and the oracle's
own error."""
import ctypes as C
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib, Link, ET, ERobot
from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH
from helpers import replaying
import coriolis_vjp_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
HOST, DEV = 0, 1
BAD = 987654321
DH_VJP, TREE_VJP = "rtbhip_coriolis_vjp", "rtbhip_tree_coriolis_vjp"
VJP = (DH_VJP, TREE_VJP)
_HAND = "the robot is not numbered in group order (joint j of the q row must be moved by link group j)"


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbols_are_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    for name in VJP:
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES and ("int %s(" % name) in hdr


def _prismatic():
    return DHRobot([RevoluteDH(a=0.3, m=1.0), PrismaticDH(alpha=0.5, m=1.0)])


def _long_tree(n):
    """a serial chain of n revolute joints"""
    links, parent = [], None
    for i in range(n):
        parent = Link(ET.tx(0.1) * ET.Rz(), m=1.0, r=[0.05, 0.0, 0.0], parent=parent, name="l%d" % i)
        links.append(parent)
    return ERobot(links, name="long%d" % n)


class _Ctx:
    def __init__(self):
        self._keep = (rtbhip.models.DH.Puma560(), _prismatic(), cases.dh_cases.random_robot(17, 0, 5), cases.tree_robot("tree5")[0],
                      cases.tree_robot(cases.HAND)[0], _long_tree(21))
        self.d, self.p, self.d17 = (r._dyn_handle() for r in self._keep[:3])
        self.t, self.h, self.t21 = (r._handle() for r in self._keep[3:])
        self._buf = np.zeros(8192)
        self.B = self._buf.ctypes.data


# (handle, q, qd, N, gC, gq, gqd, mem, stream)
ROWS = []
for _name, _kind, _ok, _spec in (("coriolis_vjp", "dyn", "d", (("prismatic", "p", EINVAL, "chain has a prismatic joint"), ("17joints", "d17", ELIMIT, "chains of 1..16 joints"))),
                                 ("tree_coriolis_vjp", "tree", "t", (("handnumbered", "h", EINVAL, _HAND), ("21joints", "t21", ELIMIT, "robots of 1..20 joints")))):
    _add = lambda tag, g, want, _name=_name: ROWS.append((_name + "-" + tag, "rtbhip_" + _name, g, want))
    _p = _name + ": "
    _add("unknown", lambda x: (BAD, x.B, x.B, 4, x.B, x.B, x.B, HOST, None), (EINVAL, _p + "unknown %s handle" % _kind))
    _add("nullq", lambda x, k=_ok: (getattr(x, k), None, x.B, 4, x.B, x.B, x.B, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullqd", lambda x, k=_ok: (getattr(x, k), x.B, None, 4, x.B, x.B, x.B, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgC", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 4, None, x.B, x.B, HOST, None), (EINVAL, _p + "NULL gC"))
    _add("nullboth", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 4, x.B, None, None, HOST, None), (EINVAL, _p + "NULL gq and NULL gqd"))
    _add("negN", lambda x, k=_ok: (getattr(x, k), x.B, x.B, -1, x.B, x.B, x.B, HOST, None), (EINVAL, _p + "negative N"))
    _add("mem7", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 4, x.B, x.B, x.B, 7, None), (EINVAL, _p + "bad mem kind"))
    _add("unknown+negN", lambda x: (BAD, x.B, x.B, -1, x.B, x.B, x.B, HOST, None), (EINVAL, _p + "unknown %s handle" % _kind))
    _add("nullq+nullgC", lambda x, k=_ok: (getattr(x, k), None, None, 4, None, None, None, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgC+nullboth", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 4, None, None, None, HOST, None), (EINVAL, _p + "NULL gC"))
    _add("negN+mem7", lambda x, k=_ok: (getattr(x, k), x.B, x.B, -1, x.B, x.B, x.B, 7, None), (EINVAL, _p + "negative N"))
    for _tag, _k, _rc, _why in _spec:
        for _mem in (HOST, DEV):          # refused before any memory is looked at
            _add(_tag + ("-dev" if _mem == DEV else ""), lambda x, k=_k, m=_mem: (getattr(x, k), x.B, x.B, 4, x.B, x.B, x.B, m, None), (_rc, _p + _why))
        _add("empty-" + _tag, lambda x, k=_k: (getattr(x, k), None, None, 0, None, None, None, HOST, None), (OK, None))
    _add("empty", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 0, x.B, x.B, x.B, HOST, None), (OK, None))
    _add("empty-dev", lambda x, k=_ok: (getattr(x, k), x.B, x.B, 0, x.B, x.B, x.B, DEV, None), (OK, None))
    _add("empty-null", lambda x, k=_ok: (getattr(x, k), None, None, 0, None, None, None, HOST, None), (OK, None))


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,fn,make,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, fn, make, want):
    ctx._buf[:] = 0.0
    rc = getattr(_lib.lib(), fn)(*make(ctx))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want
    assert not ctx._buf.any()                    # a refusal and the empty batch touch nothing


def test_the_rows_name_both_entry_points():
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for these two (rtbhip/_lib.py: _sc)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._sc}
    assert mine == set(VJP)
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert mine <= {fn for _, fn, _, want in ROWS if want[0] == OK} and mine <= {fn for _, fn, _, want in ROWS if want[0] != OK}
    assert len({r[0] for r in ROWS}) == len(ROWS)
    # a type of its own that the censuses of the other families do not see: no subclass of theirs, not the plain void pointer
    assert not issubclass(_lib._sc, _lib._sp) and not issubclass(_lib._sc, _lib._si) and _lib._sc is not _lib._si and _lib._sc != _lib._vp
    assert _lib._sc.__bases__ == (C.c_void_p,)
    assert _lib._sc.from_param(None) is None and isinstance(_lib._sc.from_param(C.c_void_p(8)), C.c_void_p)


# ------------------------------------------------------------------------------------------------ the oracle's own error (no GPU)
@pytest.mark.parametrize("name", ["puma560", "panda", "UR5"])
def test_the_oracle_is_a_hundred_times_finer_than_the_bound(name):
    """the stencil at h against h / 2, and the exact gqd against its own stencil: <= 1e-11 max(1, |ref|max), a hundredth of the bound; panda and
    UR5 also with one joint at 2^21 + 0.25 rad, h = 2^-10 against h / 2"""
    if name == "UR5":
        rob, orc, q, qd, g, a, d = cases.tree_case(name)
        Cf = cases.tree_coriolis(orc)
        b = cases.tree_oracle(orc, q, qd, g, h=cases.H / 2)[0]
    else:
        rb, q, qd, g, a, d = cases.dh_case(name)
        Cf = cases.dh_coriolis(rb)
        b = cases.dh_oracle(rb, q, qd, g, h=cases.H / 2)[0]
    err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(a).max()))
    errd = float(np.abs(d - cases.gqd_stencil(Cf, q, qd, g)).max()) / max(1.0, float(np.abs(d).max()))
    print("coriolis oracle %s: gq h against h/2 %.3e (|ref|max %.3g); exact gqd against its stencil %.3e" % (name, err, np.abs(a).max(), errd))
    assert err <= 1e-11 and errd <= 1e-11
    if name in ("panda", "UR5"):
        # one joint at 2^21 + 0.25 rad, the stencil at h = 2^-10 against h / 2: the reference can supply the number that
        # test_nonfinite_and_huge_joint_values_stay_in_their_row compares that row with
        q, qd, g = (np.array(x) for x in cases.draw(q.shape[1], 2, 5))
        q[:, 2] = BIG_ANGLE
        a, b = _oracle(name, q, qd, g, BIG_H)[0], _oracle(name, q, qd, g, BIG_H / 2)[0]
        err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(a).max()))
        print("coriolis oracle %s at a huge angle: gq h = 2^-10 against h/2 %.3e (|ref|max %.3g)" % (name, err, np.abs(a).max()))
        assert err <= 1e-11


BIG_ANGLE = 2.0 ** 21 + 0.25          # beyond 2^20: the wave of such a lane takes the library's sine and cosine (csrc/coriolis_vjp_kernels.hip: rne_trig in coriolis_vjp_lane; tree_trig)
BIG_H = 2.0 ** -10                    # q +- h and q +- 2 h are exact doubles at that magnitude (one ulp is 2^-31); at h = 1e-3 they are not, six digits lost


def _oracle(name, q, qd, g, h):
    if name in cases.DH_ROBOTS:
        return cases.dh_oracle(cases.dh_robot(name), q, qd, g, h=h)
    return cases.tree_oracle(cases.tree_robot(name)[1], q, qd, g, h=h)


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
    monkeypatch.setattr(rtbhip.autograd, "differentiable_coriolis", lambda robot, q, qd: seen.append(("dh", robot.n)) or "routed")
    monkeypatch.setattr(rtbhip.autograd, "differentiable_tree_coriolis", lambda robot, q, qd: seen.append(("tree", robot.n)) or "routed")
    puma = rtbhip.models.DH.Puma560()
    t = lambda grad, **kw: _fake_cuda(torch, (5, 6), grad, **kw)
    # either input asking for a gradient routes; a single configuration too
    assert puma.coriolis(t(True), t(False)) == "routed" and puma.coriolis(t(False), t(True)) == "routed" and puma.coriolis(t(True), t(True)) == "routed"
    assert puma.coriolis(_fake_cuda(torch, (6,), True), _fake_cuda(torch, (6,), False)) == "routed" and seen == [("dh", 6)] * 4
    del seen[:]
    rob = cases.tree_robot("tree5")[0]
    u = lambda grad: _fake_cuda(torch, (5, rob.n), grad)
    ur = rtbhip.urdf.load("UR5")
    yumi = rtbhip.urdf.load("YuMi")
    ex = tuple(e for e in cases.tree_cases.URDFS["YuMi"] if e in yumi.linkdict)
    ny = yumi.erobot(ex).n
    y = lambda grad: _fake_cuda(torch, (2, ny), grad)
    assert rob.coriolis(u(True), u(False)) == "routed" and rob.coriolis(u(False), u(True)) == "routed" and ur.coriolis(t(True), t(True)) == "routed"
    assert yumi.coriolis(y(False), y(True), exclude=ex) == "routed"
    assert seen == [("tree", rob.n), ("tree", rob.n), ("tree", 6), ("tree", ny)]
    del seen[:]
    # neither input asks, disabled gradients, float32 rows, a prismatic DH chain and a hand-numbered tree: the ordinary path, as before
    for robot, mk in ((puma, t), (rob, u)):
        with pytest.raises(_Ordinary):
            robot.coriolis(mk(False), mk(False))
        with torch.no_grad(), pytest.raises(_Ordinary):
            robot.coriolis(mk(True), mk(True))
    for robot in (puma, ur):
        with pytest.raises(TypeError, match="float64"):
            robot.coriolis(t(True, dtype=torch.float32), t(True, dtype=torch.float32))
    with pytest.raises(_Ordinary):
        _prismatic().coriolis(_fake_cuda(torch, (5, 2), True), _fake_cuda(torch, (5, 2), True))
    hand = cases.tree_robot(cases.HAND)[0]
    assert not hand._in_group_order() and rob._in_group_order()
    with pytest.raises(_Ordinary):
        hand.coriolis(_fake_cuda(torch, (5, 4), True), _fake_cuda(torch, (5, 4), True))
    assert not seen
    # host arrays never come near it
    assert not _lib.wants_grad(np.zeros((2, 6)))
    assert puma.coriolis(np.zeros((0, 6)), np.zeros((0, 6))).shape == (0, 6, 6)          # (an empty batch returns before any device is looked for)
    e = np.zeros((0, rob.n))
    assert rob.coriolis(e, e).shape == (0, rob.n, rob.n) and not seen


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the coriolis adjoint runs on the device only: not served by the CPU replay")(f))


def _ptr(x):
    return None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data_as(C.c_void_p))


def _is_tree(rb):
    return not isinstance(rb, DHRobot)


def _handle(rb):
    if not _is_tree(rb):
        return rb._dyn_handle()
    return (rb._tree(()) if callable(getattr(rb, "_tree", None)) else rb)._handle()          # (a URDFRobot serves its dynamics through the ERobot of its link tree)


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vjp(rb, q, qd, g, which=(True, True)):
    """the fused entry point on device tensors (current stream) or host arrays -> [gq, gqd], None for an output not asked for (handed over as NULL)"""
    fn = getattr(_lib.lib(), TREE_VJP if _is_tree(rb) else DH_VJP)
    if isinstance(q, np.ndarray):
        outs = [np.full(q.shape, np.nan) if w else None for w in which]
        _lib.check(fn(_handle(rb), _ptr(q), _ptr(qd), q.shape[0], _ptr(g), _ptr(outs[0]), _ptr(outs[1]), HOST, None))
        return outs
    torch = _torch()
    outs = [torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device) if w else None for w in which]
    _lib.check(fn(_handle(rb), _ptr(q), _ptr(qd), q.shape[0], _ptr(g), _ptr(outs[0]), _ptr(outs[1]), DEV, _stream(torch)))
    return outs


def _composition(rb, q, qd, g):
    """what the fused call replaces: 2 n launches of the inverse-dynamics adjoint at qd +- e_k, gtau = +-1/4 gC[:, :, k], no gravity, no qdd, summed
    -> [gq, gqd].  (Puma560's and Panda's viscous friction enters gqd as +-1/4 G^2 B gC and cancels in the sum; Coulomb friction has derivative zero.)"""
    torch = _torch()
    zero = np.zeros(3)
    tq, td = torch.zeros_like(q), torch.zeros_like(q)
    for k in range(rb.n):
        for sign in (1.0, -1.0):
            v = qd.clone()
            v[:, k] += sign
            gk = (0.25 * sign) * g[:, :, k].contiguous()
            gq, gqd = torch.empty_like(q), torch.empty_like(q)
            if _is_tree(rb):
                _lib.check(_lib.lib().rtbhip_tree_rne_vjp(_handle(rb), _ptr(q), _ptr(v), None, q.shape[0], _lib.host_ptr(zero), _ptr(gk), _ptr(gq), _ptr(gqd),
                                                          None, DEV, _stream(torch)))
            else:
                _lib.check(_lib.lib().rtbhip_rne_vjp(rb._dyn_handle(), _ptr(q), _ptr(v), None, q.shape[0], _lib.host_ptr(zero), None, _ptr(gk), _ptr(gq),
                                                     _ptr(gqd), None, DEV, _stream(torch)))
            tq, td = tq + gq, td + gqd
    return [tq, td]


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]          # (a copy: the cases are read-only)


def _distinct(name, N):
    """(robot, q, qd, gC) of N DISTINCT rows from the cases' input distribution, no oracle: for comparisons of bits and of one device result with
    another.  (cases.case repeats 8 or 2 rows, and there a row that lands a multiple of the period away still meets its expected bits.)"""
    rb = cases.dh_robot(name) if name in cases.DH_ROBOTS else cases.tree_robot(name)[0]
    return (rb,) + tuple(np.array(x) for x in cases.draw(rb.n, N, cases._seed(name) + 1))


def _scales(name):
    """max(1, |ref|max) of gq and gqd from the cached oracle rows of the same robot and the same input distribution"""
    ref = cases.dh_case(name)[4:] if name in cases.DH_ROBOTS else cases.tree_case(name)[5:]
    return [max(1.0, float(np.abs(r).max())) for r in ref]


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


SIZES = (1, 63, 64, 65, 130)
ALL = sorted(cases.DH_ROBOTS) + cases.TREES
BIG = set(cases.DH_BIG) | set(cases.TREE_BIG)              # 9 joints and more: the run-time-n kernels
SOME = ["puma560", "panda", "n2s", "n8m", "n9s", "n16m", "chain8", "tree5", "tree8", "tree9", "UR5", "KinovaGen3", "YuMi"]


@gpu
@pytest.mark.parametrize("name", ALL)
def test_gradients_equal_the_oracle(name):
    """every served robot, N = 1, 63, 64, 65, 130, both gradients at the bound; gq alone and gqd alone return the bits of the both-call"""
    torch = _torch()
    for N in SIZES:
        rb, q, qd, g, rq, rd = cases.case(name, N)
        assert (rb.n >= 9) == (name in BIG)
        dq, dqd, dg = _dev(torch, q, qd, g)
        gq, gqd = _vjp(rb, dq, dqd, dg)
        eq, ed = cases.rel_err(gq.cpu().numpy(), rq), cases.rel_err(gqd.cpu().numpy(), rd)
        print("coriolis_vjp %s N=%d: rel err gq %.3e gqd %.3e (|ref|max %.3g, %.3g)" % (name, N, eq, ed, np.abs(rq).max(), np.abs(rd).max()))
        assert eq <= cases.BOUND and ed <= cases.BOUND, (name, N, eq, ed)
        only_q, none = _vjp(rb, dq, dqd, dg, which=(True, False))
        assert none is None and torch.equal(only_q, gq)
        none, only_d = _vjp(rb, dq, dqd, dg, which=(False, True))
        assert none is None and torch.equal(only_d, gqd)


@gpu
@pytest.mark.parametrize("name", SOME)
def test_fused_call_equals_the_composition(name):
    """2 n launches of the existing adjoint at qd +- e_k, summed, against the one fused launch: within 2e-9 max(1, |ref|max) -- each is held to 1e-9 of
    the oracle"""
    torch = _torch()
    rb, q, qd, g = _distinct(name, 65)          # 65 distinct rows; the scale is the cached oracle rows'
    dq, dqd, dg = _dev(torch, q, qd, g)
    fused, comp = _vjp(rb, dq, dqd, dg), _composition(rb, dq, dqd, dg)
    for what, f, c, scale in zip(("gq", "gqd"), fused, comp, _scales(name)):
        err = float((f - c).abs().max()) / scale
        print("coriolis_vjp %s %s: fused against composition %.3e (scale %.3g)" % (name, what, err, scale))
        assert bool(torch.isfinite(f).all()) and err <= 2e-9, (name, what, err)


@gpu
@pytest.mark.parametrize("name", ["panda", "UR5"])
def test_homogeneity_in_qd(name):
    """gq(q, 2^40 qd) against 2^40 gq(q, qd) and gqd(q, 2^40 qd) against gqd(q, qd), per row at 1e-13 of the row's largest magnitude: a two-field
    adjoint scales exactly under a power of two, a polar evaluation at qd +- e_k loses about twelve digits there.  A qd row of zeros gives gq = 0."""
    torch = _torch()
    rb, q, qd, g, rq, rd = cases.case(name, 65)
    qd = np.array(qd)
    qd[7] = 0.0
    dq, dqd, dg = _dev(torch, q, qd, g)
    s = 2.0 ** 40
    a, b = _vjp(rb, dq, dqd, dg), _vjp(rb, dq, dqd * s, dg)
    for what, x, y in (("gq", a[0] * s, b[0]), ("gqd", a[1], b[1])):
        worst = float(((x - y).abs().amax(dim=1) / x.abs().amax(dim=1).clamp_min(1e-300)).max())
        print("coriolis_vjp %s %s: homogeneity, worst row %.3e" % (name, what, worst))
        assert bool(((x - y).abs().amax(dim=1) <= 1e-13 * x.abs().amax(dim=1)).all())
    assert not bool(a[0][7].any()) and not bool(b[0][7].any()) and bool(a[1][7].any())


def _frictionless(name):
    if name == "UR5":
        return rtbhip.urdf.load("UR5")
    return {"puma560": rtbhip.models.DH.Puma560, "panda": rtbhip.models.DH.Panda}[name]().nofriction(True, True)


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "UR5"])
def test_identity_through_two_functions(name):
    """sum w . (C(q, qd) qd) through the Coriolis Function and torch's matmul against sum w . rne(q, qd, 0, gravity = 0) through the inverse-dynamics
    Function, on a friction-free robot: two autograd paths to one number, the gradients of q and qd within 2e-9"""
    torch = _torch()
    rb = _frictionless(name)
    rng = np.random.default_rng(12)
    q0, qd0, w = (torch.from_numpy(rng.uniform(-r, r, (65, rb.n))).cuda() for r in (3, 2, 1))
    grads = []
    for f in (lambda a, b: (rb.coriolis(a, b) @ b.unsqueeze(2)).squeeze(2), lambda a, b: rb.rne(a, b, None, gravity=[0, 0, 0])):
        q, qd = q0.clone().requires_grad_(True), qd0.clone().requires_grad_(True)
        out = f(q, qd)
        assert out.grad_fn is not None
        (w * out).sum().backward()
        grads.append((q.grad, qd.grad))
    for what, a, b in zip(("gq", "gqd"), grads[0], grads[1]):
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print("coriolis identity %s %s: C qd against rne %.3e (|.|max %.3g)" % (name, what, err, float(b.abs().max())))
        assert err <= 2e-9


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n1s", "n8m", "n9s", "n16s", "tree5", "tree8", "UR5", "KinovaGen3"])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_guard_rows_every_row_written_inputs_unchanged(name, N):
    """gq and gqd between guard rows: the guards keep their bits, every live value is written, q, qd and gC (guarded too) are left as they were; an
    output that is not asked for is not written"""
    import flush_guard as fg
    torch = _torch()
    rb, q, qd, g, rq, rd = cases.case(name, N)
    n = rb.n
    gq, gqd = fg.Guarded(torch, N, n, "float64"), fg.Guarded(torch, N, n, "float64")
    dq = fg.Guarded(torch, N, n, "float64").load(torch, q)
    dqd = fg.Guarded(torch, N, n, "float64").load(torch, qd)
    dg = fg.Guarded(torch, N, n * n, "float64").load(torch, g.reshape(N, n * n))
    q0, qd0, g0 = dq.bits.clone(), dqd.bits.clone(), dg.bits.clone()
    fn = getattr(_lib.lib(), TREE_VJP if _is_tree(rb) else DH_VJP)
    _lib.check(fn(_handle(rb), dq.ptr, dqd.ptr, N, dg.ptr, gq.ptr, gqd.ptr, DEV, _stream(torch)))
    torch.cuda.synchronize()
    for out in (gq, gqd):
        assert out.guards_intact() and bool((out.live_bits() != out.pattern).all())
    assert torch.equal(dq.bits, q0) and torch.equal(dqd.bits, qd0) and torch.equal(dg.bits, g0)
    ref = _vjp(rb, *_dev(torch, q, qd, g))
    assert torch.equal(gq.live(), ref[0]) and torch.equal(gqd.live(), ref[1])
    assert cases.rel_err(gq.live().cpu().numpy(), rq) <= cases.BOUND and cases.rel_err(gqd.live().cpu().numpy(), rd) <= cases.BOUND
    # one output only: the other buffer, left out of the call, keeps its pattern everywhere
    for keep in (0, 1):
        a, b = fg.Guarded(torch, N, n, "float64"), fg.Guarded(torch, N, n, "float64")
        outs = (a.ptr, None) if keep == 0 else (None, b.ptr)
        _lib.check(fn(_handle(rb), dq.ptr, dqd.ptr, N, dg.ptr, outs[0], outs[1], DEV, _stream(torch)))
        torch.cuda.synchronize()
        wrote, idle = (a, b) if keep == 0 else (b, a)
        assert wrote.guards_intact() and torch.equal(wrote.live(), ref[keep])
        assert idle.guards_intact() and bool((idle.live_bits() == idle.pattern).all())


@gpu
@pytest.mark.parametrize("name", ["puma560", "n8s", "n9m", "tree7", "UR5", "KinovaGen3", "YuMi"])
def test_rows_are_independent(name):
    """a row's result does not depend on its tile mates: N = 65 DISTINCT rows against rows either side of the 8-, 32- and 64-row seams computed one
    at a time, and a row permutation permutes the results"""
    torch = _torch()
    N = 65
    rb, q, qd, g = _distinct(name, N)
    assert len({q[r].tobytes() for r in range(N)}) == N
    dq, dqd, dg = _dev(torch, q, qd, g)
    full = _vjp(rb, dq, dqd, dg)
    for r in (0, 1, 7, 8, 9, 31, 32, 62, 63, 64):
        one = _vjp(rb, dq[r:r + 1].contiguous(), dqd[r:r + 1].contiguous(), dg[r:r + 1].contiguous())
        assert torch.equal(one[0][0], full[0][r]) and torch.equal(one[1][0], full[1][r]), (name, r)
    perm = np.random.default_rng(5).permutation(N)
    pq, pqd, pg = _dev(torch, q[perm], qd[perm], g[perm])
    moved = _vjp(rb, pq, pqd, pg)
    idx = torch.from_numpy(perm).cuda()
    assert torch.equal(full[0][idx], moved[0]) and torch.equal(full[1][idx], moved[1])


@gpu
@pytest.mark.parametrize("name", ["panda", "n9s", "UR5", "tree9"])
def test_nonfinite_and_huge_joint_values_stay_in_their_row(name):
    """a register form and a run-time-n form of each entry point, N = 130 distinct rows (three tiles).  A NaN in q or qd of row 70 makes that row
    non-finite and no other: the other two tiles keep the BITS of the clean run; the tile mates (rows 64..127) stay finite and within
    2e-9 max(1, |ref|max) of the composition -- a NaN angle sends its whole wave through the library's sincos (rtb_sincos and tree_trig decide with
    wave_any), so a mate may differ from the clean run by the difference of the two routines and by nothing else; the run-time-n tree form always
    calls the library's, so there every row but 70 keeps its bits.  A NaN in gC never reaches the trigonometry: every row but 70 keeps its bits in
    every form.  One angle of 2^21 + 0.25 rad in row 5: the mates of tile 0 within the same bound, tiles 1 and 2 bit-equal, and row 5 itself at
    1e-9 max(1, |ref|max) of the oracle evaluated with h = 2^-10 (its own error there:
    test_the_oracle_is_a_hundred_times_finer_than_the_bound)."""
    torch = _torch()
    N, bad, big = 130, 70, 5
    rb, q, qd, g = _distinct(name, N)
    run = lambda a, b, c: [x.cpu().numpy() for x in _vjp(rb, *_dev(torch, a, b, c))]
    clean = run(q, qd, g)
    comp = [x.cpu().numpy() for x in _composition(rb, *_dev(torch, q, qd, g))]
    scale = _scales(name)
    for k in (0, 1):
        assert np.isfinite(clean[k]).all() and float(np.abs(clean[k] - comp[k]).max()) <= 2e-9 * scale[k]
    always_library = _is_tree(rb) and rb.n > 8          # csrc/tree_coriolis_vjp_kernels.hip: the NG = 0 branch of tree_coriolis_vjp_lane
    rows = np.arange(N)

    def check(what, got, row, depends, exact):
        tile = rows // 64 == row // 64
        mates, same = tile & (rows != row), (rows != row) if exact else ~tile
        for k, o in enumerate(("gq", "gqd")):
            if depends[k]:
                assert not np.isfinite(got[k][row]).all(), (name, what, o, "row %d is finite" % row)
            assert _bits(got[k][same], clean[k][same]), (name, what, o, "a row outside the tile differs from the clean run", np.flatnonzero((got[k] != clean[k]).any(axis=1))[:8])
            assert np.isfinite(got[k][mates]).all(), (name, what, o, "a tile mate is not finite", np.flatnonzero(~np.isfinite(got[k]).all(axis=1))[:8])
            err = float(np.abs(got[k][mates] - comp[k][mates]).max()) / scale[k]
            print("coriolis_vjp %s %s %s: tile mates against the composition %.3e" % (name, what, o, err))
            assert err <= 2e-9, (name, what, o, err)

    a = q.copy(); a[bad, 1] = np.nan
    check("NaN in q", run(a, qd, g), bad, (True, True), always_library)
    a = qd.copy(); a[bad, 1] = np.nan
    check("NaN in qd", run(q, a, g), bad, (True, False), always_library)          # (C is linear in qd: gqd does not depend on it)
    a = g.copy(); a[bad] = np.nan
    check("NaN in gC", run(q, qd, a), bad, (True, True), True)
    a = q.copy(); a[big, 2] = BIG_ANGLE
    got = run(a, qd, g)
    check("huge angle", got, big, (False, False), always_library)
    ref = _oracle(name, a[big:big + 1], qd[big:big + 1], g[big:big + 1], BIG_H)
    for k, o in enumerate(("gq", "gqd")):
        err = cases.rel_err(got[k][big:big + 1], ref[k])
        print("coriolis_vjp %s huge angle %s: row %d against the oracle at h = 2^-10 %.3e (|ref|max %.3g)" % (name, o, big, err, np.abs(ref[k]).max()))
        assert err <= cases.BOUND, (name, o, err)


@gpu
@pytest.mark.parametrize("name", ["puma560", "n9s", "tree6", "KinovaGen3"])
@pytest.mark.parametrize("N", [1, 65])
def test_host_memory_call_is_bit_equal(name, N):
    torch = _torch()
    rb, q, qd, g, rq, rd = cases.case(name, N)
    dev = _vjp(rb, *_dev(torch, q, qd, g))
    host = _vjp(rb, np.array(q), np.array(qd), np.array(g))
    assert np.array_equal(host[0], dev[0].cpu().numpy()) and np.array_equal(host[1], dev[1].cpu().numpy())
    only = _vjp(rb, np.array(q), np.array(qd), np.array(g), which=(False, True))
    assert only[0] is None and np.array_equal(only[1], host[1])


@gpu
def test_limits_and_refusals_on_device_tensors():
    torch = _torch()
    x = torch.zeros(4 * 21 * 21, dtype=torch.float64, device="cuda")
    p = C.c_void_p(x.data_ptr())
    err = lambda: _lib.lib().rtbhip_last_error().decode()
    keep = [cases.dh_cases.random_robot(17, 1, 5), _prismatic(), _long_tree(21), cases.tree_robot(cases.HAND)[0]]
    dh, tree = _lib.lib().rtbhip_coriolis_vjp, _lib.lib().rtbhip_tree_coriolis_vjp
    assert dh(keep[0]._dyn_handle(), p, p, 4, p, p, p, DEV, None) == ELIMIT and err() == "coriolis_vjp: chains of 1..16 joints"
    assert dh(keep[1]._dyn_handle(), p, p, 4, p, p, p, DEV, None) == EINVAL and err() == "coriolis_vjp: chain has a prismatic joint"
    assert tree(keep[2]._handle(), p, p, 4, p, p, p, DEV, None) == ELIMIT and err() == "tree_coriolis_vjp: robots of 1..20 joints"
    assert tree(keep[3]._handle(), p, p, 4, p, p, p, DEV, None) == EINVAL and err() == "tree_coriolis_vjp: " + _HAND
    torch.cuda.synchronize()
    assert not bool(x.any())
    # 16 joints and 20 joints are inside
    for rb in (cases.dh_robot("n16s"), _long_tree(20)):
        q, qd, g = cases.draw(rb.n, 3, 1)
        assert all(bool(torch.isfinite(o).all()) for o in _vjp(rb, *_dev(torch, q, qd, g)))
    # the front end of a hand-numbered robot and of a prismatic chain: the ordinary path, no graph
    for rb in (keep[3], keep[1]):
        q = torch.zeros((3, rb.n), dtype=torch.float64, device="cuda", requires_grad=True)
        assert rb.coriolis(q, q.detach()).grad_fn is None


# ---- autograd end to end
def _robots():
    return {"puma560": rtbhip.models.DH.Puma560(), "UR5": rtbhip.urdf.load("UR5")}


def _leaf(torch, rb, N, seed=3):
    q, qd, g = cases.draw(rb.n, N, seed)
    mk = lambda a: torch.from_numpy(np.array(a)).cuda()
    return mk(q).requires_grad_(True), mk(qd).requires_grad_(True), mk(g)


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_forward_bits_and_gradcheck(name):
    torch = _torch()
    rb = _robots()[name]
    q, qd, _ = _leaf(torch, rb, 3)
    Cm = rb.coriolis(q, qd)
    assert Cm.grad_fn is not None and tuple(Cm.shape) == (3, rb.n, rb.n)
    with torch.no_grad():
        assert torch.equal(rb.coriolis(q, qd), Cm)
    plain = rb.coriolis(q.detach(), qd.detach())
    assert torch.equal(plain, Cm) and plain.grad_fn is None
    assert torch.equal(rb.coriolis(q, qd.detach()), Cm) and torch.equal(rb.coriolis(q.detach(), qd), Cm)
    assert torch.autograd.gradcheck(lambda a, b: rb.coriolis(a, b), (q, qd))


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_backward_is_one_launch_and_asks_for_what_is_needed(monkeypatch, name):
    torch = _torch()
    import rtbhip.autograd
    rb = _robots()[name]
    q, qd, g = _leaf(torch, rb, 130)
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, attr):
            fn = getattr(real, attr)
            if "vjp" not in attr:
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((attr, _lib.last_launch()[:2], a[5] is not None, a[6] is not None))
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    mine = TREE_VJP if _is_tree(rb) else DH_VJP
    loss = (rb.coriolis(q, qd) * g).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [(mine, (3, 64), True, True)]          # three tiles of 64 rows, both gradients
    ref = _vjp(rb, q.detach(), qd.detach(), g)
    assert torch.equal(q.grad, ref[0]) and torch.equal(qd.grad, ref[1])
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    # one input only: NULL for the other
    del seen[:]
    q1 = q.detach().clone().requires_grad_(True)
    (rb.coriolis(q1, qd.detach()) * g).sum().backward()
    qd1 = qd.detach().clone().requires_grad_(True)
    (rb.coriolis(q.detach(), qd1) * g).sum().backward()
    torch.cuda.synchronize()
    assert seen == [(mine, (3, 64), True, False), (mine, (3, 64), False, True)]
    assert torch.equal(q1.grad, ref[0]) and torch.equal(qd1.grad, ref[1])
    # a loss that delivers an expanded (stride-0) gradient; a single configuration
    q2, qd2 = q.detach().clone().requires_grad_(True), qd.detach().clone().requires_grad_(True)
    rb.coriolis(q2, qd2).sum().backward()
    ones = _vjp(rb, q.detach(), qd.detach(), torch.ones_like(g))
    assert torch.equal(q2.grad, ones[0]) and torch.equal(qd2.grad, ones[1])
    a, b = q.detach()[0].clone().requires_grad_(True), qd.detach()[0].clone().requires_grad_(True)
    Cm = rb.coriolis(a, b)
    assert tuple(Cm.shape) == (rb.n, rb.n)
    (Cm * g[0]).sum().backward()
    assert tuple(a.grad.shape) == (rb.n,) and torch.equal(a.grad, ref[0][0]) and torch.equal(b.grad, ref[1][0])


@gpu
@pytest.mark.parametrize("name", ["panda", "UR5", "KinovaGen3"])
def test_graph_capture_and_replay(name):
    """the launch a backward pass makes, under torch.cuda.graph: the entry points only enqueue on the caller's stream -- captured after one eager
    warm-up (the table's upload), replayed to the eager result and again on new inputs"""
    torch = _torch()
    rb, q, qd, g, rq, rd = cases.case(name, 130)
    dq, dqd, dg = _dev(torch, q, qd, g)
    eager0 = [x.clone() for x in _vjp(rb, dq, dqd, dg)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _vjp(rb, dq, dqd, dg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager0[0]) and torch.equal(outs[1], eager0[1])
    dq.copy_(dq.flip(0))
    dqd.copy_(dqd * 2.0)
    dg.copy_(dg * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in outs]
    again = _vjp(rb, dq, dqd, dg)
    assert torch.equal(replayed[0], again[0]) and torch.equal(replayed[1], again[1])
