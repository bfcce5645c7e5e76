"""Differentiable DHRobot.inertia / ERobot.inertia: rtbhip_inertia_vjp, rtbhip_tree_inertia_vjp and the two Functions of rtbhip/autograd.py.

The oracle and its bound are those of tests/inertia_vjp_cases.py: five-point Richardson differences (h = 1e-3) of the reference's inertia matrix
(oracle.inertia_dh, oracle.erobot.erobot_inertia), one q column at a time, contracted with a NON-symmetric gM; bound 1e-9 max(1, |ref|max) over the
compared array.  The fused call against the composition it replaces -- n launches of rtbhip_rne_vjp / rtbhip_tree_rne_vjp at qdd = e_i,
gtau = gM[:, i, :], summed -- at 2e-9 max(1, |ref|max): each side is held to 1e-9 of the same oracle.  gradcheck: torch's default tolerances.

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
import inertia_vjp_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
HOST, DEV = 0, 1
BAD = 987654321
DH_VJP, TREE_VJP = "rtbhip_inertia_vjp", "rtbhip_tree_inertia_vjp"
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


# (handle, q, N, gM, gq, mem, stream)
ROWS = []
for _name, _kind, _ok, _spec in (("inertia_vjp", "dyn", "d", (("prismatic", "p", EINVAL, "chain has a prismatic joint"), ("17joints", "d17", ELIMIT, "chains of 1..16 joints"))),
                                 ("tree_inertia_vjp", "tree", "t", (("handnumbered", "h", EINVAL, _HAND), ("21joints", "t21", ELIMIT, "robots of 1..20 joints")))):
    _add = lambda tag, g, want, _name=_name: ROWS.append((_name + "-" + tag, "rtbhip_" + _name, g, want))
    _p = _name + ": "
    _add("unknown", lambda x: (BAD, x.B, 4, x.B, x.B, HOST, None), (EINVAL, _p + "unknown %s handle" % _kind))
    _add("nullq", lambda x, k=_ok: (getattr(x, k), None, 4, x.B, x.B, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgM", lambda x, k=_ok: (getattr(x, k), x.B, 4, None, x.B, HOST, None), (EINVAL, _p + "NULL gM"))
    _add("nullgq", lambda x, k=_ok: (getattr(x, k), x.B, 4, x.B, None, HOST, None), (EINVAL, _p + "NULL gq"))
    _add("negN", lambda x, k=_ok: (getattr(x, k), x.B, -1, x.B, x.B, HOST, None), (EINVAL, _p + "negative N"))
    _add("mem7", lambda x, k=_ok: (getattr(x, k), x.B, 4, x.B, x.B, 7, None), (EINVAL, _p + "bad mem kind"))
    _add("unknown+negN", lambda x: (BAD, x.B, -1, x.B, x.B, HOST, None), (EINVAL, _p + "unknown %s handle" % _kind))
    _add("nullq+nullgM", lambda x, k=_ok: (getattr(x, k), None, 4, None, None, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgM+nullgq", lambda x, k=_ok: (getattr(x, k), x.B, 4, None, None, HOST, None), (EINVAL, _p + "NULL gM"))
    _add("negN+mem7", lambda x, k=_ok: (getattr(x, k), x.B, -1, x.B, x.B, 7, None), (EINVAL, _p + "negative N"))
    for _tag, _k, _rc, _why in _spec:
        for _mem in (HOST, DEV):          # refused before any memory is looked at
            _add(_tag + ("-dev" if _mem == DEV else ""), lambda x, k=_k, m=_mem: (getattr(x, k), x.B, 4, x.B, x.B, m, None), (_rc, _p + _why))
        _add("empty-" + _tag, lambda x, k=_k: (getattr(x, k), None, 0, None, None, HOST, None), (OK, None))
    _add("empty", lambda x, k=_ok: (getattr(x, k), x.B, 0, x.B, x.B, HOST, None), (OK, None))
    _add("empty-dev", lambda x, k=_ok: (getattr(x, k), x.B, 0, x.B, x.B, DEV, None), (OK, None))
    _add("empty-null", lambda x, k=_ok: (getattr(x, k), None, 0, None, None, HOST, None), (OK, None))


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
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for these two (rtbhip/_lib.py: _si)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._si}
    assert mine == set(VJP)
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert mine <= {fn for _, fn, _, want in ROWS if want[0] == OK} and mine <= {fn for _, fn, _, want in ROWS if want[0] != OK}
    assert len({r[0] for r in ROWS}) == len(ROWS)
    # a type of its own that the censuses of the other families do not see: no subclass of theirs, not the plain void pointer
    assert not issubclass(_lib._si, _lib._sp) and _lib._si != _lib._vp and issubclass(_lib._si, C.c_void_p)
    assert _lib._si.from_param(None) is None and isinstance(_lib._si.from_param(C.c_void_p(8)), C.c_void_p)


# ------------------------------------------------------------------------------------------------ the oracle's own error (no GPU)
@pytest.mark.parametrize("name", ["puma560", "panda", "UR5"])
def test_the_oracle_is_a_hundred_times_finer_than_the_bound(name):
    """the stencil at h against h / 2: <= 1e-11 max(1, |ref|max), a hundredth of the bound the adjoint is held to; panda and UR5 also with one
    joint at 2^21 + 0.25 rad, h = 2^-10 against h / 2"""
    if name == "UR5":
        rob, orc, q, g, a = cases.tree_case(name)
        b = cases.tree_oracle(orc, q, g, h=cases.H / 2)
    else:
        rb, q, g, a = cases.dh_case(name, 24)
        b = cases.dh_oracle(rb, q, g, h=cases.H / 2)
    err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(a).max()))
    print("inertia oracle %s: h against h/2 %.3e (|ref|max %.3g)" % (name, err, np.abs(a).max()))
    assert err <= 1e-11
    if name in ("panda", "UR5"):
        # one joint at 2^21 + 0.25 rad, the stencil at h = 2^-10 against h / 2: the reference can supply the number that
        # test_nonfinite_and_huge_joint_values_stay_in_their_row compares that row with
        q, g = (np.array(x) for x in cases.draw(q.shape[1], 2, 5))
        q[:, 2] = BIG_ANGLE
        a, b = _oracle(name, q, g, BIG_H), _oracle(name, q, g, BIG_H / 2)
        err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(a).max()))
        print("inertia oracle %s at a huge angle: h = 2^-10 against h/2 %.3e (|ref|max %.3g)" % (name, err, np.abs(a).max()))
        assert err <= 1e-11


BIG_ANGLE = 2.0 ** 21 + 0.25          # beyond 2^20: the wave of such a lane takes the library's sine and cosine (csrc/inertia_vjp_kernels.hip: rne_trig in inertia_vjp_lane; tree_trig)
BIG_H = 2.0 ** -10                    # q +- h and q +- 2 h are exact doubles at that magnitude (one ulp is 2^-31); at h = 1e-3 they are not, six digits lost


def _oracle(name, q, g, h):
    if name in cases.DH_ROBOTS:
        return cases.dh_oracle(cases.dh_robot(name), q, g, h=h)
    return cases.tree_oracle(cases.tree_robot(name)[1], q, g, h=h)


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
    monkeypatch.setattr(rtbhip.autograd, "differentiable_inertia", lambda robot, q: seen.append(("dh", robot.n)) or "routed")
    monkeypatch.setattr(rtbhip.autograd, "differentiable_tree_inertia", lambda robot, q: seen.append(("tree", robot.n)) or "routed")
    puma = rtbhip.models.DH.Puma560()
    t = lambda grad, **kw: _fake_cuda(torch, (5, 6), grad, **kw)
    assert puma.inertia(t(True)) == "routed" and puma.inertia(_fake_cuda(torch, (6,), True)) == "routed" and seen == [("dh", 6), ("dh", 6)]
    del seen[:]
    rob = cases.tree_robot("tree5")[0]
    u = lambda grad: _fake_cuda(torch, (5, rob.n), grad)
    ur = rtbhip.urdf.load("UR5")
    yumi = rtbhip.urdf.load("YuMi")
    ex = tuple(e for e in cases.tree_cases.URDFS["YuMi"] if e in yumi.linkdict)
    ny = yumi.erobot(ex).n
    assert rob.inertia(u(True)) == "routed" and ur.inertia(t(True)) == "routed" and yumi.inertia(_fake_cuda(torch, (2, ny), True), exclude=ex) == "routed"
    assert seen == [("tree", rob.n), ("tree", 6), ("tree", ny)]
    del seen[:]
    # plain tensors, disabled gradients, float32 rows, a prismatic DH chain and a hand-numbered tree: the ordinary path, as before
    for robot, mk in ((puma, t), (rob, u)):
        with pytest.raises(_Ordinary):
            robot.inertia(mk(False))
        with torch.no_grad(), pytest.raises(_Ordinary):
            robot.inertia(mk(True))
    with pytest.raises(TypeError, match="float64"):
        puma.inertia(t(True, dtype=torch.float32))
    with pytest.raises(TypeError, match="float64"):
        ur.inertia(t(True, dtype=torch.float32))
    with pytest.raises(_Ordinary):
        _prismatic().inertia(_fake_cuda(torch, (5, 2), True))
    hand = cases.tree_robot(cases.HAND)[0]
    assert not hand._in_group_order() and rob._in_group_order()
    with pytest.raises(_Ordinary):
        hand.inertia(_fake_cuda(torch, (5, 4), True))
    assert not seen
    # host arrays never come near it
    assert not _lib.wants_grad(np.zeros((2, 6)))
    e = np.zeros((0, rob.n))                     # (an empty batch returns before any device is looked for)
    assert rob.inertia(e).shape == (0, rob.n, rob.n) and not seen


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the inertia adjoint runs on the device only: not served by the CPU replay")(f))


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


def _vjp(rb, q, g, out=None):
    """the fused entry point on device tensors (current stream) or host arrays -> gq"""
    fn = getattr(_lib.lib(), TREE_VJP if _is_tree(rb) else DH_VJP)
    if isinstance(q, np.ndarray):
        gq = np.full(q.shape, np.nan)
        _lib.check(fn(_handle(rb), _ptr(q), q.shape[0], _ptr(g), _ptr(gq), HOST, None))
        return gq
    torch = _torch()
    gq = torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device) if out is None else out
    _lib.check(fn(_handle(rb), _ptr(q), q.shape[0], _ptr(g), gq if isinstance(gq, C.c_void_p) else _ptr(gq), DEV, _stream(torch)))
    return gq


def _composition(rb, q, g):
    """what the fused call replaces: n launches of the inverse-dynamics adjoint at qd = 0, qdd = e_i, gtau = gM[:, i, :], no gravity, summed"""
    torch = _torch()
    n = rb.n
    zero = np.zeros(3)
    total = None
    for i in range(n):
        e = torch.zeros_like(q)
        e[:, i] = 1.0
        gi = g[:, i, :].contiguous()
        gq = torch.empty_like(q)
        if _is_tree(rb):
            _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rb._handle(), _ptr(q), None, _ptr(e), q.shape[0], _lib.host_ptr(zero), _ptr(gi), _ptr(gq), None, None,
                                                      DEV, _stream(torch)))
        else:
            _lib.check(_lib.lib().rtbhip_rne_vjp(rb._dyn_handle(), _ptr(q), None, _ptr(e), q.shape[0], _lib.host_ptr(zero), None, _ptr(gi), _ptr(gq), None,
                                                 None, DEV, _stream(torch)))
        total = gq if total is None else total + gq
    return total


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _case(name, N):
    """(robot, q (N, n), gM (N, n, n), ref (N, n)) of a DH robot or a link tree (its ROWS rows repeated cyclically to N)"""
    if name in cases.DH_ROBOTS:
        return cases.dh_case(name, N)
    rob, orc, q, g, ref = cases.tree_case(name)
    return rob, cases.tiled(q, N), cases.tiled(g, N), cases.tiled(ref, N)


def _distinct(name, N):
    """(robot, q, gM) of N DISTINCT rows from the cases' input distribution, no oracle: for comparisons of bits and of one device result with
    another.  (A tree case repeats 8 rows, and there a row that lands a multiple of 8 away still meets its expected bits.)"""
    rb = cases.dh_robot(name) if name in cases.DH_ROBOTS else cases.tree_robot(name)[0]
    return (rb,) + tuple(np.array(x) for x in cases.draw(rb.n, N, cases._seed(name, N) + 1))


def _scale(name):
    """max(1, |ref|max) from the cached oracle rows of the same robot and the same input distribution"""
    ref = cases.dh_case(name, 65)[3] if name in cases.DH_ROBOTS else cases.tree_case(name)[4]
    return max(1.0, float(np.abs(ref).max()))


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


SIZES = (1, 63, 64, 65, 130)
ALL = sorted(cases.DH_ROBOTS) + cases.TREES
BIG = set(cases.DH_BIG) | set(cases.TREE_BIG)              # 9 joints and more: the run-time-n kernels, at N = 65 only
_ORACLE = [(name, N) for name in ALL for N in SIZES if N == 65 or name not in BIG]
SOME = ["puma560", "panda", "n2s", "n8m", "n9s", "n16m", "chain8", "tree5", "tree8", "tree9", "UR5", "KinovaGen3", "YuMi"]


@gpu
@pytest.mark.parametrize("name,N", _ORACLE, ids=["%s-%d" % x for x in _ORACLE])
def test_gradient_equals_the_oracle(name, N):
    torch = _torch()
    rb, q, g, ref = _case(name, N)
    assert (rb.n >= 9) == (name in BIG)
    got = _vjp(rb, *_dev(torch, q, g)).cpu().numpy()
    err = cases.rel_err(got, ref)
    print("inertia_vjp %s N=%d: rel err %.3e (|ref|max %.3g)" % (name, N, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, N, err)


@gpu
@pytest.mark.parametrize("name", SOME)
def test_fused_call_equals_the_composition(name):
    """n launches of the existing adjoint, summed, against the one fused launch: within 2e-9 max(1, |ref|max) -- each is held to 1e-9 of the oracle.
    (The fused kernel is the specialised form: its passes skip the exact zeros of a robot at rest, start at link i and read the folded gM, so
    the two differ by rounding, not only by the order of the n - 1 adds.)"""
    torch = _torch()
    rb, q, g = _distinct(name, 65)          # 65 distinct rows; the scale is the cached oracle rows'
    dq, dg = _dev(torch, q, g)
    fused, comp = _vjp(rb, dq, dg).cpu().numpy(), _composition(rb, dq, dg).cpu().numpy()
    scale = _scale(name)
    err = float(np.abs(fused - comp).max()) / scale
    print("inertia_vjp %s: fused against composition %.3e (scale %.3g)" % (name, err, scale))
    assert np.isfinite(fused).all() and err <= 2e-9, (name, err)


@gpu
@pytest.mark.parametrize("name", ["panda", "n5s", "n9m", "tree6", "UR5", "tree9"])
def test_mirrored_entries_both_count(name):
    """a gM that is zero except at one (i, j), i != j, gives the same gq as its transpose (and not zero): M[i,j] and M[j,i] are one computed value"""
    torch = _torch()
    rb, q, g, ref = _case(name, 65)
    n = rb.n
    for i, j in ((0, n - 1), (1, 2), (n - 2, 1)):
        one = np.zeros_like(g)
        one[:, i, j] = 0.7
        dq, a, b = _dev(torch, q, one, one.transpose(0, 2, 1))
        ga, gb = _vjp(rb, dq, a), _vjp(rb, dq, b)
        assert torch.equal(ga, gb)
        if name in cases.DH_ROBOTS:          # generic link tables (a tree has structural zeros: two branches, a point mass on the last joint's axis)
            assert float(ga.abs().max()) > 0


@gpu
@pytest.mark.parametrize("name", ["puma560", "n8s", "n12m", "tree8", "UR5", "KinovaGen3"])
def test_symmetrised_gradient_gives_the_same_answer(name):
    torch = _torch()
    rb, q, g, ref = _case(name, 65)
    dq, a, b = _dev(torch, q, g, 0.5 * (g + g.transpose(0, 2, 1)))
    ga, gb = _vjp(rb, dq, a).cpu().numpy(), _vjp(rb, dq, b).cpu().numpy()
    err = float(np.abs(ga - gb).max()) / max(1.0, float(np.abs(ref).max()))
    print("inertia_vjp %s: gM against (gM + gM^T) / 2 %.3e" % (name, err))
    assert err <= cases.BOUND and cases.rel_err(gb, ref) <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n1s", "n8m", "n9s", "n16s", "tree5", "tree8", "UR5", "KinovaGen3"])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_guard_rows_every_row_written_inputs_unchanged(name, N):
    """gq between guard rows of one allocation: the guards keep their bits, every live value is written, q and gM (guarded too) are left as they were"""
    import flush_guard as fg
    torch = _torch()
    rb, q, g, ref = _case(name, N)
    n = rb.n
    gq = fg.Guarded(torch, N, n, "float64")
    dq = fg.Guarded(torch, N, n, "float64").load(torch, q)
    dg = fg.Guarded(torch, N, n * n, "float64").load(torch, g.reshape(N, n * n))
    q0, g0 = dq.bits.clone(), dg.bits.clone()
    fn = getattr(_lib.lib(), TREE_VJP if _is_tree(rb) else DH_VJP)
    _lib.check(fn(_handle(rb), dq.ptr, N, dg.ptr, gq.ptr, DEV, _stream(torch)))
    torch.cuda.synchronize()
    assert gq.guards_intact() and bool((gq.live_bits() != gq.pattern).all())
    assert torch.equal(dq.bits, q0) and torch.equal(dg.bits, g0)
    assert torch.equal(gq.live(), _vjp(rb, *_dev(torch, q, g)))
    assert cases.rel_err(gq.live().cpu().numpy(), ref) <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["puma560", "n8s", "n9m", "tree7", "UR5", "KinovaGen3", "YuMi"])
def test_rows_are_independent(name):
    """N = 65 DISTINCT rows: rows either side of the 8-, 32- and 64-row seams have the bits of the same row computed alone, and a row permutation
    of the inputs permutes gq bit for bit"""
    torch = _torch()
    N = 65
    rb, q, g = _distinct(name, N)
    assert len({q[r].tobytes() for r in range(N)}) == N
    perm = np.random.default_rng(5).permutation(N)
    dq, dg, pq, pg = _dev(torch, q, g, q[perm], g[perm])
    full = _vjp(rb, dq, dg)
    for r in (0, 1, 7, 8, 9, 31, 32, 62, 63, 64):
        assert torch.equal(_vjp(rb, dq[r:r + 1].contiguous(), dg[r:r + 1].contiguous())[0], full[r]), (name, r)
    assert torch.equal(full[torch.from_numpy(perm).cuda()], _vjp(rb, pq, pg))


@gpu
@pytest.mark.parametrize("name", ["panda", "n9s", "UR5", "tree9"])
def test_nonfinite_and_huge_joint_values_stay_in_their_row(name):
    """a register form and a run-time-n form of each entry point, N = 130 distinct rows (three tiles).  A NaN in q of row 70 makes that row
    non-finite and no other: the other two tiles keep the BITS of the clean run; the tile mates (rows 64..127) stay finite and within
    2e-9 max(1, |ref|max) of the composition -- a NaN angle sends its whole wave through the library's sincos (rtb_sincos and tree_trig decide with
    wave_any), so a mate may differ from the clean run by the difference of the two routines and by nothing else; the run-time-n tree form always
    calls the library's, so there every row but 70 keeps its bits.  A NaN in gM never reaches the trigonometry: every row but 70 keeps its bits in
    every form.  One angle of 2^21 + 0.25 rad in row 5: the mates of tile 0 within the same bound, tiles 1 and 2 bit-equal, and row 5 itself at
    1e-9 max(1, |ref|max) of the oracle evaluated with h = 2^-10 (its own error there: test_the_oracle_is_a_hundred_times_finer_than_the_bound)."""
    torch = _torch()
    N, bad, big = 130, 70, 5
    rb, q, g = _distinct(name, N)
    run = lambda a, b: _vjp(rb, *_dev(torch, a, b)).cpu().numpy()
    clean = run(q, g)
    comp = _composition(rb, *_dev(torch, q, g)).cpu().numpy()
    scale = _scale(name)
    assert np.isfinite(clean).all() and float(np.abs(clean - comp).max()) <= 2e-9 * scale
    always_library = _is_tree(rb) and rb.n > 8          # csrc/tree_inertia_vjp_kernels.hip: the NG = 0 branch of tree_inertia_vjp_lane
    rows = np.arange(N)

    def check(what, got, row, depends, exact):
        tile = rows // 64 == row // 64
        mates, same = tile & (rows != row), (rows != row) if exact else ~tile
        if depends:
            assert not np.isfinite(got[row]).all(), (name, what, "row %d is finite" % row)
        assert _bits(got[same], clean[same]), (name, what, "a row outside the tile differs from the clean run", np.flatnonzero((got != clean).any(axis=1))[:8])
        assert np.isfinite(got[mates]).all(), (name, what, "a tile mate is not finite", np.flatnonzero(~np.isfinite(got).all(axis=1))[:8])
        err = float(np.abs(got[mates] - comp[mates]).max()) / scale
        print("inertia_vjp %s %s: tile mates against the composition %.3e" % (name, what, err))
        assert err <= 2e-9, (name, what, err)

    a = q.copy(); a[bad, 1] = np.nan
    check("NaN in q", run(a, g), bad, True, always_library)
    a = g.copy(); a[bad] = np.nan
    check("NaN in gM", run(q, a), bad, True, True)
    a = q.copy(); a[big, 2] = BIG_ANGLE
    got = run(a, g)
    check("huge angle", got, big, False, always_library)
    ref = _oracle(name, a[big:big + 1], g[big:big + 1], BIG_H)
    err = cases.rel_err(got[big:big + 1], ref)
    print("inertia_vjp %s huge angle: row %d against the oracle at h = 2^-10 %.3e (|ref|max %.3g)" % (name, big, err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)


@gpu
@pytest.mark.parametrize("name", ["puma560", "n9s", "tree6", "KinovaGen3"])
@pytest.mark.parametrize("N", [1, 65])
def test_host_memory_call_is_bit_equal(name, N):
    torch = _torch()
    rb, q, g, ref = _case(name, N)
    dev = _vjp(rb, *_dev(torch, q, g))
    host = _vjp(rb, np.array(q), np.array(g))
    assert np.array_equal(host, dev.cpu().numpy())


@gpu
def test_limits_and_refusals_on_device_tensors():
    torch = _torch()
    x = torch.zeros(4 * 21 * 21, dtype=torch.float64, device="cuda")
    p = C.c_void_p(x.data_ptr())
    err = lambda: _lib.lib().rtbhip_last_error().decode()
    keep = [cases.dh_cases.random_robot(17, 1, 5), _prismatic(), _long_tree(21), cases.tree_robot(cases.HAND)[0]]
    assert _lib.lib().rtbhip_inertia_vjp(keep[0]._dyn_handle(), p, 4, p, p, DEV, None) == ELIMIT and err() == "inertia_vjp: chains of 1..16 joints"
    assert _lib.lib().rtbhip_inertia_vjp(keep[1]._dyn_handle(), p, 4, p, p, DEV, None) == EINVAL and err() == "inertia_vjp: chain has a prismatic joint"
    assert _lib.lib().rtbhip_tree_inertia_vjp(keep[2]._handle(), p, 4, p, p, DEV, None) == ELIMIT and err() == "tree_inertia_vjp: robots of 1..20 joints"
    assert _lib.lib().rtbhip_tree_inertia_vjp(keep[3]._handle(), p, 4, p, p, DEV, None) == EINVAL and err() == "tree_inertia_vjp: " + _HAND
    torch.cuda.synchronize()
    assert not bool(x.any())
    # the forward calls serve both sizes' neighbours: 16 joints and 20 joints are inside
    for rb in (cases.dh_robot("n16s"), _long_tree(20)):
        q, g = cases.draw(rb.n, 3, 1)
        assert bool(torch.isfinite(_vjp(rb, *_dev(torch, q, g))).all())
    # the front end of a hand-numbered robot and of a prismatic chain: the ordinary path, no graph
    for rb in (keep[3], keep[1]):
        q = torch.zeros((3, rb.n), dtype=torch.float64, device="cuda", requires_grad=True)
        assert rb.inertia(q).grad_fn is None


# ---- autograd end to end
def _robots():
    return {"puma560": rtbhip.models.DH.Puma560(), "UR5": rtbhip.urdf.load("UR5")}


def _leaf(torch, rb, N, seed=3):
    q, g = cases.draw(rb.n, N, seed)
    return torch.from_numpy(np.array(q)).cuda().requires_grad_(True), torch.from_numpy(np.array(g)).cuda()


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_gradcheck(name):
    torch = _torch()
    rb = _robots()[name]
    q, _ = _leaf(torch, rb, 3)
    M = rb.inertia(q)
    assert M.grad_fn is not None and tuple(M.shape) == (3, rb.n, rb.n)
    with torch.no_grad():
        assert torch.equal(rb.inertia(q), M)
    assert torch.equal(rb.inertia(q.detach()), M) and rb.inertia(q.detach()).grad_fn is None
    assert torch.autograd.gradcheck(lambda a: rb.inertia(a), (q,))


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_backward_is_one_launch_and_runs_once(monkeypatch, name):
    torch = _torch()
    import rtbhip.autograd
    rb = _robots()[name]
    q, g = _leaf(torch, rb, 130)
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, attr):
            fn = getattr(real, attr)
            if "vjp" not in attr:
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((attr, _lib.last_launch()[:2]))
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    loss = (rb.inertia(q) * g).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [(TREE_VJP if _is_tree(rb) else DH_VJP, (3, 64))]          # three tiles of 64 rows
    assert torch.equal(q.grad, _vjp(rb, q.detach(), g))
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_single_configuration_views_and_side_stream(name):
    torch = _torch()
    rb = _robots()[name]
    n = rb.n
    q, g = _leaf(torch, rb, 4)
    ref = _vjp(rb, q.detach(), g)
    one = q.detach()[0].clone().requires_grad_(True)
    M = rb.inertia(one)
    assert tuple(M.shape) == (n, n)
    (M * g[0]).sum().backward()
    assert tuple(one.grad.shape) == (n,) and torch.equal(one.grad, ref[0])
    # a non-contiguous view: every other row of a longer batch; the rows not used get a zero gradient
    wide = torch.cat([q.detach(), q.detach()], dim=0)[torch.tensor([0, 4, 1, 5, 2, 6, 3, 7])].contiguous().requires_grad_(True)
    view = wide[::2]
    assert not view.is_contiguous()
    (rb.inertia(view) * g).sum().backward()
    assert torch.equal(wide.grad[::2], ref) and bool((wide.grad[1::2] == 0).all())
    # a loss that delivers an expanded (stride-0) gradient
    q2 = q.detach().clone().requires_grad_(True)
    rb.inertia(q2).sum().backward()
    assert torch.equal(q2.grad, _vjp(rb, q.detach(), torch.ones_like(g)))
    # a side stream
    q3 = q.detach().clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (rb.inertia(q3) * g).sum().backward()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(q3.grad, ref)


@gpu
@pytest.mark.parametrize("name", ["puma560", "UR5"])
def test_kinetic_energy_identity(name):
    """qd^T M(q) qd through the inertia Function and qd . itorque(q, qd) through the inverse-dynamics Function: two autograd paths to one number"""
    torch = _torch()
    rb = _robots()[name]
    q, _ = _leaf(torch, rb, 65)
    qd = torch.from_numpy(np.random.default_rng(8).uniform(-2, 2, (65, rb.n))).cuda()
    (qd.unsqueeze(1) @ rb.inertia(q) @ qd.unsqueeze(2)).sum().backward()
    a = q.grad.clone()
    q.grad = None
    (qd * rb.itorque(q, qd)).sum().backward()
    b = q.grad
    err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    print("kinetic energy %s: d(qd^T M qd)/dq against d(qd . itorque)/dq %.3e (|.|max %.3g)" % (name, err, float(b.abs().max())))
    assert err <= 2e-9


@gpu
@pytest.mark.parametrize("name", ["panda", "UR5", "KinovaGen3"])
def test_graph_capture_and_replay(name):
    """the entry points only enqueue on the caller's stream: captured after one eager warm-up (the table's upload), replayed on new inputs"""
    torch = _torch()
    N = 130
    rb, q, g, ref = _case(name, N)
    dq, dg = _dev(torch, q, g)
    eager0 = _vjp(rb, dq, dg).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _vjp(rb, dq, dg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    dq.copy_(dq.flip(0))
    dg.copy_(dg * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert torch.equal(replayed, _vjp(rb, dq, dg))
