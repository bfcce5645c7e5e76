"""Differentiable ERobot.rne / gravload / itorque / accel and URDFRobot.rne: rtbhip_tree_rne_vjp and the two tree Functions of rtbhip/autograd.py.

The oracle and its bound are those of tests/tree_rne_vjp_cases.py: five-point Richardson differences (h = 1e-3) of the restated reference,
oracle.erobot.erobot_rne, contracted with gtau; bound 1e-9 max(1, |ref|max) over the compared array -- the DH adjoint's bound -- and the exact
identity gqdd = (reference inertia rows) . gtau at the same bound.  accel: the same stencil on erobot_accel, bound 1e-9 kappa max(1, |ref|max) with
kappa = max over the rows of cond(erobot_inertia(q)): the backward pass solves with M twice, so rne's contract is amplified by at most cond(M).
gradcheck: torch's default tolerances.  Every case draws 16 distinct rows and repeats them cyclically to N (the oracle is a Python loop).

No GPU is needed for the exports, the refusals of the raw ABI, the census, the front end's routing (a stand-in for a CUDA tensor) and the oracle's
own error."""
import ctypes as C
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import replaying
import tree_rne_vjp_cases as cases

OK, EINVAL = 0, -1
HOST, DEV = 0, 1
BAD = 987654321
VJP = "rtbhip_tree_rne_vjp"


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbol_is_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    assert hasattr(_lib.lib(), VJP) and VJP in _lib.SIGNATURES and ("int %s(" % VJP) in hdr


class _Ctx:
    def __init__(self):
        self._keep = cases.robot("tree5")[0]
        self.t = self._keep._handle()
        self._buf = np.zeros(4096)
        self.B = self._buf.ctypes.data
        self.G = self.B + 8 * 2048


# (tree, q, qd, qdd, N, gravity3, gtau, gq, gqd, gqdd, mem, stream)
_NOTHING = "gq, gqd and gqdd are all NULL: there is nothing to compute"
_P = "tree_rne_vjp: "
ROWS = [
    ("unknown", lambda x: (BAD, x.B, x.B, x.B, 4, x.G, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "unknown tree handle")),
    ("nullq", lambda x: (x.t, None, x.B, x.B, 4, x.G, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgtau", lambda x: (x.t, x.B, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "NULL gtau")),
    ("nothing", lambda x: (x.t, x.B, x.B, x.B, 4, x.G, x.B, None, None, None, HOST, None), (EINVAL, _P + _NOTHING)),
    ("negN", lambda x: (x.t, x.B, x.B, x.B, -1, x.G, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "negative N")),
    ("mem7", lambda x: (x.t, x.B, x.B, x.B, 4, x.G, x.B, x.B, x.B, x.B, 7, None), (EINVAL, _P + "bad mem kind")),
    ("nullgravity", lambda x: (x.t, x.B, x.B, x.B, 4, None, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "NULL gravity")),
    ("nullgravity-dev", lambda x: (x.t, x.B, x.B, x.B, 4, None, x.B, x.B, x.B, x.B, DEV, None), (EINVAL, _P + "NULL gravity")),
    ("unknown+negN", lambda x: (BAD, x.B, x.B, x.B, -1, x.G, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _P + "unknown tree handle")),
    ("nullq+nothing", lambda x: (x.t, None, None, None, 4, x.G, x.B, None, None, None, HOST, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgtau+nothing", lambda x: (x.t, x.B, None, None, 4, x.G, None, None, None, None, HOST, None), (EINVAL, _P + "NULL gtau")),
    ("nothing+nullgravity", lambda x: (x.t, x.B, None, None, 4, None, x.B, None, None, None, HOST, None), (EINVAL, _P + _NOTHING)),
    ("empty", lambda x: (x.t, x.B, x.B, x.B, 0, x.G, x.B, x.B, x.B, x.B, HOST, None), (OK, None)),
    ("empty-dev", lambda x: (x.t, x.B, x.B, x.B, 0, x.G, x.B, x.B, x.B, x.B, DEV, None), (OK, None)),
    ("empty-null", lambda x: (x.t, None, None, None, 0, None, None, None, None, None, HOST, None), (OK, None)),
]


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,make,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, make, want):
    ctx._buf[:] = 0.0
    rc = getattr(_lib.lib(), VJP)(*make(ctx))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want
    assert not ctx._buf.any()                    # a refusal and the empty batch touch nothing


def test_the_rows_name_the_entry_point():
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for this one (rtbhip/_lib.py: _st)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._st}
    assert mine == {VJP}
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert any(want[0] == OK for _, _, want in ROWS) and any(want[0] != OK for _, _, want in ROWS)
    assert len({r[0] for r in ROWS}) == len(ROWS)
    # a type of its own: the censuses of the other two families do not see it
    assert _lib._st is not _lib._sq and _lib._st is not _lib._sp and issubclass(_lib._st, _lib._sp)


# ------------------------------------------------------------------------------------------------ the oracle's own error (no GPU)
@pytest.mark.parametrize("name", ["chain8", "tree6", "tree8", "tree9", "UR5"])
def test_the_oracle_is_a_hundred_times_inside_the_bound(name):
    """h against h / 2 on the 16 rows the other tests compare on: <= 1e-11 max(1, |ref|max).
    What the comparison sees is the rounding noise of the h / 2 stencil, about 1.6 eps |tau|max / (h / 2) = 3.5e-13 |tau|max: independent of the
    gradient's size, while the figure is taken relative to max(1, |ref|max).  It stays under 1e-11 while |tau|max <= 28 max(1, |ref|max); the
    robots here are the case file's trees of 4..11 joints (and UR5) with |tau|max <= 20 max(1, |ref|max) for each of the three gradients, which the
    test asserts of its inputs.  Where the torques dwarf the contracted gradient the same measurement gives more -- tree5 1.3e-11 (gqd), tree7
    1.3e-11 (gqd), hand4 1.1e-11 (gqd), YuMi 1.6e-11 (gqdd), each at a ratio of 28..40 -- still sixty times inside the bound the adjoint is held
    to, and the adjoint agrees with the oracle to 6e-12 on all of them (tests/test_tree_rne_vjp_emu.py prints the figures)."""
    from oracle import erobot as oer
    rob, orc, q, qd, qdd, g, grav, a = cases.case(name)
    b = cases.rne_oracle(orc, q, qd, qdd, g, grav, h=cases.H / 2)
    tau = float(np.abs(oer.erobot_rne(orc, q, qd, qdd, grav)).max())
    for x, y in zip(a, b):
        err = float(np.abs(x - y).max()) / max(1.0, float(np.abs(x).max()))
        print("oracle %s: h against h/2 %.3e (|ref|max %.3g, |tau|max %.3g)" % (name, err, np.abs(x).max(), tau))
        assert tau <= 20.0 * max(1.0, float(np.abs(x).max()))
        assert err <= 1e-11
    assert cases.rel_err(a[2], cases.inertia_gqdd(orc, q, g)) <= 1.1e-11


# ------------------------------------------------------------------------------------------------ front-end routing (no GPU)
class _Ordinary(AssertionError):
    pass


def _fake_cuda(torch, shape, requires_grad):
    """what rtbhip takes for a CUDA tensor; the ordinary path stops at the first thing it asks of it"""
    class FakeCudaTensor:
        is_cuda = True

        def __init__(self):
            self.dtype, self.shape, self.requires_grad, self.device = torch.float64, tuple(shape), requires_grad, "cuda:0"

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
    monkeypatch.setattr(rtbhip.autograd, "differentiable_tree_rne", lambda robot, q, qd, qdd, gravity: seen.append(("rne", robot.n, gravity)) or "routed")
    monkeypatch.setattr(rtbhip.autograd, "differentiable_tree_accel", lambda robot, q, qd, tq, gravity: seen.append(("accel", robot.n, gravity)) or "routed")
    # the DH Functions are not where an ETS robot goes
    monkeypatch.setattr(rtbhip.autograd, "differentiable_rne", lambda *a: pytest.fail("the DH Function"))
    monkeypatch.setattr(rtbhip.autograd, "differentiable_accel", lambda *a: pytest.fail("the DH Function"))
    rob = cases.robot("tree5")[0]
    n = rob.n
    t = lambda grad: _fake_cuda(torch, (5, n), grad)
    # a grad-requiring q, qd or qdd -- any one of them -- reaches the Function
    for args in ((t(True), t(False), t(False)), (t(False), t(True), t(False)), (t(False), t(False), t(True)), (t(True), None, None)):
        del seen[:]
        assert rob.rne(*args) == "routed" and seen == [("rne", n, None)]
        if args[1] is not None:
            del seen[:]
            assert rob.accel(*args) == "routed" and seen == [("accel", n, None)]
    del seen[:]
    assert rob.gravload(t(True)) == "routed" and rob.itorque(t(True), t(False)) == "routed"
    assert seen == [("rne", n, None), ("rne", n, [0, 0, 0])]
    del seen[:]
    ur = rtbhip.urdf.load("UR5")
    u = lambda grad: _fake_cuda(torch, (5, 6), grad)
    assert ur.rne(u(True), u(False), u(False)) == "routed" and ur.gravload(u(True)) == "routed" and ur.itorque(u(False), u(True)) == "routed"
    assert ur.accel(u(False), u(True), u(False)) == "routed"
    yumi = rtbhip.urdf.load("YuMi")
    ex = tuple(e for e in cases.URDFS["YuMi"] if e in yumi.linkdict)
    ny = yumi.erobot(ex).n
    assert yumi.rne(_fake_cuda(torch, (2, ny), True), exclude=ex) == "routed"
    assert [s[:2] for s in seen] == [("rne", 6), ("rne", 6), ("rne", 6), ("accel", 6), ("rne", ny)]
    del seen[:]
    # plain tensors and disabled gradients: the ordinary path, as before
    with pytest.raises(_Ordinary):
        rob.rne(t(False), t(False), t(False))
    with pytest.raises(_Ordinary):
        rob.accel(t(False), t(False), t(False))
    with torch.no_grad(), pytest.raises(_Ordinary):
        rob.rne(t(True), t(True), t(True))
    with torch.no_grad(), pytest.raises(_Ordinary):
        rob.accel(t(True), t(True), t(True))
    with pytest.raises(_Ordinary):
        rob.inertia(t(True))
    with pytest.raises(_Ordinary):
        rob.coriolis(t(True), t(True))
    with pytest.raises(TypeError, match="Symbolic"):
        rob.rne(t(True), t(True), t(True), symbolic=True)
    # a hand-numbered robot: rne is differentiable (columns go by jindex), accel takes the ordinary path (M is not symmetric there)
    hand = cases.robot("hand4")[0]
    h = lambda grad: _fake_cuda(torch, (5, 4), grad)
    assert not hand._in_group_order() and rob._in_group_order()
    assert hand.rne(h(True), h(True), h(True)) == "routed" and seen == [("rne", 4, None)]
    del seen[:]
    with pytest.raises(_Ordinary):
        hand.accel(h(True), h(True), h(True))
    assert not seen
    # host arrays never come near it
    q = np.zeros((2, n))
    assert not any(_lib.wants_grad(x) for x in (q, None))
    e = np.zeros((0, n))                         # (an empty batch returns before any device is looked for)
    assert rob.rne(e, e, e).shape == (0, n) and rob.accel(e, e, e).shape == (0, n) and not seen


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the link-tree adjoint runs on the device only: not served by the CPU replay")(f))


def _ptr(x):
    return None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data_as(C.c_void_p))


def _vjp(rob, q, qd, qdd, g, want=(True, True, True), gravity=None, stream=None):
    """rtbhip_tree_rne_vjp on device tensors (current stream) or host arrays -> [gq, gqd, gqdd], None where not wanted"""
    host = isinstance(q, np.ndarray)
    if host:
        outs = [np.full(q.shape, np.nan) if w else None for w in want]
        mem = HOST
    else:
        torch = _torch()
        outs = [torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device) if w else None for w in want]
        mem = DEV
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    gc = np.ascontiguousarray(rob.gravity if gravity is None else gravity, dtype=np.float64)
    _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rob._handle(), _ptr(q), _ptr(qd), _ptr(qdd), q.shape[0], _lib.host_ptr(gc), _ptr(g), _ptr(outs[0]),
                                              _ptr(outs[1]), _ptr(outs[2]), mem, stream))
    return outs


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _tiled_case(name, N, variant="plain"):
    """the case's 16 rows repeated cyclically to N, with the oracle's answers tiled the same way"""
    rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name, variant)
    t = lambda x: cases.tiled(x, N)
    return rob, orc, t(q), t(qd), t(qdd), t(g), gravity, [t(r) for r in ref]


def _check(name, tag, got, ref):
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        if a is None or b is None:
            continue
        err = cases.rel_err(a.cpu().numpy() if hasattr(a, "cpu") else a, b)
        print("tree_rne_vjp %s %s %s: rel err %.3e" % (name, tag, what, err))
        assert err <= cases.BOUND, (name, tag, what, err)


SIZES = (1, 63, 64, 65, 130)


_IDENTITY = {}


def _gqdd_identity(name, N):
    if name not in _IDENTITY:
        rob, orc, q, qd, qdd, g, gravity, ref = cases.case(name)
        a = cases.inertia_gqdd(orc, q, g)
        a.setflags(write=False)
        _IDENTITY[name] = a
    return cases.tiled(_IDENTITY[name], N)


@gpu
@pytest.mark.parametrize("name", cases.ROBOTS)
@pytest.mark.parametrize("N", SIZES)
def test_gradients_equal_the_oracle(name, N):
    torch = _torch()
    rob, orc, q, qd, qdd, g, gravity, ref = _tiled_case(name, N)
    got = _vjp(rob, *_dev(torch, q, qd, qdd, g), gravity=gravity)
    _check(name, "N=%d" % N, got, ref)
    assert cases.rel_err(got[2].cpu().numpy(), _gqdd_identity(name, N)) <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["one_r", "chain8", "tree5", "tree8", "tree9", "UR5", "KinovaGen3", "hand4"])
def test_every_subset_autograd_can_ask_for_and_nothing_else_is_written(name):
    """q only, qd only, qdd only: the requested gradient has the bits of the all-three call, and of three adjacent poison-filled blocks only the one
    whose pointer was passed changes (nor does anything past row N)"""
    torch = _torch()
    N = 65
    rob, orc, q, qd, qdd, g, gravity, ref = _tiled_case(name, N)
    dq, dqd, dqdd, dg = _dev(torch, q, qd, qdd, g)
    full = _vjp(rob, dq, dqd, dqdd, dg)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gc = np.ascontiguousarray(rob.gravity, dtype=np.float64)
    for k in range(3):
        block = torch.full((3, N + 1, rob.n), -7.25, dtype=torch.float64, device="cuda")
        ptrs = [C.c_void_p(block[i].data_ptr()) if i == k else None for i in range(3)]
        _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rob._handle(), _ptr(dq), _ptr(dqd), _ptr(dqdd), N, _lib.host_ptr(gc), _ptr(dg), ptrs[0], ptrs[1], ptrs[2],
                                                  DEV, stream))
        torch.cuda.synchronize()
        assert torch.equal(block[k, :N], full[k])
        rest = torch.ones((3, N + 1), dtype=torch.bool)
        rest[k, :N] = False
        assert bool((block[rest.cuda()] == -7.25).all())
    _check(name, "subsets", full, ref)


@gpu
@pytest.mark.parametrize("name", ["chain3", "tree6", "tree9", "UR5", "hand4"])
@pytest.mark.parametrize("variant", ["noqd", "noqdd", "gravity"])
def test_absent_inputs_and_gravity(name, variant):
    torch = _torch()
    N = 65
    rob, orc, q, qd, qdd, g, gravity, ref = _tiled_case(name, N, variant)
    got = _vjp(rob, *_dev(torch, q, qd, qdd, g), gravity=gravity)
    _check(name, variant, got, ref)


@gpu
@pytest.mark.parametrize("name", ["tree7", "KinovaGen3"])
@pytest.mark.parametrize("N", [1, 65])
def test_host_memory_call_is_bit_equal(name, N):
    torch = _torch()
    rob, orc, q, qd, qdd, g, gravity, _ = _tiled_case(name, N)
    dev = _vjp(rob, *_dev(torch, q, qd, qdd, g))
    host = _vjp(rob, q.copy(), qd.copy(), qdd.copy(), g.copy())
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy())
    only = _vjp(rob, q.copy(), None, qdd.copy(), g.copy(), want=(True, False, False))
    assert np.array_equal(only[0], _vjp(rob, *_dev(torch, q, None, qdd, g), want=(True, False, False))[0].cpu().numpy())


# ---- autograd end to end
def _grad_case(torch, name, N, seed=3):
    rob, orc = cases.robot(name)
    q, qd, qdd, g = cases.draw(rob.n, seed, rows=N)
    mk = lambda x: torch.from_numpy(np.array(x)).cuda().requires_grad_(True)
    return rob, mk(q), mk(qd), mk(qdd), torch.from_numpy(np.array(g)).cuda()


@gpu
def test_gradcheck():
    torch = _torch()
    rob, q, qd, qdd, _ = _grad_case(torch, "tree3", 3)
    assert rob.n == 3 and not cases._props(rob)["serial"]
    tau = rob.rne(q, qd, qdd)
    assert tau.grad_fn is not None
    assert torch.autograd.gradcheck(lambda a, b, c: rob.rne(a, b, c), (q, qd, qdd))


@gpu
def test_backward_is_one_launch_for_what_was_asked_and_runs_once(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    rob, q, qd, qdd, g = _grad_case(torch, "tree6", 130)
    qd = qd.detach()                                   # no gradient asked for qd
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "vjp" not in name:
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((name, [x is not None for x in a[7:10]], _lib.last_launch()[:2]))
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    tau = rob.rne(q, qd, qdd)
    loss = (tau * g).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [("rtbhip_tree_rne_vjp", [True, False, True], (3, 64))]          # three tiles of 64 rows
    want = _vjp(rob, q.detach(), qd, qdd.detach(), g)
    assert torch.equal(q.grad, want[0]) and torch.equal(qdd.grad, want[2]) and qd.grad is None
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


@gpu
def test_no_grad_path_is_unchanged_and_streams_are_honoured():
    torch = _torch()
    rob, q, qd, qdd, g = _grad_case(torch, "tree7", 65)
    tau = rob.rne(q, qd, qdd)
    with torch.no_grad():
        t0 = rob.rne(q, qd, qdd)
    t1 = rob.rne(q.detach(), qd.detach(), qdd.detach())
    assert t0.grad_fn is None and t1.grad_fn is None and not t0.requires_grad and torch.equal(tau, t0) and torch.equal(tau, t1)
    (tau * g).sum().backward()
    torch.cuda.synchronize()
    want = [x.grad.clone() for x in (q, qd, qdd)]
    for x in (q, qd, qdd):
        x.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (rob.rne(q, qd, qdd) * g).sum().backward()
    side.synchronize()
    torch.cuda.synchronize()
    for x, w in zip((q, qd, qdd), want):
        assert torch.equal(x.grad, w)


@gpu
def test_single_configuration_views_and_float32():
    torch = _torch()
    rob, q, qd, qdd, g = _grad_case(torch, "tree5", 4)
    n = rob.n
    ref = _vjp(rob, q.detach(), qd.detach(), qdd.detach(), g)
    one = [x.detach()[0].clone().requires_grad_(True) for x in (q, qd, qdd)]
    tau = rob.rne(*one)
    assert tuple(tau.shape) == (n,)
    (tau * g[0]).sum().backward()
    for x, r in zip(one, ref):
        assert tuple(x.grad.shape) == (n,) and torch.equal(x.grad, r[0])
    # a non-contiguous view: every other row of a longer batch
    wide = [torch.cat([x.detach(), x.detach()], dim=0)[torch.tensor([0, 4, 1, 5, 2, 6, 3, 7])].contiguous().requires_grad_(True) for x in (q, qd, qdd)]
    views = [x[::2] for x in wide]
    assert not views[0].is_contiguous()
    (rob.rne(*views) * g).sum().backward()
    for x, r in zip(wide, ref):
        assert torch.equal(x.grad[::2], r) and bool((x.grad[1::2] == 0).all())
    # float32 rows are refused as they were, with or without requires_grad
    x32 = [x.detach().float() for x in (q, qd, qdd)]
    with pytest.raises(TypeError):
        rob.rne(*x32)
    with pytest.raises(TypeError):
        rob.rne(*[x.requires_grad_(True) for x in x32])


@gpu
def test_gravload_itorque_and_the_urdf_front_end_back_propagate():
    torch = _torch()
    N = 5
    er, orc, q, qd, qdd, g, gravity, _ = _tiled_case("UR5", N)
    ur = rtbhip.urdf.load("UR5")
    dq, dqd, dqdd, dg = _dev(torch, q, qd, qdd, g)
    for x in (dq, dqd, dqdd):
        x.requires_grad_(True)
    tg = ur.gravload(dq)
    assert tg.grad_fn is not None
    (tg * dg).sum().backward()
    ref = cases.rne_oracle(orc, q, None, None, g, gravity, which=(0,))
    assert cases.rel_err(dq.grad.cpu().numpy(), ref[0]) <= cases.BOUND
    dq.grad = None
    ti = ur.itorque(dq, dqdd)
    assert ti.grad_fn is not None
    (ti * dg).sum().backward()
    ref = cases.rne_oracle(orc, q, None, qdd, g, np.zeros(3), which=(0, 2))
    assert cases.rel_err(dq.grad.cpu().numpy(), ref[0]) <= cases.BOUND and cases.rel_err(dqdd.grad.cpu().numpy(), ref[2]) <= cases.BOUND
    dq.grad = dqdd.grad = None
    (ur.rne(dq, dqd, dqdd) * dg).sum().backward()
    want = _vjp(er, dq.detach(), dqd.detach(), dqdd.detach(), dg)
    for x, w in zip((dq, dqd, dqdd), want):
        assert torch.equal(x.grad, w)
    # exclude=: YuMi without its grippers
    ey, orcy, q, qd, qdd, g, gravity, refy = _tiled_case("YuMi", N)
    yumi = rtbhip.urdf.load("YuMi")
    ex = tuple(e for e in cases.URDFS["YuMi"] if e in yumi.linkdict)
    x = [t.requires_grad_(True) for t in _dev(torch, q, qd, qdd)]
    (yumi.rne(*x, exclude=ex) * _dev(torch, g)[0]).sum().backward()
    _check("YuMi", "exclude", [t.grad for t in x], refy)


def test_accel_of_ur5_has_no_reference_to_compare_with():
    """(no GPU)  The reference keeps SpatialInertia(m, r) of every link and no inertia tensor (Robot.py:1793-1800).  UR5's last moving link carries
    its mass ON its joint axis, the links behind it are massless: row and column 6 of the reference's M(q) are exactly zero, and its accel
    (numpy.linalg.solve) raises for every q.  kappa is infinite and the accel bound says nothing, so the device comparison below runs on branched
    random trees, whose M is regular; UR5's rne gradients are compared in every other test of this file."""
    from oracle import erobot as oer
    rob, orc = cases.robot("UR5")
    q, qd, tq, g = cases.draw(rob.n, 77, rows=2)
    M = oer.erobot_inertia(orc, q)
    assert not M[:, 5, :].any() and not M[:, :, 5].any() and all(np.isinf(np.linalg.cond(m)) for m in M)
    with pytest.raises(np.linalg.LinAlgError):
        oer.erobot_accel(orc, q, qd, tq, cases.gravity_of(rob, "plain"))


@gpu
@pytest.mark.parametrize("name", ["tree5", "tree6"])
@pytest.mark.parametrize("N", [1, 65])
def test_accel_back_propagates(name, N):
    torch = _torch()
    rob, orc = cases.robot(name)
    q16, qd16, tq16, g16 = cases.draw(rob.n, 77)
    grav = cases.gravity_of(rob, "plain")
    ref16, M16 = _accel_ref(name, orc, q16, qd16, tq16, g16, grav)
    t = lambda a: cases.tiled(a, N)
    q, qd, tq, g, ref, M = t(q16), t(qd16), t(tq16), t(g16), [t(r) for r in ref16], t(M16)
    kappa = max(float(np.linalg.cond(m)) for m in M16)
    x = [a.requires_grad_(True) for a in _dev(torch, q, qd, tq)]
    qdd = rob.accel(*x)
    assert qdd.grad_fn is not None and tuple(qdd.shape) == ((rob.n,) if N == 1 else q.shape)
    (qdd.reshape(q.shape) * _dev(torch, g)[0]).sum().backward()
    torch.cuda.synchronize()
    for what, a, r in zip(("gq", "gqd", "gtorque"), x, ref):
        err = float(np.abs(a.grad.cpu().numpy() - r).max())
        print("tree accel vjp %s N=%d %s: err %.3e, bound %.3e (kappa %.1f)" % (name, N, what, err, 1e-9 * kappa * max(1.0, np.abs(r).max()), kappa))
        assert err <= 1e-9 * kappa * max(1.0, float(np.abs(r).max())), (name, N, what, err)
    lam = np.stack([np.linalg.solve(m, gi) for m, gi in zip(M, g)])
    assert float(np.abs(x[2].grad.cpu().numpy() - lam).max()) <= 1e-9 * kappa * max(1.0, float(np.abs(lam).max()))
    with torch.no_grad():
        assert torch.equal(rob.accel(*x), qdd)


_ACCEL = {}


def _accel_ref(name, orc, q, qd, tq, g, grav):
    """the accel oracle and the reference's inertia rows of the 16 drawn rows: computed once per robot"""
    from oracle import erobot as oer
    if name not in _ACCEL:
        _ACCEL[name] = (cases.accel_oracle(orc, q, qd, tq, g, grav), oer.erobot_inertia(orc, q))
    return _ACCEL[name]


@gpu
def test_graph_capture_and_replay():
    """rtbhip_tree_rne_vjp only enqueues on the caller's stream: captured after one eager warm-up (the group table's upload), replayed on new inputs"""
    torch = _torch()
    N = 130
    rob, orc, q, qd, qdd, g, gravity, _ = _tiled_case("tree8", N)
    dq, dqd, dqdd, dg = _dev(torch, q, qd, qdd, g)
    eager0 = [x.clone() for x in _vjp(rob, dq, dqd, dqdd, dg)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _vjp(rob, dq, dqd, dqdd, dg)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager0):
        assert torch.equal(a, b)
    dq.copy_(dq.flip(0))
    dg.copy_(dg * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in outs]
    for a, b in zip(replayed, _vjp(rob, dq, dqd, dqdd, dg)):
        assert torch.equal(a, b)
