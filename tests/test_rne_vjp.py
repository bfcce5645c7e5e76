"""Differentiable DHRobot.rne / gravload / itorque / accel: rtbhip_rne_vjp, rtbhip_rne_vjp_f32 and the two Functions of rtbhip/autograd.py.

The oracle and its bound are those of tests/rne_vjp_cases.py: five-point Richardson differences (h = 1e-3) of the compiled reference, oracle.rne_dh,
contracted with gtau; bound 1e-9 max(1, |ref|max) over the compared array -- rne's contract in this project (tests/test_f32_io.py, smoke()) -- and
the exact identity gqdd = (reference inertia rows) . gtau at the same bound.  accel: the same stencil on oracle.accel_dh, bound
1e-9 kappa max(1, |ref|max) with kappa = max over the rows of cond(oracle.inertia_dh(q)): the backward pass solves with M twice, so rne's contract is
amplified by at most cond(M).  float32: f32_call(x32) == fp64_call(x32.double()).float() bit for bit.  gradcheck: torch's default tolerances.

No GPU is needed for the exports, the refusals of the raw ABI, the census, the front end's routing (a stand-in for a CUDA tensor) and the oracle's
own error."""
import ctypes as C
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH
from helpers import replaying
import rne_vjp_cases as cases

OK, EINVAL = 0, -1
HOST, DEV = 0, 1
BAD = 987654321
VJP = ("rtbhip_rne_vjp", "rtbhip_rne_vjp_f32")


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbols_are_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    for name in VJP:
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES and ("int %s(" % name) in hdr


def _prismatic():
    return DHRobot([RevoluteDH(a=0.3, m=1.0), PrismaticDH(alpha=0.5, m=1.0)])


class _Ctx:
    def __init__(self):
        self._keep = (rtbhip.models.DH.Puma560(), _prismatic())
        self.d, self.p = self._keep[0]._dyn_handle(), self._keep[1]._dyn_handle()
        self._buf = np.zeros(4096)
        self.B = self._buf.ctypes.data
        self.G = self.B + 8 * 2048


# (dyn, q, qd, qdd, N, grav3, fext6, gtau, gq, gqd, gqdd, mem, stream)
_NOTHING = "gq, gqd and gqdd are all NULL: there is nothing to compute"
_F32 = "rne_vjp_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)"
ROWS = []
for _name, _mem in (("rne_vjp", HOST), ("rne_vjp_f32", DEV)):
    _add = lambda tag, g, want, _name=_name: ROWS.append((_name + "-" + tag, "rtbhip_" + _name, g, want))
    _p = _name + ": "
    _add("unknown", lambda x, m=_mem: (BAD, x.B, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "unknown dyn handle"))
    _add("nullq", lambda x, m=_mem: (x.d, None, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgtau", lambda x, m=_mem: (x.d, x.B, x.B, x.B, 4, x.G, None, None, x.B, x.B, x.B, m, None), (EINVAL, _p + "NULL gtau"))
    _add("nothing", lambda x, m=_mem: (x.d, x.B, x.B, x.B, 4, x.G, None, x.B, None, None, None, m, None), (EINVAL, _p + _NOTHING))
    _add("negN", lambda x, m=_mem: (x.d, x.B, x.B, x.B, -1, x.G, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "negative N"))
    _add("mem7", lambda x: (x.d, x.B, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, x.B, 7, None), (EINVAL, _p + "bad mem kind"))
    _add("nullgravity", lambda x, m=_mem: (x.d, x.B, x.B, x.B, 4, None, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "NULL gravity"))
    _add("prismatic", lambda x, m=_mem: (x.p, x.B, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "chain has a prismatic joint"))
    _add("unknown+negN", lambda x, m=_mem: (BAD, x.B, x.B, x.B, -1, x.G, None, x.B, x.B, x.B, x.B, m, None), (EINVAL, _p + "unknown dyn handle"))
    _add("nullq+nothing", lambda x, m=_mem: (x.d, None, None, None, 4, x.G, None, x.B, None, None, None, m, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgtau+nothing", lambda x, m=_mem: (x.d, x.B, None, None, 4, x.G, None, None, None, None, None, m, None), (EINVAL, _p + "NULL gtau"))
    _add("empty", lambda x, m=_mem: (x.d, x.B, x.B, x.B, 0, x.G, None, x.B, x.B, x.B, x.B, m, None), (OK, None))
    _add("empty-prismatic", lambda x, m=_mem: (x.p, None, None, None, 0, None, None, None, None, None, None, m, None), (OK, None))
    _add("empty-null", lambda x, m=_mem: (x.d, None, None, None, 0, None, None, None, None, None, None, m, None), (OK, None))
ROWS.append(("rne_vjp_f32-hostmem", "rtbhip_rne_vjp_f32", lambda x: (x.d, x.B, x.B, x.B, 4, x.G, None, x.B, x.B, x.B, x.B, HOST, None), (EINVAL, _F32)))


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,fn,make,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, fn, make, want):
    rc = getattr(_lib.lib(), fn)(*make(ctx))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want


def test_the_rows_name_both_entry_points():
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for these two (rtbhip/_lib.py: _sq)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._sq}
    assert mine == set(VJP)
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert mine <= {fn for _, fn, _, want in ROWS if want[0] == OK} and mine <= {fn for _, fn, _, want in ROWS if want[0] != OK}
    assert len({r[0] for r in ROWS}) == len(ROWS)


# ------------------------------------------------------------------------------------------------ the oracle's own error (no GPU)
@pytest.mark.parametrize("name", ["puma560", "panda"])
def test_the_oracle_is_a_hundred_times_inside_the_bound(name):
    rb = cases.robot(name)
    q, qd, qdd, g = cases.draw(rb, 16, 99)
    a, b = cases.rne_oracle(rb, q, qd, qdd, g), cases.rne_oracle(rb, q, qd, qdd, g, h=cases.H / 2)
    for x, y in zip(a, b):
        assert float(np.abs(x - y).max()) <= 1e-11 * max(1.0, float(np.abs(x).max()))
    assert float(np.abs(a[2] - cases.inertia_gqdd(rb, q, g)).max()) <= 1.1e-11


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
    monkeypatch.setattr(rtbhip.autograd, "differentiable_rne", lambda robot, q, qd, qdd, gravity, fext: seen.append("rne") or "routed")
    monkeypatch.setattr(rtbhip.autograd, "differentiable_accel", lambda robot, q, qd, tq, gravity: seen.append("accel") or "routed")
    puma = rtbhip.models.DH.Puma560()
    t = lambda grad: _fake_cuda(torch, (5, 6), grad)
    # a grad-requiring q, qd or qdd -- any one of them -- reaches the Function
    for args in ((t(True), t(False), t(False)), (t(False), t(True), t(False)), (t(False), t(False), t(True)), (t(True), None, None)):
        del seen[:]
        assert puma.rne(*args) == "routed" and seen == ["rne"]
        if args[1] is not None:
            del seen[:]
            assert puma.accel(*args) == "routed" and seen == ["accel"]
    del seen[:]
    assert puma.gravload(t(True)) == "routed" and puma.itorque(t(True), t(False)) == "routed" and seen == ["rne", "rne"]
    del seen[:]
    # plain tensors, disabled gradients, base_wrench=True and a chain with a prismatic joint: the ordinary path, as before
    with pytest.raises(_Ordinary):
        puma.rne(t(False), t(False), t(False))
    with torch.no_grad(), pytest.raises(_Ordinary):
        puma.rne(t(True), t(True), t(True))
    with torch.no_grad(), pytest.raises(_Ordinary):
        puma.accel(t(True), t(True), t(True))
    with pytest.raises(_Ordinary):
        puma.rne(t(True), t(True), t(True), base_wrench=True)
    with pytest.raises(_Ordinary):
        puma.accel(t(False), t(False), t(False))
    pris = _prismatic()
    p = lambda grad: _fake_cuda(torch, (5, 2), grad)
    with pytest.raises(_Ordinary):
        pris.rne(p(True), p(True), p(True))
    with pytest.raises(_Ordinary):
        pris.accel(p(True), p(True), p(True))
    assert not seen
    # host arrays never come near it
    q = np.zeros((2, 6))
    assert not puma._wants_grad(q, q, q) and not puma._wants_grad(q, None, None)


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the inverse-dynamics adjoint runs on the device only: not served by the CPU replay")(f))


def _ptr(x):
    return None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data_as(C.c_void_p))


def _vjp(rb, q, qd, qdd, g, want=(True, True, True), gravity=None, fext=None, stream=None):
    """rtbhip_rne_vjp(_f32) on device tensors (current stream) or host arrays of one dtype -> [gq, gqd, gqdd], None where not wanted"""
    host = isinstance(q, np.ndarray)
    if host:
        outs = [np.full(q.shape, np.nan) if w else None for w in want]
        fn, mem = _lib.lib().rtbhip_rne_vjp, HOST
    else:
        torch = _torch()
        outs = [torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device) if w else None for w in want]
        fn = _lib.lib().rtbhip_rne_vjp_f32 if q.dtype == torch.float32 else _lib.lib().rtbhip_rne_vjp
        mem = DEV
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    f = None if fext is None else np.ascontiguousarray(fext, dtype=np.float64)
    gc = np.ascontiguousarray(rb._gravity_c(gravity))
    _lib.check(fn(rb._dyn_handle(), _ptr(q), _ptr(qd), _ptr(qdd), q.shape[0], _lib.host_ptr(gc), _lib.host_ptr(f), _ptr(g), _ptr(outs[0]), _ptr(outs[1]),
                  _ptr(outs[2]), mem, stream))
    return outs


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check(name, tag, got, ref):
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, ref):
        if a is None or b is None:
            continue
        err = cases.rel_err(a.cpu().numpy() if hasattr(a, "cpu") else a, b)
        print("rne_vjp %s %s %s: rel err %.3e" % (name, tag, what, err))
        assert err <= cases.BOUND, (name, tag, what, err)


SIZES = (1, 63, 64, 65, 130)


@gpu
@pytest.mark.parametrize("name", sorted(cases.ROBOTS))
@pytest.mark.parametrize("N", SIZES)
def test_gradients_equal_the_oracle(name, N):
    torch = _torch()
    rb, q, qd, qdd, g, _, _, ref = cases.case(name, N)
    got = _vjp(rb, *_dev(torch, q, qd, qdd, g))
    _check(name, "N=%d" % N, got, ref)
    assert cases.rel_err(got[2].cpu().numpy(), cases.inertia_gqdd(rb, q, g)) <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n3s", "n8m", "n9s", "n12m"])
def test_every_subset_autograd_can_ask_for_and_nothing_else_is_written(name):
    """q only, qd only, qdd only: the requested gradient has the bits of the all-three call, and of three adjacent poison-filled blocks only the one
    whose pointer was passed changes (nor does anything past row N)"""
    torch = _torch()
    N = 65
    rb, q, qd, qdd, g, _, _, ref = cases.case(name, N)
    dq, dqd, dqdd, dg = _dev(torch, q, qd, qdd, g)
    full = _vjp(rb, dq, dqd, dqdd, dg)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gc = np.ascontiguousarray(rb._gravity_c(None))
    for k in range(3):
        block = torch.full((3, N + 1, rb.n), -7.25, dtype=torch.float64, device="cuda")
        ptrs = [C.c_void_p(block[i].data_ptr()) if i == k else None for i in range(3)]
        _lib.check(_lib.lib().rtbhip_rne_vjp(rb._dyn_handle(), _ptr(dq), _ptr(dqd), _ptr(dqdd), N, _lib.host_ptr(gc), None, _ptr(dg), ptrs[0], ptrs[1], ptrs[2],
                                             DEV, stream))
        torch.cuda.synchronize()
        assert torch.equal(block[k, :N], full[k])
        rest = torch.ones((3, N + 1), dtype=torch.bool)
        rest[k, :N] = False
        assert bool((block[rest.cuda()] == -7.25).all())
    _check(name, "subsets", full, ref)


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n5s", "n5m", "n9m"])
@pytest.mark.parametrize("variant", ["noqd", "noqdd", "gravity", "fext", "base"])
def test_absent_inputs_gravity_wrench_and_base(name, variant):
    torch = _torch()
    N = 65
    rb, q, qd, qdd, g, gravity, fext, ref = cases.case(name, N, variant)
    got = _vjp(rb, *_dev(torch, q, qd, qdd, g), gravity=gravity, fext=fext)
    _check(name, variant, got, ref)


@gpu
@pytest.mark.parametrize("name", ["puma560", "n9s"])
@pytest.mark.parametrize("N", [1, 65])
def test_host_memory_call_is_bit_equal(name, N):
    torch = _torch()
    rb, q, qd, qdd, g, _, _, _ = cases.case(name, N)
    dev = _vjp(rb, *_dev(torch, q, qd, qdd, g))
    host = _vjp(rb, q.copy(), qd.copy(), qdd.copy(), g.copy())
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy())
    only = _vjp(rb, q.copy(), None, qdd.copy(), g.copy(), want=(True, False, False))
    assert np.array_equal(only[0], _vjp(rb, *_dev(torch, q, None, qdd, g), want=(True, False, False))[0].cpu().numpy())


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n9m"])
@pytest.mark.parametrize("N", [1, 65])
def test_f32_equals_rounded_fp64(name, N):
    torch = _torch()
    rb, q, qd, qdd, g, _, _, _ = cases.case(name, N)
    x32 = [x.float() for x in _dev(torch, q, qd, qdd, g)]
    got = _vjp(rb, *x32)
    want = _vjp(rb, *[x.double() for x in x32])
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b.float())


# ---- autograd end to end
def _puma_case(torch, N=3, seed=3):
    rb = cases.robot("puma560")
    q, qd, qdd, g = cases.draw(rb, N, seed)
    mk = lambda x: torch.from_numpy(np.array(x)).cuda().requires_grad_(True)
    return rb, mk(q), mk(qd), mk(qdd), torch.from_numpy(np.array(g)).cuda()


@gpu
def test_gradcheck():
    torch = _torch()
    rb, q, qd, qdd, _ = _puma_case(torch)
    tau = rb.rne(q, qd, qdd)
    assert tau.grad_fn is not None
    assert torch.autograd.gradcheck(lambda a, b, c: rb.rne(a, b, c), (q, qd, qdd))


@gpu
def test_backward_is_one_launch_for_what_was_asked_and_runs_once(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    rb, q, qd, qdd, g = _puma_case(torch, N=130)
    qd = qd.detach()                                   # no gradient asked for qd
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "vjp" not in name:
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((name, [x is not None for x in a[8:11]], _lib.last_launch()[:2]))
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    tau = rb.rne(q, qd, qdd)
    loss = (tau * g).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [("rtbhip_rne_vjp", [True, False, True], (3, 64))]          # three tiles of 64 rows
    want = _vjp(rb, q.detach(), qd, qdd.detach(), g)
    assert torch.equal(q.grad, want[0]) and torch.equal(qdd.grad, want[2]) and qd.grad is None
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


@gpu
def test_no_grad_path_is_unchanged_and_streams_are_honoured():
    torch = _torch()
    rb, q, qd, qdd, g = _puma_case(torch, N=65)
    tau = rb.rne(q, qd, qdd)
    with torch.no_grad():
        t0 = rb.rne(q, qd, qdd)
    t1 = rb.rne(q.detach(), qd.detach(), qdd.detach())
    assert t0.grad_fn is None and t1.grad_fn is None and not t0.requires_grad and torch.equal(tau, t0) and torch.equal(tau, t1)
    tw, wb = rb.rne(q, qd, qdd, base_wrench=True)
    assert tw.grad_fn is None and wb.grad_fn is None
    (tau * g).sum().backward()
    torch.cuda.synchronize()
    want = [x.grad.clone() for x in (q, qd, qdd)]
    for x in (q, qd, qdd):
        x.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (rb.rne(q, qd, qdd) * g).sum().backward()
    side.synchronize()
    torch.cuda.synchronize()
    for x, w in zip((q, qd, qdd), want):
        assert torch.equal(x.grad, w)


@gpu
def test_single_configuration_views_and_float32():
    torch = _torch()
    rb, q, qd, qdd, g = _puma_case(torch, N=4)
    ref = _vjp(rb, q.detach(), qd.detach(), qdd.detach(), g)
    one = [x.detach()[0].clone().requires_grad_(True) for x in (q, qd, qdd)]
    tau = rb.rne(*one)
    assert tuple(tau.shape) == (6,)
    (tau * g[0]).sum().backward()
    for x, r in zip(one, ref):
        assert tuple(x.grad.shape) == (6,) and torch.equal(x.grad, r[0])
    # a non-contiguous view: every other row of a longer batch
    wide = [torch.cat([x.detach(), x.detach()], dim=0)[torch.tensor([0, 4, 1, 5, 2, 6, 3, 7])].contiguous().requires_grad_(True) for x in (q, qd, qdd)]
    views = [x[::2] for x in wide]
    assert not views[0].is_contiguous()
    (rb.rne(*views) * g).sum().backward()
    for x, r in zip(wide, ref):
        assert torch.equal(x.grad[::2], r) and bool((x.grad[1::2] == 0).all())
    x32 = [x.detach().float().requires_grad_(True) for x in (q, qd, qdd)]
    t32 = rb.rne(*x32)
    assert t32.dtype == torch.float32
    (t32 * g.float()).sum().backward()
    x64 = [x.detach().double().requires_grad_(True) for x in x32]
    (rb.rne(*x64) * g.float().double()).sum().backward()
    for a, b in zip(x32, x64):
        assert a.grad.dtype == torch.float32 and torch.equal(a.grad, b.grad.float())


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda"])
def test_gravload_and_itorque_back_propagate(name):
    torch = _torch()
    N = 5
    rb, q, _, qdd, g, _, _, _ = cases.case(name, N)
    dq, dqdd, dg = _dev(torch, q, qdd, g)
    dq.requires_grad_(True)
    dqdd.requires_grad_(True)
    tg = rb.gravload(dq)
    assert tg.grad_fn is not None
    (tg * dg).sum().backward()
    ref = cases.rne_oracle(rb, q, None, None, g, which=(0,))
    assert cases.rel_err(dq.grad.cpu().numpy(), ref[0]) <= cases.BOUND
    dq.grad = None
    ti = rb.itorque(dq, dqdd)
    assert ti.grad_fn is not None
    (ti * dg).sum().backward()
    ref = cases.rne_oracle(rb, q, None, qdd, g, gravity=[0, 0, 0], which=(0, 2))
    assert cases.rel_err(dq.grad.cpu().numpy(), ref[0]) <= cases.BOUND and cases.rel_err(dqdd.grad.cpu().numpy(), ref[2]) <= cases.BOUND


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda"])
@pytest.mark.parametrize("N", [1, 65])
def test_accel_back_propagates(name, N):
    from oracle import oracle
    torch = _torch()
    rb, q, qd, tq, g, _, _, _ = cases.case(name, N)
    ref = cases.accel_oracle(rb, q, qd, tq, g)
    M = oracle.inertia_dh(rb.L24(), rb.mdh, q)
    kappa = max(float(np.linalg.cond(m)) for m in M)
    x = [t.requires_grad_(True) for t in _dev(torch, q, qd, tq)]
    qdd = rb.accel(*x)
    assert qdd.grad_fn is not None and tuple(qdd.shape) == ((rb.n,) if N == 1 else q.shape)
    (qdd.reshape(q.shape) * _dev(torch, g)[0]).sum().backward()
    torch.cuda.synchronize()
    for what, t, r in zip(("gq", "gqd", "gtorque"), x, ref):
        err = float(np.abs(t.grad.cpu().numpy() - r).max())
        print("accel vjp %s N=%d %s: err %.3e, bound %.3e (kappa %.1f)" % (name, N, what, err, 1e-9 * kappa * max(1.0, np.abs(r).max()), kappa))
        assert err <= 1e-9 * kappa * max(1.0, float(np.abs(r).max())), (name, N, what, err)
    lam = np.stack([np.linalg.solve(m, gi) for m, gi in zip(M, g)])
    assert float(np.abs(x[2].grad.cpu().numpy() - lam).max()) <= 1e-9 * kappa * max(1.0, float(np.abs(lam).max()))
    with torch.no_grad():
        assert torch.equal(rb.accel(*x), qdd)


@gpu
def test_graph_capture_and_replay():
    """rtbhip_rne_vjp only enqueues on the caller's stream: captured after one eager warm-up (the link table's upload), replayed on new inputs"""
    torch = _torch()
    N = 130
    rb, q, qd, qdd, g, _, _, _ = cases.case("panda", N)
    dq, dqd, dqdd, dg = _dev(torch, q, qd, qdd, g)
    eager0 = [x.clone() for x in _vjp(rb, dq, dqd, dqdd, dg)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _vjp(rb, dq, dqd, dqdd, dg)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager0):
        assert torch.equal(a, b)
    dq.copy_(dq.flip(0))
    dg.copy_(dg * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in outs]
    for a, b in zip(replayed, _vjp(rb, dq, dqd, dqdd, dg)):
        assert torch.equal(a, b)
