"""Differentiable ETS.link_frames / fkine_all: rtbhip_link_frames_vjp and _FramesVJP of rtbhip/autograd.py -- the gradient of a loss on every link
frame, one backward launch for all of them.

The oracle and its bound are those of tests/link_frames_vjp_cases.py: one prefix chain per mark through the compiled reference restated in
oracle/ (oracle.fkine, oracle.jacob0), contracted in NumPy; G ~ U(-1, 1); bound 1e-10 absolute, the project's kinematics criterion.
gradcheck: torch's default tolerances.  Every case draws 24 distinct rows and repeats them cyclically to N.

No GPU is needed for the exports, the refusals of the raw ABI, the census and the front end's routing (a stand-in for a CUDA tensor, as in
tests/test_f32_io.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import product_ets, replaying
import link_frames_vjp_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
HOST, DEV = 0, 1
BAD = 987654321
VJP = "rtbhip_link_frames_vjp"


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbol_is_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    assert hasattr(_lib.lib(), VJP) and VJP in _lib.SIGNATURES and ("int %s(" % VJP) in hdr


class _Ctx:
    def __init__(self):
        self._keep = rtbhip.models.Panda().ets(), product_ets([("tx", 0.3), ("Rz", 0.2)])
        self.c, self.k = self._keep[0]._handle(), self._keep[1]._handle()       # Panda (22 transforms); a chain of constants
        self._buf = np.zeros(4096)
        self.B = self._buf.ctypes.data
        self._marks = {k: np.array(v, dtype=np.int32) for k, v in dict(ok=[0, 2, 22], down=[3, 2, 5], far=[0, 2, 23], neg=[-1, 2, 5], many=[1] * 34, k=[0, 1, 2]).items()}
        self.M, self.Mdown, self.Mfar, self.Mneg, self.Mmany, self.Mk = (self._marks[k].ctypes.data for k in ("ok", "down", "far", "neg", "many", "k"))


# (chain, q, N, base16, marks, nmarks, gF, gq, mem, stream)
_P = "link_frames_vjp: "
_MARKS = "marks must be nondecreasing transform counts in 0..m"
ROWS = [
    ("unknown", lambda x: (BAD, x.B, 4, None, x.M, 3, x.B, x.B, HOST, None), (EINVAL, _P + "unknown chain handle")),
    ("mem7", lambda x: (x.c, x.B, 4, None, x.M, 3, x.B, x.B, 7, None), (EINVAL, _P + "bad mem kind")),
    ("negN", lambda x: (x.c, x.B, -1, None, x.M, 3, x.B, x.B, HOST, None), (EINVAL, _P + "negative N")),
    ("nullmarks", lambda x: (x.c, x.B, 4, None, None, 3, x.B, x.B, HOST, None), (EINVAL, _P + "NULL marks")),
    ("nullq", lambda x: (x.c, None, 4, None, x.M, 3, x.B, x.B, HOST, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgF", lambda x: (x.c, x.B, 4, None, x.M, 3, None, x.B, HOST, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgq", lambda x: (x.c, x.B, 4, None, x.M, 3, x.B, None, HOST, None), (EINVAL, _P + "NULL gq")),
    ("nullgq-dev", lambda x: (x.c, x.B, 4, None, x.M, 3, x.B, None, DEV, None), (EINVAL, _P + "NULL gq")),
    ("nojoints", lambda x: (x.k, x.B, 4, None, x.Mk, 3, x.B, x.B, HOST, None), (EINVAL, _P + "chain has no joints")),
    ("toomany", lambda x: (x.c, x.B, 4, None, x.Mmany, 34, x.B, x.B, HOST, None), (ELIMIT, _P + "at most 33 frames per call")),
    ("decreasing", lambda x: (x.c, x.B, 4, None, x.Mdown, 3, x.B, x.B, HOST, None), (EINVAL, _P + _MARKS)),
    ("outofrange", lambda x: (x.c, x.B, 4, None, x.Mfar, 3, x.B, x.B, HOST, None), (EINVAL, _P + _MARKS)),
    ("negative-mark", lambda x: (x.c, x.B, 4, None, x.Mneg, 3, x.B, x.B, HOST, None), (EINVAL, _P + _MARKS)),
    ("decreasing-empty", lambda x: (x.c, x.B, 0, None, x.Mdown, 3, x.B, x.B, HOST, None), (EINVAL, _P + _MARKS)),
    # first failure wins, in the order of the rows above
    ("unknown+negN", lambda x: (BAD, x.B, -1, None, x.M, 3, x.B, x.B, HOST, None), (EINVAL, _P + "unknown chain handle")),
    ("mem7+negN", lambda x: (x.c, x.B, -1, None, x.M, 3, x.B, x.B, 7, None), (EINVAL, _P + "bad mem kind")),
    ("nullmarks+nullq", lambda x: (x.c, None, 4, None, None, 3, x.B, x.B, HOST, None), (EINVAL, _P + "NULL marks")),
    ("nullq+nullgq", lambda x: (x.c, None, 4, None, x.M, 3, x.B, None, HOST, None), (EINVAL, _P + "NULL input with N > 0")),
    ("nullgq+nojoints", lambda x: (x.k, x.B, 4, None, x.Mk, 3, x.B, None, HOST, None), (EINVAL, _P + "NULL gq")),
    ("nojoints+decreasing", lambda x: (x.k, x.B, 4, None, x.Mdown, 3, x.B, x.B, HOST, None), (EINVAL, _P + "chain has no joints")),
    ("empty", lambda x: (x.c, x.B, 0, None, x.M, 3, x.B, x.B, HOST, None), (OK, None)),
    ("empty-dev", lambda x: (x.c, x.B, 0, None, x.M, 3, x.B, x.B, DEV, None), (OK, None)),
    ("empty-null", lambda x: (x.c, None, 0, None, None, 0, None, None, HOST, None), (OK, None)),
    ("empty-nomarks", lambda x: (x.c, x.B, 0, None, x.M, 0, x.B, x.B, HOST, None), (OK, None)),
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


def test_mark_refusals_are_those_of_link_frames(ctx):
    """the same lowering (chain.cpp: compile_frames) says the same thing under either name"""
    L = _lib.lib()
    for marks, nm in ((ctx.Mdown, 3), (ctx.Mfar, 3), (ctx.Mmany, 34)):
        rc0 = L.rtbhip_link_frames(ctx.c, ctx.B, 4, None, marks, nm, ctx.B, HOST, None)
        e0 = L.rtbhip_last_error().decode()
        rc1 = L.rtbhip_link_frames_vjp(ctx.c, ctx.B, 4, None, marks, nm, ctx.B, ctx.B, HOST, None)
        e1 = L.rtbhip_last_error().decode()
        assert rc0 == rc1 != 0 and e0.startswith("link_frames: ") and e1 == "link_frames_vjp: " + e0[len("link_frames: "):]


def test_no_marks_means_zeros(ctx):
    """nmarks == 0 with N > 0: no frame depends on q -- gq is zero-filled on the host without a launch"""
    ctx._buf[:] = 7.0
    assert _lib.lib().rtbhip_link_frames_vjp(ctx.c, ctx.B + 8 * 1024, 4, None, None, 0, None, ctx.B, HOST, None) == OK
    assert not ctx._buf[:28].any() and bool((ctx._buf[28:] == 7.0).all())
    ctx._buf[:] = 0.0


def test_the_rows_name_the_entry_point():
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for this one (rtbhip/_lib.py: _sf)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._sf}
    assert mine == {VJP}
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert any(want[0] == OK for _, _, want in ROWS) and any(want[0] != OK for _, _, want in ROWS)
    assert len({r[0] for r in ROWS}) == len(ROWS)
    # a type of its own: the censuses of the other three families do not see it
    assert all(_lib._sf is not t for t in (_lib._st, _lib._sq, _lib._sp)) and issubclass(_lib._sf, _lib._sp)


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

    class Recording:
        @staticmethod
        def apply(q, ets, marks, base):
            seen.append((ets.n, [int(m) for m in marks], None if base is None else np.asarray(base).shape))
            return "routed"

    monkeypatch.setattr(rtbhip.autograd, "_FramesVJP", Recording)
    ets = cases.ets_of("panda")
    t = lambda grad, n=7: _fake_cuda(torch, (5, n), grad)
    assert ets.link_frames(t(True), [0, 2, 22]) == "routed" and seen == [(7, [0, 2, 22], None)]
    del seen[:]
    assert ets.link_frames(t(True), [4], base=np.eye(4)) == "routed" and seen == [(7, [4], (16,))]
    del seen[:]
    # the robots' fkine_all hand the tensor straight through
    assert rtbhip.models.Panda().fkine_all(t(True)) == "routed" and seen == [(7, cases.PANDA_MARKS, None)]
    del seen[:]
    puma = rtbhip.models.DH.Puma560()
    assert puma.fkine_all(t(True, 6)) == "routed" and [s[0] for s in seen] == [6] and len(seen[0][1]) == 7
    del seen[:]
    # plain tensors and disabled gradients: the ordinary path, as before
    with pytest.raises(_Ordinary):
        ets.link_frames(t(False), [0, 2, 22])
    with torch.no_grad(), pytest.raises(_Ordinary):
        ets.link_frames(t(True), [0, 2, 22])
    with pytest.raises(_Ordinary):
        puma.fkine_all(t(False, 6))
    # a chain of constants has nothing to differentiate: the ordinary path
    with pytest.raises(_Ordinary):
        product_ets([("tx", 0.3), ("Rz", 0.2)]).link_frames(_fake_cuda(torch, (5, 0), True), [0, 1])
    assert not seen
    # host arrays never come near it
    assert not _lib.wants_grad(np.zeros((2, 7)))
    assert ets.link_frames(np.zeros((0, 7)), [0, 1]).shape == (0, 2, 4, 4) and not seen


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the all-frame adjoint runs on the device only: not served by the CPU replay")(f))


def _ptr(x):
    return None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data_as(C.c_void_p))


def _vjp(ets, marks, base, q, G, stream=None):
    """rtbhip_link_frames_vjp on device tensors (current stream) or host arrays -> gq"""
    mk = np.ascontiguousarray(marks, dtype=np.int32)
    b = None if base is None else np.ascontiguousarray(base, dtype=np.float64).reshape(16)
    if isinstance(q, np.ndarray):
        out, mem = np.full(q.shape, np.nan), HOST
    else:
        torch = _torch()
        out, mem = torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device), DEV
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    _lib.check(_lib.lib().rtbhip_link_frames_vjp(ets._handle(), _ptr(q), q.shape[0], _lib.host_ptr(b), _lib.host_ptr(mk), len(mk), _ptr(G), _ptr(out),
                                                 mem, stream))
    return out


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _tiled_case(name, N):
    ets, marks, base, q, G, ref = cases.case(name)
    return ets, marks, base, cases.tiled(q, N), cases.tiled(G, N), cases.tiled(ref, N)


def _err(got, ref):
    return float(np.abs((got.detach().cpu().numpy() if hasattr(got, "cpu") else got) - ref).max())


SIZES = (1, 63, 64, 65, 193)


def test_every_kernel_size_is_among_the_cases():
    ns = sorted(cases.ets_of(name).n for name in cases.CASES)
    assert set(range(1, 9)) <= set(ns) and 9 in ns and 32 in ns


@gpu
@pytest.mark.parametrize("name", list(cases.CASES))
@pytest.mark.parametrize("N", SIZES)
def test_gradients_equal_the_oracle(name, N):
    torch = _torch()
    ets, marks, base, q, G, ref = _tiled_case(name, N)
    dq, dG = _dev(torch, q, G)
    got = _vjp(ets, marks, base, dq, dG)
    torch.cuda.synchronize()
    err = _err(got, ref)
    print("link_frames_vjp %s N=%d (n = %d, %d marks): err %.3e" % (name, N, ets.n, len(marks), err))
    assert err <= cases.BOUND, (name, N, err)
    assert _lib.last_launch()[:2] == ((N + 63) // 64, 64)          # one configuration per lane, 64-lane tiles
    again = _vjp(ets, marks, base, dq, dG)
    assert torch.equal(got, again)                                 # the same inputs: the same bits
    if name == "zeros":
        assert not bool(got.any())
    if name == "cols":
        assert not bool(got[:, [0, 2, 4]].any())


@gpu
@pytest.mark.parametrize("name", ["two", "panda_base", "cols", "n9"])
def test_host_memory_call_is_bit_equal(name):
    torch = _torch()
    ets, marks, base, q, G, ref = _tiled_case(name, 65)
    dev = _vjp(ets, marks, base, *_dev(torch, q, G))
    host = _vjp(ets, marks, base, q.copy(), G.copy())
    assert np.array_equal(host, dev.cpu().numpy()) and _err(host, ref) <= cases.BOUND


@gpu
def test_the_bottom_row_of_G_changes_no_bit_and_no_marks_means_zeros():
    torch = _torch()
    ets, marks, base, q, G, ref = _tiled_case("panda_base", 65)
    dq, dG = _dev(torch, q, G)
    a = _vjp(ets, marks, base, dq, dG)
    dG[:, :, 3, :] = 1e300
    assert torch.equal(a, _vjp(ets, marks, base, dq, dG))
    assert not bool(_vjp(ets, [], base, dq, None).any())


# ---- autograd end to end
def _grad_q(torch, q):
    return torch.from_numpy(np.array(q)).cuda().requires_grad_(True)


@gpu
def test_equals_the_composition_of_per_prefix_fkine_calls(monkeypatch):
    """what a user had before: one differentiable fkine of a prefix chain per frame -- and the fused backward is ONE launch"""
    torch = _torch()
    import rtbhip.autograd
    N = 130
    ets, marks, base, q, G, ref = _tiled_case("panda_base", N)
    dG = _dev(torch, G)[0]
    a = _grad_q(torch, q)
    loss = None
    for m, k in enumerate(marks):
        pre = ets[:k]
        if pre.n == 0:
            continue
        term = (pre.eval(a[:, :pre.q_width], base=base) * dG[:, m]).sum()
        loss = term if loss is None else loss + term
    loss.backward()
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "vjp" not in name:
                return fn

            def call(*args):
                rc = fn(*args)
                seen.append((name, _lib.last_launch()[:2]))
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    b = _grad_q(torch, q)
    F = ets.link_frames(b, marks, base=base)
    assert F.grad_fn is not None and torch.equal(F, ets.link_frames(b.detach(), marks, base=base))
    loss = (F * dG).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [("rtbhip_link_frames_vjp", (3, 64))]           # three tiles of 64 rows
    err = float((a.grad - b.grad).abs().max())
    print("link_frames_vjp against %d prefix fkine calls: %.3e" % (len(marks), err))
    assert err <= cases.BOUND and _err(b.grad, ref) <= cases.BOUND
    assert torch.equal(b.grad, _vjp(ets, marks, base, b.detach(), dG))
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


@gpu
def test_gradcheck():
    torch = _torch()
    ets, marks, base, q, G, ref = cases.case("rxry")
    assert ets.n == 3
    a = _grad_q(torch, q[:3])
    assert torch.autograd.gradcheck(lambda x: ets.link_frames(x, marks), (a,))


@gpu
def test_partial_losses_single_rows_and_streams():
    torch = _torch()
    N = 65
    ets, marks, base, q, G, ref = _tiled_case("panda", N)
    assert len(marks) >= 8
    dG = _dev(torch, G)[0]
    # a loss that uses only frames 2 and 5
    a = _grad_q(torch, q)
    F = ets.link_frames(a, marks)
    (F[:, [2, 5]] * dG[:, [2, 5]]).sum().backward()
    spec = cases.CASES["panda"][0]
    want = cases.tiled(cases.oracle_gq(spec, [marks[2], marks[5]], cases.case("panda")[3], cases.case("panda")[4][:, [2, 5]]), N)
    assert _err(a.grad, want) <= cases.BOUND
    # a .sum() loss: the incoming gradient is an expanded scalar
    b = _grad_q(torch, q)
    ets.link_frames(b, marks).sum().backward()
    ones = np.ones((cases.ROWS, len(marks), 4, 4))
    assert _err(b.grad, cases.tiled(cases.oracle_gq(spec, marks, cases.case("panda")[3], ones), N)) <= cases.BOUND
    # one configuration, 1-D
    one = _grad_q(torch, q[3])
    F1 = ets.link_frames(one, marks)
    assert tuple(F1.shape) == (len(marks), 4, 4)
    (F1 * dG[3]).sum().backward()
    assert tuple(one.grad.shape) == (7,) and _err(one.grad, ref[3]) <= cases.BOUND
    # rows wider than the chain reads: the surplus columns get zeros
    wide = _grad_q(torch, np.concatenate([q, np.ones((N, 2))], axis=1))
    (ets.link_frames(wide, marks) * dG).sum().backward()
    assert _err(wide.grad[:, :7], ref) <= cases.BOUND and not bool(wide.grad[:, 7:].any())
    # a side stream
    c = _grad_q(torch, q)
    (ets.link_frames(c, marks) * dG).sum().backward()
    torch.cuda.synchronize()
    want = c.grad.clone()
    c.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (ets.link_frames(c, marks) * dG).sum().backward()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(c.grad, want) and _err(want, ref) <= cases.BOUND
    # no_grad and plain tensors: the ordinary call, the same bits
    with torch.no_grad():
        F0 = ets.link_frames(c, marks)
    assert F0.grad_fn is None and not F0.requires_grad and torch.equal(F0, F.detach())
    # float32 rows are refused as they were
    with pytest.raises(TypeError):
        ets.link_frames(c.detach().float().requires_grad_(True), marks)


def _fkine_all_check(torch, robot, spec, cols, marks, n, N, seed):
    """fkine_all of a serial robot on a grad-requiring q against the oracle; forward bits equal to the detached call"""
    rng = np.random.default_rng(seed)
    q, G = rng.uniform(-3, 3, (N, n)), rng.uniform(-1, 1, (N, len(marks), 4, 4))
    a = _grad_q(torch, q)
    F = robot.fkine_all(a)
    assert tuple(F.shape) == (N, len(marks), 4, 4) and F.grad_fn is not None and torch.equal(F, robot.fkine_all(a.detach()))
    (F * _dev(torch, G)[0]).sum().backward()
    err = _err(a.grad, cases.oracle_gq(spec, marks, q, G, None, cols, n))
    print("fkine_all backward %s: err %.3e" % (type(robot).__name__, err))
    assert err <= cases.BOUND


@gpu
def test_dh_and_model_robots_back_propagate_through_fkine_all():
    torch = _torch()
    puma = rtbhip.models.DH.Puma560()
    spec, cols = cases.spec_from_ets(puma.ets())
    k = 1 if (puma.base is not None and not np.array_equal(puma.base, np.eye(4))) else 0
    marks = [k]
    for l in puma.links:
        k += len(l.ets())
        marks.append(k)
    _fkine_all_check(torch, puma, spec, cols, marks, 6, 65, 11)
    panda = rtbhip.models.Panda()
    _fkine_all_check(torch, panda, cases.CASES["panda"][0], None, cases.PANDA_MARKS, 7, 65, 12)


def _y_robot():
    """a 2-joint trunk that forks into two 1-joint leaves"""
    from rtbhip.erobot import ERobot, Link
    ET = rtbhip.ET
    l0 = Link(ets=ET.tz(0.3) * ET.Rz(), name="t0")
    l1 = Link(ets=ET.tx(0.2) * ET.Rx(0.4) * ET.Ry(flip=True), parent=l0, name="t1")
    la = Link(ets=ET.ty(0.25) * ET.Rz(0.3) * ET.Rx(), parent=l1, name="a")
    lb = Link(ets=ET.tx(-0.15) * ET.Ry(-0.6) * ET.tz(), parent=l1, name="b")
    return ERobot([l0, l1, la, lb], name="y")


@gpu
def test_a_forked_robot_sums_the_trunk_over_both_leaves(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    er = _y_robot()
    assert er.n == 4 and sum(1 for l in er.links if not l.children) == 2
    N = 65
    rng = np.random.default_rng(21)
    q, G = rng.uniform(-3, 3, (N, er.n)), rng.uniform(-1, 1, (N, len(er.links) + 1, 4, 4))
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "vjp" not in name:
                return fn

            def call(*args):
                seen.append(name)
                return fn(*args)
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    a = _grad_q(torch, q)
    F = er.fkine_all(a)
    assert F.grad_fn is not None and torch.equal(F, er.fkine_all(a.detach()))
    (F * _dev(torch, G)[0]).sum().backward()
    assert seen == [VJP, VJP]                                      # one backward launch per leaf path; autograd adds the trunk's two contributions
    ref = cases.oracle_fkine_all(er, q, G)
    assert _err(a.grad, ref) <= cases.BOUND
    # the trunk joints' gradients are the sum over both leaves: a loss on one leaf's frame alone gives a different trunk gradient
    trunk = sorted({int(j) for l in er.links if l.children for j in er.ets(end=l).jindices})
    b = _grad_q(torch, q)
    leaf = next(l for l in er.links if not l.children)
    (er.fkine_all(b)[:, leaf.number] * _dev(torch, G)[0][:, leaf.number]).sum().backward()
    assert float((a.grad[:, trunk] - b.grad[:, trunk]).abs().max()) > 1e-3


@gpu
def test_urdf_fkine_all_back_propagates():
    torch = _torch()
    ur = rtbhip.urdf.load("UR5")
    er = ur.erobot()
    N = 65
    rng = np.random.default_rng(22)
    q, G = rng.uniform(-3, 3, (N, er.n)), rng.uniform(-1, 1, (N, len(er.links) + 1, 4, 4))
    a = _grad_q(torch, q)
    F = ur.fkine_all(a)
    assert F.grad_fn is not None and torch.equal(F, ur.fkine_all(a.detach()))
    (F * _dev(torch, G)[0]).sum().backward()
    err = _err(a.grad, cases.oracle_fkine_all(er, q, G))
    print("URDF UR5 fkine_all backward: err %.3e" % err)
    assert err <= cases.BOUND
