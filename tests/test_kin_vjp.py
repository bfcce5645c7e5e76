"""Differentiable fkine / jacob0: rtbhip_fkine_jacob_vjp, rtbhip_fkine_jacob_vjp_f32, rtbhip_kin_vjp_from_jacobian and rtbhip/autograd.py.

The oracle is the compiled reference restated in oracle/ (oracle.fkine, oracle.jacob0, oracle.hessian0, as tests/test_00_gpu_parity.py and
tests/test_diff_kinematics.py use them), contracted in NumPy:

    gq[i,k] = sum_rc gJ[i,r,c] H[i,k,r,c]  +  sum (B_R^T gT[i])[:, :3] * ([w_k]x R[i])  +  (B_R^T gT[i])[:, 3] . v_k

with R the rotation of the reference's T (no base) and (v_k ; w_k) column k of the reference's J.  Bound: the project's kinematics criterion,
1e-10 absolute (README rows a1-a6), with gT and gJ drawn from U(-1, 1).  float32: the f32 commit's rule, f32_call(x32) == fp64_call(x32.double()).float()
bit for bit.  gradcheck: torch's default tolerances.

No GPU is needed for the exports, the refusals of the raw ABI and the front end's routing (a stand-in for a CUDA tensor, as in tests/test_f32_io.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import product_ets, tool_base, chain_from_ets, mixed_spec, replaying

OK, EINVAL, ELIMIT = 0, -1, -3
HOST, DEV = 0, 1
BAD = 987654321
KIN_REG_MAX = 10          # csrc/kin_reg.h kKinRegMax: up to here the fused register tile, beyond it forward launch + k_vjp_from_jac_any
VJP = ("rtbhip_fkine_jacob_vjp", "rtbhip_fkine_jacob_vjp_f32", "rtbhip_kin_vjp_from_jacobian")


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbols_are_exported_and_declared():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtbhip.h")).read()
    for name in VJP:
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES and ("int %s(" % name) in hdr


class _Ctx:
    def __init__(self):
        self._keep = rtbhip.models.Panda().ets()
        self.c = self._keep._handle()
        self._buf = np.zeros(4096)
        self.B = self._buf.ctypes.data


# chain forms: (handle, q, N, base, tool, gT, gJ, gq, mem, stream); from_jacobian: (T, J, gT, gJ, N, n, gq, mem, stream)
_NOTHING = "gT and gJ are both NULL: there is nothing to differentiate"
_F32 = "fkine_jacob_vjp_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)"
ROWS = []
for _name, _mem in (("fkine_jacob_vjp", HOST), ("fkine_jacob_vjp_f32", DEV)):
    _add = lambda tag, g, want, _name=_name: ROWS.append((_name + "-" + tag, "rtbhip_" + _name, g, want))
    _p = _name + ": "
    _add("unknown", lambda x, m=_mem: (BAD, x.B, 4, None, None, x.B, x.B, x.B, m, None), (EINVAL, _p + "unknown chain handle"))
    _add("nullq", lambda x, m=_mem: (x.c, None, 4, None, None, x.B, x.B, x.B, m, None), (EINVAL, _p + "NULL input with N > 0"))
    _add("nullgq", lambda x, m=_mem: (x.c, x.B, 4, None, None, x.B, x.B, None, m, None), (EINVAL, _p + "NULL gq"))
    _add("nothing", lambda x, m=_mem: (x.c, x.B, 4, None, None, None, None, x.B, m, None), (EINVAL, _p + _NOTHING))
    _add("negN", lambda x, m=_mem: (x.c, x.B, -1, None, None, x.B, x.B, x.B, m, None), (EINVAL, _p + "negative N"))
    _add("mem7", lambda x: (x.c, x.B, 4, None, None, x.B, x.B, x.B, 7, None), (EINVAL, _p + "bad mem kind"))
    _add("unknown+negN", lambda x, m=_mem: (BAD, x.B, -1, None, None, x.B, x.B, x.B, m, None), (EINVAL, _p + "unknown chain handle"))
    _add("nullgq+nothing", lambda x, m=_mem: (x.c, x.B, 4, None, None, None, None, None, m, None), (EINVAL, _p + "NULL gq"))
    _add("empty", lambda x, m=_mem: (x.c, x.B, 0, None, None, x.B, x.B, x.B, m, None), (OK, None))
    _add("empty-null", lambda x, m=_mem: (x.c, None, 0, None, None, None, None, None, m, None), (OK, None))
ROWS.append(("fkine_jacob_vjp_f32-hostmem", "rtbhip_fkine_jacob_vjp_f32", lambda x: (x.c, x.B, 4, None, None, x.B, x.B, x.B, HOST, None), (EINVAL, _F32)))
ROWS.append(("fkine_jacob_vjp_f32-hostmem-empty", "rtbhip_fkine_jacob_vjp_f32", lambda x: (x.c, x.B, 0, None, None, x.B, x.B, x.B, HOST, None), (EINVAL, _F32)))
_add = lambda tag, g, want: ROWS.append(("kin_vjp_from_jacobian-" + tag, "rtbhip_kin_vjp_from_jacobian", g, want))
_p = "kin_vjp_from_jacobian: "
_add("nullJ", lambda x: (x.B, None, x.B, x.B, 4, 7, x.B, HOST, None), (EINVAL, _p + "NULL input with N > 0"))
_add("negN", lambda x: (x.B, x.B, x.B, x.B, -1, 7, x.B, HOST, None), (EINVAL, _p + "negative N"))
_add("mem7", lambda x: (x.B, x.B, x.B, x.B, 4, 7, x.B, 7, None), (EINVAL, _p + "bad mem kind"))
_add("n33", lambda x: (x.B, x.B, x.B, x.B, 4, 33, x.B, HOST, None), (ELIMIT, _p + "n must be 1..RTBHIP_MAX_JOINTS"))
_add("n0", lambda x: (x.B, x.B, x.B, x.B, 4, 0, x.B, HOST, None), (ELIMIT, _p + "n must be 1..RTBHIP_MAX_JOINTS"))
_add("nullgq", lambda x: (x.B, x.B, x.B, x.B, 4, 7, None, HOST, None), (EINVAL, _p + "NULL gq"))
_add("nothing", lambda x: (x.B, x.B, None, None, 4, 7, x.B, HOST, None), (EINVAL, _p + _NOTHING))
_add("gT-without-T", lambda x: (None, x.B, x.B, None, 4, 7, x.B, HOST, None), (EINVAL, _p + "gT needs T"))
_add("n33+nullgq", lambda x: (x.B, x.B, x.B, x.B, 4, 33, None, HOST, None), (ELIMIT, _p + "n must be 1..RTBHIP_MAX_JOINTS"))
_add("empty", lambda x: (x.B, x.B, x.B, x.B, 0, 7, x.B, HOST, None), (OK, None))
_add("empty-dev-null", lambda x: (None, None, None, None, 0, 7, None, DEV, None), (OK, None))


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,fn,make,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, fn, make, want):
    rc = getattr(_lib.lib(), fn)(*make(ctx))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want


def test_the_rows_name_every_vjp_entry_point():
    """the census tests/test_api_refusals.py keeps for the other compute entry points, for these three (rtbhip/_lib.py: _sp)"""
    mine = {n for n, (_, a) in _lib.SIGNATURES.items() if a and a[-1] is _lib._sp}
    assert mine == set(VJP)
    assert all(a[-2] == _lib._i32 for n, (_, a) in _lib.SIGNATURES.items() if n in mine)
    assert mine <= {fn for _, fn, _, want in ROWS if want[0] == OK} and mine <= {fn for _, fn, _, want in ROWS if want[0] != OK}
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_chain_without_joints_is_refused():
    e = rtbhip.ET.tx(0.5) * rtbhip.ET.Rx(0.25)
    buf = np.zeros(64)
    B = buf.ctypes.data
    assert _lib.lib().rtbhip_fkine_jacob_vjp(e._handle(), B, 2, None, None, B, None, B, HOST, None) == EINVAL
    assert _lib.lib().rtbhip_last_error().decode() == "fkine_jacob_vjp: chain has no joints"


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


def _calls(robot):
    ets = robot.ets()
    return {"eval": ets.eval, "fkine": ets.fkine, "jacob0": ets.jacob0, "fkine_jacob0": ets.fkine_jacob0, "robot.fkine": robot.fkine, "robot.jacob0": robot.jacob0}


def test_routing_with_a_stand_in_tensor(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    seen = []
    monkeypatch.setattr(rtbhip.autograd, "differentiable", lambda ets, what, q, base, tool: seen.append(what) or "routed")
    panda = rtbhip.models.Panda()
    want = {"eval": "T", "fkine": "T", "jacob0": "J", "fkine_jacob0": "TJ", "robot.fkine": "T", "robot.jacob0": "J"}
    for name, call in _calls(panda).items():
        del seen[:]
        assert call(_fake_cuda(torch, (5, 7), True)) == "routed" and seen == [want[name]], name
        # requires_grad without enabled gradients, and a plain tensor with them: the ordinary entry point, as before
        del seen[:]
        with torch.no_grad(), pytest.raises(_Ordinary):
            call(_fake_cuda(torch, (5, 7), True))
        with pytest.raises(_Ordinary):
            call(_fake_cuda(torch, (5, 7), False))
        assert not seen, name
    # the forms that stay non-differentiable take the ordinary path whatever q asks for
    ets = panda.ets()
    for call in (ets.jacobe, lambda q: ets.fkine_jacob0(q, frame=1), lambda q: ets.fkine_jacob0(q, packed=True), ets.hessian0):
        with pytest.raises(_Ordinary):
            call(_fake_cuda(torch, (5, 7), True))
    assert not seen


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the vector-Jacobian products run on the device only: not served by the CPU replay")(f))


def _chain(n):
    spec = []
    for j in range(n):
        spec.append((("Rz", "Ry", "tz", "Rx")[j % 4], None, j % 5 == 1))
        spec.append((("tx", "tz", "ty")[j % 3], 0.2 + 0.03 * j))
    return product_ets(spec)


CHAINS = {          # name -> (ets, tool, base)
    "n1": lambda: (_chain(1), None, None),
    "n2": lambda: (_chain(2), None, None),
    "panda": lambda: (rtbhip.models.Panda().ets(), None, None),
    "regmax": lambda: (_chain(KIN_REG_MAX), None, None),
    "regmax+1": lambda: (_chain(KIN_REG_MAX + 1),) + tuple(tool_base()),
    "n20": lambda: (_chain(20), None, None),
    "mixed": lambda: (product_ets(mixed_spec()),) + tuple(tool_base()),
    "panda+tool+base": lambda: (rtbhip.models.Panda().ets(),) + tuple(tool_base()),
}
SIZES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def _chain_of(name):
    return CHAINS[name]()


def _oracle_gq(ets, q, tool, base, gT, gJ):
    """(pose term, Jacobian term) of gq from the reference's T, J and H"""
    from oracle import oracle
    ch = chain_from_ets(ets)
    T, J, H = oracle.fkine(ch, q, tool=tool), oracle.jacob0(ch, q, tool=tool), oracle.hessian0(ch, q, tool=tool)
    gP = gT[:, :3, :] if base is None else np.einsum("ri,nrc->nic", base[:3, :3], gT[:, :3, :])
    w = J[:, 3:, :]                                                        # (N, 3, n)
    dR = np.cross(w.transpose(0, 2, 1)[:, :, None, :], T[:, None, :3, :3].transpose(0, 1, 3, 2)).transpose(0, 1, 3, 2)      # [w_k]x R: (N, n, 3, 3)
    pose = np.einsum("nrc,nkrc->nk", gP[:, :, :3], dR) + np.einsum("nr,nrk->nk", gP[:, :, 3], J[:, :3, :])
    return pose, np.einsum("nrc,nkrc->nk", gJ, H)


@functools.lru_cache(maxsize=None)
def _case(name, N):
    """inputs and the oracle's answers for one (chain, N): computed once, shared, never written to"""
    ets, tool, base = _chain_of(name)
    rng = np.random.default_rng(1000 * N + len(name))
    q = rng.uniform(-3, 3, (N, ets.n))
    gT, gJ = rng.uniform(-1, 1, (N, 4, 4)), rng.uniform(-1, 1, (N, 6, ets.n))
    pose, jac = _oracle_gq(ets, q, tool, base, gT, gJ)
    for a in (q, gT, gJ, pose, jac):
        a.setflags(write=False)
    return q, gT, gJ, pose, jac


def _ptr(x):
    return None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data_as(C.c_void_p))


def _vjp(ets, q, gT, gJ, tool=None, base=None):
    """rtbhip_fkine_jacob_vjp(_f32) on device tensors (or host arrays) of one dtype -> gq"""
    host = isinstance(q, np.ndarray)
    if host:
        gq = np.full(q.shape, np.nan)
        fn, mem, stream = _lib.lib().rtbhip_fkine_jacob_vjp, HOST, None
    else:
        torch = _torch()
        gq = torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device)
        fn = _lib.lib().rtbhip_fkine_jacob_vjp_f32 if q.dtype == torch.float32 else _lib.lib().rtbhip_fkine_jacob_vjp
        mem, stream = DEV, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    b, t = _lib.small(base, 16), _lib.small(tool, 16)
    _lib.check(fn(ets._handle(), _ptr(q), q.shape[0], _lib.host_ptr(b), _lib.host_ptr(t), _ptr(gT), _ptr(gJ), _ptr(gq), mem, stream))
    return gq


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


OBSERVED = {}        # the largest deviations from the oracle seen by this run (printed by the last oracle test's teardown)


@gpu
@pytest.mark.parametrize("name", sorted(CHAINS))
@pytest.mark.parametrize("N", SIZES)
def test_gq_equals_the_oracle(name, N):
    torch = _torch()
    ets, tool, base = _chain_of(name)
    q, gT, gJ, pose, jac = _case(name, N)
    dq, dgT, dgJ = _dev(torch, q, gT, gJ)
    for mode, got, ref in (("gT", _vjp(ets, dq, dgT, None, tool, base), pose), ("gJ", _vjp(ets, dq, None, dgJ, tool, base), jac),
                           ("both", _vjp(ets, dq, dgT, dgJ, tool, base), pose + jac)):
        err = float(np.abs(got.cpu().numpy() - ref).max())
        OBSERVED[mode] = max(OBSERVED.get(mode, 0.0), err)
        print("kin_vjp %s N=%d %s: max |gq - oracle| = %.3e" % (name, N, mode, err))
        assert err <= 1e-10, (name, N, mode, err)


@gpu
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_from_jacobian_agrees_with_the_chain_call(name):
    """the library's own T and J (no base: the pure-function form has none) through rtbhip_kin_vjp_from_jacobian"""
    torch = _torch()
    ets, tool, _ = _chain_of(name)
    N = 129
    q, gT, gJ, _, _ = _case(name, N)
    dq, dgT, dgJ = _dev(torch, q, gT, gJ)
    T, J = ets.fkine_jacob0(dq, tool=tool)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for a, b in ((dgT, None), (None, dgJ), (dgT, dgJ)):
        got = torch.full((N, ets.n), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().rtbhip_kin_vjp_from_jacobian(_ptr(T if a is not None else None), _ptr(J), _ptr(a), _ptr(b), N, ets.n, _ptr(got), DEV, stream))
        want = _vjp(ets, dq, a, b, tool, None)
        if ets.n > KIN_REG_MAX:
            assert torch.equal(got, want)              # the chain call IS this kernel on that T and J
        else:
            assert float((got - want).abs().max()) <= 1e-10


@gpu
@pytest.mark.parametrize("name", ["panda+tool+base", "regmax+1"])
@pytest.mark.parametrize("N", [1, 65])
def test_host_memory_call_is_bit_equal(name, N):
    torch = _torch()
    ets, tool, base = _chain_of(name)
    q, gT, gJ, _, _ = _case(name, N)
    dq, dgT, dgJ = _dev(torch, q, gT, gJ)
    for a, b in ((0, None), (None, 0), (0, 0)):
        host = _vjp(ets, q.copy(), None if a is None else gT.copy(), None if b is None else gJ.copy(), tool, base)
        dev = _vjp(ets, dq, None if a is None else dgT, None if b is None else dgJ, tool, base)
        assert np.array_equal(host, dev.cpu().numpy())
    T = ets.eval(q, tool=tool)
    J = ets.jacob0(q, tool=tool)
    got = np.full((N, ets.n), np.nan)
    _lib.check(_lib.lib().rtbhip_kin_vjp_from_jacobian(_ptr(np.ascontiguousarray(T.reshape(N, 16))), _ptr(np.ascontiguousarray(J.reshape(N, 6 * ets.n))),
                                                       _ptr(gT.copy()), _ptr(gJ.copy()), N, ets.n, _ptr(got), HOST, None))
    dT, dJ = _dev(torch, T.reshape(N, 16), J.reshape(N, 6 * ets.n))
    dgot = torch.full((N, ets.n), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().rtbhip_kin_vjp_from_jacobian(_ptr(dT), _ptr(dJ), _ptr(dgT), _ptr(dgJ), N, ets.n, _ptr(dgot), DEV, None))
    torch.cuda.synchronize()
    assert np.array_equal(got, dgot.cpu().numpy())


@gpu
def test_wider_q_rows_get_zero_columns():
    """a chain that reads columns 2 and 0 of a three-column q (a branch of a tree robot on the robot-wide q): column 1 of gq is written as zero"""
    torch = _torch()
    ET = rtbhip.ET
    wide = ET.Rz(jindex=2) * ET.tx(1.0) * ET.Ry(jindex=0) * ET.tz(0.3)
    narrow = ET.Rz(jindex=1) * ET.tx(1.0) * ET.Ry(jindex=0) * ET.tz(0.3)
    rng = np.random.default_rng(5)
    N = 65
    q = rng.uniform(-3, 3, (N, 3))
    gT, gJ = rng.uniform(-1, 1, (N, 4, 4)), rng.uniform(-1, 1, (N, 6, 2))
    dq, dgT, dgJ = _dev(torch, q, gT, gJ)
    got = _vjp(wide, dq, dgT, dgJ)
    ref = _vjp(narrow, dq[:, [0, 2]].contiguous(), dgT, dgJ)
    assert torch.equal(got[:, 1], torch.zeros(N, dtype=torch.float64, device="cuda"))
    assert torch.equal(got[:, 0], ref[:, 0]) and torch.equal(got[:, 2], ref[:, 1])


@gpu
@pytest.mark.parametrize("name", ["panda+tool+base", "mixed", "n20"])
@pytest.mark.parametrize("N", [65, 129])
def test_f32_equals_rounded_fp64(name, N):
    torch = _torch()
    ets, tool, base = _chain_of(name)
    q, gT, gJ, _, _ = _case(name, N)
    q32, gT32, gJ32 = [x.float() for x in _dev(torch, q, gT, gJ)]

    def misaligned(x):
        flat = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
        v = flat[1:].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for views in (False, True):
        a, b, c = (misaligned(q32), misaligned(gT32), misaligned(gJ32)) if views else (q32, gT32, gJ32)
        for u, v in ((b, None), (None, c), (b, c)):
            got = _vjp(ets, a, u, v, tool, base)
            want = _vjp(ets, q32.double(), None if u is None else gT32.double(), None if v is None else gJ32.double(), tool, base)
            assert got.dtype == torch.float32 and torch.equal(got, want.float())


# ---- autograd end to end
def _panda_case(torch, N=3, seed=3):
    ets = rtbhip.models.Panda().ets()
    tool, base = tool_base()
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = (6.0 * torch.rand((N, 7), generator=g, dtype=torch.float64) - 3.0).cuda().requires_grad_(True)
    return ets, tool, base, q


@gpu
@pytest.mark.parametrize("what", ["fkine", "jacob0", "fkine_jacob0"])
def test_gradcheck(what):
    torch = _torch()
    ets, tool, base, q = _panda_case(torch)
    f = {"fkine": lambda x: ets.fkine(x, base=base, tool=tool), "jacob0": lambda x: ets.jacob0(x, tool=tool),
         "fkine_jacob0": lambda x: ets.fkine_jacob0(x, base=base, tool=tool)}[what]
    out = f(q)
    assert all(o.grad_fn is not None for o in (out if isinstance(out, tuple) else (out,)))
    assert torch.autograd.gradcheck(f, (q,))


@gpu
def test_one_backward_launch_serves_both_outputs(monkeypatch):
    torch = _torch()
    import rtbhip.autograd
    ets, tool, base, q = _panda_case(torch, N=129)
    real, seen = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "vjp" not in name:
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((name, _lib.last_launch()))          # on the thread the backward runs on
                return rc
            return call

    monkeypatch.setattr(rtbhip.autograd, "lib", lambda: Counting())
    T, J = ets.fkine_jacob0(q, base=base, tool=tool)
    assert T.grad_fn is not None and T.grad_fn is J.grad_fn
    loss = (T * T).sum() + (J * J).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [("rtbhip_fkine_jacob_vjp", (3, 64, 32 * 43 * 8))]          # three tiles of 64 rows; LDS = reg_lds_doubles(7) doubles
    gq = _vjp(ets, q.detach(), (2 * T).detach().contiguous(), (2 * J).detach().contiguous(), tool, base)
    assert torch.equal(q.grad, gq)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


@gpu
def test_no_grad_path_is_unchanged_and_streams_are_honoured():
    torch = _torch()
    ets, tool, base, q = _panda_case(torch, N=65)
    T, J = ets.fkine_jacob0(q, base=base, tool=tool)
    plain = q.detach()
    with torch.no_grad():
        T0, J0 = ets.fkine_jacob0(q, base=base, tool=tool)
        E0 = ets.eval(q, base=base, tool=tool)
    T1, J1 = ets.fkine_jacob0(plain, base=base, tool=tool)
    for a in (T0, J0, E0, T1, J1, ets.jacob0(plain, tool=tool)):
        assert a.grad_fn is None and not a.requires_grad
    assert torch.equal(T, T0) and torch.equal(J, J0) and torch.equal(T, T1) and torch.equal(J, J1) and torch.equal(E0, T0)
    assert torch.equal(ets.eval(q, base=base, tool=tool), T) and torch.equal(ets.jacob0(q, tool=tool), ets.jacob0(plain, tool=tool))
    w = torch.linspace(-1, 1, 65 * 16, dtype=torch.float64, device="cuda").reshape(65, 4, 4)
    (ets.eval(q, base=base, tool=tool) * w).sum().backward()
    torch.cuda.synchronize()
    want = q.grad.clone()
    q.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (ets.eval(q, base=base, tool=tool) * w).sum().backward()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(q.grad, want)


@gpu
def test_single_configuration_and_float32():
    torch = _torch()
    ets, tool, base, q = _panda_case(torch, N=2)
    one = q.detach()[0].clone().requires_grad_(True)
    T = ets.eval(one, base=base, tool=tool)
    assert tuple(T.shape) == (4, 4)
    T.sum().backward()
    ets.eval(q, base=base, tool=tool)[0].sum().backward()
    assert tuple(one.grad.shape) == (7,) and torch.equal(one.grad, q.grad[0])
    q32 = q.detach().float().requires_grad_(True)
    T32, J32 = ets.fkine_jacob0(q32, base=base, tool=tool)
    assert T32.dtype == torch.float32
    (T32.sum() + J32.sum()).backward()
    q64 = q32.detach().double().requires_grad_(True)
    T64, J64 = ets.fkine_jacob0(q64, base=base, tool=tool)
    (T64.sum() + J64.sum()).backward()
    assert q32.grad.dtype == torch.float32 and torch.equal(q32.grad, q64.grad.float())


@gpu
@pytest.mark.parametrize("kind", ["dh", "urdf"])
def test_robot_classes_back_propagate(kind):
    torch = _torch()
    robot = rtbhip.models.DH.Puma560() if kind == "dh" else rtbhip.urdf.load("Panda")
    ets = robot.ets()
    rng = np.random.default_rng(17)
    N = 5
    qn, gT = rng.uniform(-2, 2, (N, ets.n)), rng.uniform(-1, 1, (N, 4, 4))
    q = torch.from_numpy(qn).cuda().requires_grad_(True)
    T = robot.fkine(q)
    assert T.grad_fn is not None
    (torch.as_tensor(T) * torch.from_numpy(gT).cuda()).sum().backward()
    base = getattr(robot, "base", None) if kind == "urdf" else None
    base = None if base is None else np.asarray(getattr(base, "A", base), dtype=np.float64)
    pose, _ = _oracle_gq(ets, qn, None, base, gT, np.zeros((N, 6, ets.n)))
    assert float(np.abs(q.grad.cpu().numpy() - pose).max()) <= 1e-10
    J = robot.jacob0(q.detach().requires_grad_(True))
    assert J.grad_fn is not None
