"""float32 device tensors in, float32 tensors out: ETS fkine / eval, jacob0, jacobe, fkine_jacob0 (two arrays, packed, out=) and DHRobot.rne.

The float32 entry points (rtbhip_fkine_jacob_f32, rtbhip_fkine_jacob_packed_f32, rtbhip_rne_f32) share the fp64 kernels' bodies: a float is widened
after its load, the arithmetic is fp64, a result is rounded once before its store.  A float32 value is exactly representable in fp64, so

    f32_call(q32)  ==  fp64_call(q32.double()).float()          bit for bit (torch.equal)

against the fp64 kernel of the same dispatch class.  Every kinematics size takes the same class in both forms (1..10 joints the register tile,
longer chains the run-time-n tile).  DHRobot.rne: the Panda and the Puma560 take their built-in structure instantiation in both forms; any other
all-revolute table of up to 8 links would take a kernel compiled at run time in fp64, which float32 does not have -- there the fp64 side is put on
the general kernel with rtbhip.tune("rne_sig", 0) (the run-time instantiations are bit-equal to it by tests/test_jit_gpu.py).  No size needs the
one-ulp fallback bound.  The fp64 results themselves are pinned on the oracle by the existing tests; one chain is checked against the oracle
directly here with 2^-24 |x| + 1e-10 (half an ulp of the final rounding plus the project's 1e-10 contract).

The dtype rules (mixed element types, out= of another type, half / integer tensors, methods without a float32 entry point) are checked on a
stand-in for a CUDA tensor whose data pointer raises: they need no GPU, and they prove the refusal happens before anything could be launched."""
import numpy as np
import pytest

import rtbhip
from helpers import product_ets, tool_base, chain_from_ets, replaying

SIZES = (1, 63, 64, 65, 1000, 1000003)


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ dtype rules (no GPU)
class _Refused(AssertionError):
    pass


def _fake_cuda(dtype, shape):
    """what rtbhip takes for a CUDA tensor (is_torch: a type of a torch module with data_ptr) -- but nothing can be read through it"""
    class FakeCudaTensor:
        is_cuda = True

        def __init__(self):
            self.dtype, self.shape = dtype, tuple(shape)
            self.device = "cuda:0"

        def dim(self):
            return len(self.shape)

        def element_size(self):
            return _torch().empty(0, dtype=self.dtype).element_size()

        def data_ptr(self):
            raise _Refused("the tensor's pointer was asked for: the dtype check did not stop the call")

        def reshape(self, *a):
            raise _Refused("the tensor was reshaped: the dtype check did not stop the call")

        contiguous = detach = reshape

        def __getitem__(self, k):
            raise _Refused("the tensor was sliced: the dtype check did not stop the call")

    FakeCudaTensor.__module__ = "torch"
    return FakeCudaTensor()


DH_REFUSING = {                      # every dynamics method without a float32 entry point: name -> number of (N, n) arguments
    "inertia": 1, "coriolis": 2, "gravload": 1, "itorque": 2, "accel": 3,
}


@pytest.mark.parametrize("method", sorted(DH_REFUSING))
@pytest.mark.parametrize("dtype", ["float32", "float16", "int64"])
def test_dh_dynamics_methods_refuse_other_dtypes(method, dtype):
    torch = _torch()
    robot = rtbhip.models.DH.Puma560()
    args = [_fake_cuda(getattr(torch, dtype), (5, 6)) for _ in range(DH_REFUSING[method])]
    with pytest.raises(TypeError, match="float64"):
        getattr(robot, method)(*args)


def test_dh_rne_base_wrench_refuses_float32():
    torch = _torch()
    robot = rtbhip.models.DH.Puma560()
    a = [_fake_cuda(torch.float32, (5, 6)) for _ in range(3)]
    with pytest.raises(TypeError, match="float64"):
        robot.rne(*a, base_wrench=True)


@pytest.mark.parametrize("method,nargs", [("rne", 3), ("inertia", 1), ("coriolis", 2), ("gravload", 1), ("itorque", 2), ("accel", 3)])
def test_erobot_dynamics_methods_refuse_float32(method, nargs):
    torch = _torch()
    from test_erobot_rne import random_tree
    prod, _ = random_tree(np.random.default_rng(3), n_links=5)
    robot = rtbhip.ERobot(prod)
    n = robot.n
    args = [_fake_cuda(torch.float32, (5, n)) for _ in range(nargs)]
    with pytest.raises(TypeError, match="float64"):
        getattr(robot, method)(*args)


def test_dh_rne_mixed_dtypes_and_half():
    torch = _torch()
    robot = rtbhip.models.DH.Puma560()
    f32, f64, f16, bf16, i32 = (lambda: _fake_cuda(torch.float32, (5, 6))), (lambda: _fake_cuda(torch.float64, (5, 6))), \
        (lambda: _fake_cuda(torch.float16, (5, 6))), (lambda: _fake_cuda(torch.bfloat16, (5, 6))), (lambda: _fake_cuda(torch.int32, (5, 6)))
    for trio in ((f32(), f64(), f32()), (f64(), f32(), f64()), (f32(), f32(), f64())):
        with pytest.raises(TypeError, match="one dtype"):
            robot.rne(*trio)
    for bad in (f16, bf16, i32):
        with pytest.raises(TypeError, match=r"float64 or torch\.float32"):
            robot.rne(bad(), bad(), bad())


def test_ets_dtype_rules():
    torch = _torch()
    ets = rtbhip.models.Panda().ets()
    for dt in (torch.float16, torch.bfloat16, torch.int64):
        for call in (ets.eval, ets.fkine, ets.jacob0, ets.jacobe, ets.fkine_jacob0):
            with pytest.raises(TypeError, match=r"float64 or torch\.float32"):
                call(_fake_cuda(dt, (5, 7)))
    # methods without a float32 entry point keep refusing a float32 device q, with the message they always had
    q32 = lambda: _fake_cuda(torch.float32, (5, 7))
    for call in (ets.hessian0, ets.hessiane, lambda q: ets.jacob0_dot(q, q), lambda q: ets.manipulability(q), lambda q: ets.jacob0_analytical(q)):
        with pytest.raises(TypeError, match="^device q must be float64$"):
            call(q32())


def test_numpy_float32_keeps_host_behaviour_signature():
    """a host float32 array is converted to float64 on the host and float64 comes back (the reference does the same) -- checked where it needs
    no device: the shaping step"""
    ets = rtbhip.models.Panda().ets()
    q2, single, tm = ets._shape_q(np.zeros((3, 7), dtype=np.float32), f32_ok=True)
    assert q2.dtype == np.float64 and not tm and not single


# ------------------------------------------------------------------------------------------------ parity on the device
def gpu(f):
    """needs the device: the float32 entry points are device kernels (device memory only) -- the CPU replay of the GPU suite
    (tests/test_gpu_suite_on_cpu_replay.py) replays the fp64 host-buffer calls and has nothing to serve these with"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="float32 rows exist on the device only: not served by the CPU replay")(f))


def _q32(torch, N, n, seed, lo=-3.0, hi=3.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((hi - lo) * torch.rand((N, n), generator=g, dtype=torch.float32) + lo).cuda()


def _chain20():
    spec = []
    for j in range(20):
        spec.append((("Rz", "Ry", "Rx", "tz")[j % 4], None, j % 5 == 3))
        spec.append((("tx", "tz", "ty")[j % 3], 0.05 + 0.01 * j))
    return product_ets(spec)


def _chain(n):
    spec = []
    for j in range(n):
        spec.append((("Rz", "Ry", "tz")[j % 3], None, j == 1))
        spec.append(("tx", 0.2 + 0.1 * j))
    return product_ets(spec)


KIN_CHAINS = {
    "panda": lambda: rtbhip.models.Panda().ets(),
    "puma560": lambda: rtbhip.models.Puma560ETS().ets(),
    "twenty": _chain20,
    "one": lambda: _chain(1),
    "two": lambda: _chain(2),
    "three": lambda: _chain(3),
}


def _check_kin(torch, ets, q32, base=None, tool=None):
    """every float32 kinematics call of the table against float(fp64 call on the widened q)"""
    q64 = q32.double()
    N, n = q32.shape[0], ets.n
    T32, J32 = ets.fkine_jacob0(q32, base=base, tool=tool)
    T64, J64 = ets.fkine_jacob0(q64, base=base, tool=tool)
    assert T32.dtype == torch.float32 and J32.dtype == torch.float32 and T32.shape == T64.shape and J32.shape == J64.shape      # (N = 1 is ONE configuration: (4, 4) and (6, n))
    assert torch.equal(T32, T64.float()) and torch.equal(J32, J64.float())
    assert torch.equal(ets.eval(q32, base=base, tool=tool), ets.eval(q64, base=base, tool=tool).float())
    assert torch.equal(ets.jacob0(q32, tool=tool), ets.jacob0(q64, tool=tool).float())
    Je32 = ets.jacobe(q32, tool=tool)
    assert Je32.dtype == torch.float32 and torch.equal(Je32, ets.jacobe(q64, tool=tool).float())
    Tp, Jp, TJ = ets.fkine_jacob0(q32, base=base, tool=tool, packed=True)
    _, _, TJ64 = ets.fkine_jacob0(q64, base=base, tool=tool, packed=True)
    assert TJ.dtype == torch.float32 and TJ.shape == TJ64.shape
    assert torch.equal(TJ, TJ64.float()) and torch.equal(Tp, T32) and torch.equal(Jp, J32)
    out = torch.full((N, 16 + 6 * n), float("nan"), dtype=torch.float32, device=q32.device)
    _, _, TJo = ets.fkine_jacob0(q32, base=base, tool=tool, frame=1, packed=True, out=out)
    assert TJo.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any())
    _, _, TJe64 = ets.fkine_jacob0(q64, base=base, tool=tool, frame=1, packed=True)
    assert torch.equal(out.reshape(TJe64.shape), TJe64.float())


@gpu
@pytest.mark.parametrize("name", sorted(KIN_CHAINS))
@pytest.mark.parametrize("N", SIZES)
def test_kin_f32_equals_rounded_fp64(name, N):
    torch = _torch()
    ets = KIN_CHAINS[name]()
    _check_kin(torch, ets, _q32(torch, N, ets.n, 11 + N % 97))


@gpu
@pytest.mark.parametrize("name", ["panda", "twenty", "two"])
def test_kin_f32_base_and_tool(name):
    torch = _torch()
    ets = KIN_CHAINS[name]()
    tool, base = tool_base()
    _check_kin(torch, ets, _q32(torch, 1000, ets.n, 5), base=base, tool=tool)


@gpu
@pytest.mark.parametrize("name", ["panda", "twenty"])
def test_kin_f32_views(name):
    """a non-contiguous q, and an offset view whose base pointer is 4-byte but not 16-byte aligned"""
    torch = _torch()
    ets = KIN_CHAINS[name]()
    n, N = ets.n, 1000
    wide = _q32(torch, N, 2 * n, 3)
    _check_kin(torch, ets, wide[:, ::2])
    flat = torch.empty(N * n + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(N, n)
    view.copy_(_q32(torch, N, n, 4))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _check_kin(torch, ets, view)


@gpu
def test_kin_f32_out_must_match_q_dtype():
    torch = _torch()
    ets = KIN_CHAINS["panda"]()
    q32 = _q32(torch, 10, 7, 1)
    with pytest.raises(ValueError, match="float32"):
        ets.fkine_jacob0(q32, packed=True, out=torch.empty((10, 58), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="float64"):
        ets.fkine_jacob0(q32.double(), packed=True, out=torch.empty((10, 58), dtype=torch.float32, device="cuda"))


@gpu
def test_kin_f32_single_configuration_and_robot_level():
    torch = _torch()
    robot = rtbhip.models.Panda()
    q = _q32(torch, 1, 7, 2)[0]
    T = robot.ets().eval(q)
    assert T.dtype == torch.float32 and tuple(T.shape) == (4, 4) and torch.equal(T, robot.ets().eval(q.double()).float())
    qb = _q32(torch, 100, 7, 2)
    for nm in ("jacob0", "jacobe"):
        a, b = getattr(robot, nm)(qb), getattr(robot, nm)(qb.double())
        assert a.dtype == torch.float32 and torch.equal(a, b.float())
    a, b = robot.fkine(qb), robot.fkine(qb.double())
    assert torch.equal(torch.as_tensor(a), torch.as_tensor(b).float())


@gpu
def test_kin_f32_against_the_oracle():
    """Panda, straight against the CPU oracle in fp64: 2^-24 |x| (the final rounding) + 1e-10 (the project's contract)"""
    torch = _torch()
    from oracle import oracle
    ets = KIN_CHAINS["panda"]()
    ch = chain_from_ets(ets)
    q32 = _q32(torch, 1000, 7, 9)
    T, J = ets.fkine_jacob0(q32)
    q = q32.double().cpu().numpy()
    for got, ref in ((T, oracle.fkine(ch, q)), (J, oracle.jacob0(ch, q))):
        got = got.double().cpu().numpy()
        assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-10), float(np.abs(got - ref).max())


@gpu
def test_fp64_path_unchanged_across_routes():
    """the fp64 calls return the same bits whichever route serves them (built-in structure instantiation or not), as before"""
    torch = _torch()
    ets, dh = KIN_CHAINS["panda"](), rtbhip.models.DH.Panda()
    q = _q32(torch, 1000, 7, 21).double()
    qd, qdd = _q32(torch, 1000, 7, 22).double(), _q32(torch, 1000, 7, 23).double()
    try:
        T1, J1 = ets.fkine_jacob0(q)
        tau1 = dh.rne(q, qd, qdd)
        rtbhip.tune("sig_builtin", 0)
        rtbhip.tune("rne_sig", 0)
        T2, J2 = ets.fkine_jacob0(q)
        tau2 = dh.rne(q, qd, qdd)
    finally:
        rtbhip.tune("sig_builtin", 1)
        rtbhip.tune("rne_sig", 1)
    assert torch.equal(T1, T2) and torch.equal(J1, J2) and torch.equal(tau1, tau2)


# ---- DHRobot.rne
def _mdh3():
    from rtbhip.dh import DHRobot, RevoluteMDH
    L = [RevoluteMDH(a=0.1 * j, d=0.2, alpha=(0.0, -np.pi / 2, np.pi / 2)[j], m=1.0 + j, r=[0.01, 0.02 * j, 0.03], I=[0.1, 0.2, 0.3, 0.01, 0.02, 0.03], G=1)
         for j in range(3)]
    return DHRobot(L, name="mdh3")


def _dh12():
    from rtbhip.dh import DHRobot, RevoluteDH, PrismaticDH
    L = []
    for j in range(12):
        kw = dict(a=0.05 * (j % 3), alpha=(np.pi / 2, 0.0, -np.pi / 2)[j % 3], m=0.5 + 0.1 * j, r=[0.01, 0.0, 0.02], I=[0.05, 0.04, 0.03, 0, 0, 0], G=1)
        L.append(PrismaticDH(theta=0.1, **kw) if j % 5 == 4 else RevoluteDH(d=0.1, **kw))
    return DHRobot(L, name="dh12")


RNE_ROBOTS = {
    "panda": (lambda: rtbhip.models.DH.Panda(), False),          # built-in instantiation in both forms
    "puma560": (lambda: rtbhip.models.DH.Puma560(), False),      # built-in instantiation in both forms
    "mdh3": (_mdh3, True),                                       # fp64 would take a run-time instantiation: compared on the general kernel
    "dh12": (_dh12, False),                                      # run-time-n kernel in both forms
}


def _check_rne(torch, robot, general, N, seed, **kw):
    n = robot.n
    q, qd, qdd = _q32(torch, N, n, seed), _q32(torch, N, n, seed + 1, -1, 1), _q32(torch, N, n, seed + 2, -2, 2)
    tau32 = robot.rne(q, qd, qdd, **kw)
    assert tau32.dtype == torch.float32
    try:
        if general:
            rtbhip.tune("rne_sig", 0)
        tau64 = robot.rne(q.double(), qd.double(), qdd.double(), **kw)
    finally:
        rtbhip.tune("rne_sig", 1)
    assert tau32.shape == tau64.shape and torch.equal(tau32, tau64.float()), float((tau32.double() - tau64).abs().max())
    return q, qd, qdd, tau32


@gpu
@pytest.mark.parametrize("name", sorted(RNE_ROBOTS))
@pytest.mark.parametrize("N", SIZES)
def test_rne_f32_equals_rounded_fp64(name, N):
    torch = _torch()
    make, general = RNE_ROBOTS[name]
    _check_rne(torch, make(), general, N, 31 + N % 89)


@gpu
@pytest.mark.parametrize("name", sorted(RNE_ROBOTS))
def test_rne_f32_fext_gravity_and_views(name):
    torch = _torch()
    make, general = RNE_ROBOTS[name]
    robot = make()
    _check_rne(torch, robot, general, 1000, 7, fext=[1.0, -2.0, 3.0, 0.1, 0.2, -0.3])
    _check_rne(torch, robot, general, 1000, 8, gravity=[0.5, -1.0, 3.7])
    n, N = robot.n, 1000
    flat = torch.empty(N * n + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(N, n)
    view.copy_(_q32(torch, N, n, 12))
    wide = _q32(torch, N, 2 * n, 13, -1, 1)
    qdd = _q32(torch, N, n, 14)
    assert view.data_ptr() % 16 == 4
    a = robot.rne(view, wide[:, ::2], qdd)
    try:
        if general:
            rtbhip.tune("rne_sig", 0)
        b = robot.rne(view.double(), wide[:, ::2].double(), qdd.double())
    finally:
        rtbhip.tune("rne_sig", 1)
    assert torch.equal(a, b.float())


@gpu
def test_rne_f32_against_the_oracle():
    torch = _torch()
    from oracle import oracle, chains
    robot, tab = rtbhip.models.DH.Puma560(), chains.puma560()
    q, qd, qdd, tau = _check_rne(torch, robot, False, 500, 41)
    ref = oracle.rne_dh(tab.L24(), 0, q.double().cpu().numpy(), qd.double().cpu().numpy(), qdd.double().cpu().numpy(), -tab.gravity)
    got = tau.double().cpu().numpy()
    # (rne's contract is relative to the largest torque: smoke() and tests/test_00_gpu_parity.py use 1e-9 * max(1, |ref|max); here the tighter 1e-10)
    assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-10 * max(1.0, np.abs(ref).max())), float(np.abs(got - ref).max())


@gpu
def test_rne_f32_mixed_dtypes_on_the_device():
    torch = _torch()
    robot = rtbhip.models.DH.Panda()
    q = _q32(torch, 10, 7, 1)
    with pytest.raises(TypeError, match="one dtype"):
        robot.rne(q, q.double(), q)
    with pytest.raises(TypeError, match=r"float64 or torch\.float32"):
        robot.rne(q.half(), q.half(), q.half())
    with pytest.raises(TypeError, match="float64"):
        robot.inertia(q)
