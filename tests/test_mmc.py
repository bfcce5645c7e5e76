"""The reactive QP servo: rtbhip_mmc and rtbhip.servo (mmc, mmc_servo, joint_velocity_damper).

The oracle and its bounds are those of tests/mmc_cases.py: the definition of the header's comment in NumPy on the oracle's fkine / jacob0 / jacobe /
jacobm and p_servo's restated error, the QP by enumeration of the held sets with the full KKT system;  K eps c scale per row for the step,
K_LOOP eps cmax^2 amp max|q_ref| for the loop, K and K_LOOP from the CPU replay of the lane body (tests/test_mmc_emu.py).  arrived, its and
status must equal the oracle's exactly.  Every device test prints the largest ratio it sees beside the constant.

No GPU is needed for the exports, the refusals of the raw ABI, the census of the launcher's instantiations and joint_velocity_damper."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import replaying
import mmc_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
BAD = 987654321
FN = "rtbhip_mmc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = _lib.rtbhip_mmc_args


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
def test_symbol_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "rtbhip.h")).read()
    assert hasattr(_lib.lib(), FN) and FN in _lib.SIGNATURES and ("int %s(const rtbhip_mmc_args *args);" % FN) in hdr
    res, args = _lib.SIGNATURES[FN]
    assert res is C.c_int and len(args) == 1 and args[0]._type_ is ARGS          # ONE argument: the parameter block
    m = re.search(r"typedef struct rtbhip_mmc_args \{(.*?)\} rtbhip_mmc_args;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            rest = re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip(), count=1)
            names += [re.sub(r"[\s*]|\[\d+\]", "", x) for x in rest.split(",")]
    assert [n for n in names if n] == [f[0] for f in ARGS._fields_], names
    assert C.sizeof(ARGS) == 232 and ARGS.gain6.offset == 64 and ARGS.steps.offset == 128 and ARGS.stream.offset == 224


class _Ctx:
    def __init__(self):
        import link_frames_vjp_cases as fcases
        import ik_vjp_cases as ikc
        self._keep = (cases.model("panda").ets, fcases.ets_of("cols"), ikc.model("n11").ets, ikc.model("n5").ets)
        self.p, self.cols, self.n11, self.n5 = (e._handle() for e in self._keep)
        self._buf = np.zeros(8192)
        self.B = self._buf.ctypes.data
        self._lim = dict(nanlo=np.zeros(14), nanhi=np.zeros(14), nanv=np.ones(7), negv=np.ones(7))
        self._lim["nanlo"][2] = self._lim["nanhi"][7 + 4] = self._lim["nanv"][6] = np.nan
        self._lim["negv"][0] = -0.5
        for k, v in self._lim.items():
            setattr(self, k, v.ctypes.data)


def _block(x, **kw):
    """a valid block on the Panda (host addresses: a refusal and the empty batch never read the device arrays), then the named fields changed"""
    a = ARGS()
    a.size, a.method, a.chain, a.N, a.nTep = C.sizeof(ARGS), 1, x.p, 4, 4
    a.q, a.Tep, a.qlim, a.qdlim, a.qd, a.q_out, a.arrived, a.its, a.status = x.B, x.B, x.B, x.B, x.B, x.B, x.B, x.B, x.B
    a.gain6 = (C.c_double * 6)(1, 1, 1, 1, 1, 1)
    a.threshold, a.dt, a.steps = 0.1, 0.01, 1
    a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = 0.01, 1.0, 1.0, 0.05, 0.9, 1.0
    for k, v in kw.items():
        if k.startswith("gain"):
            a.gain6[int(k[4:])] = v
        else:
            setattr(a, k, getattr(x, v) if isinstance(v, str) else v)
    return a


_P = "mmc: "
_NULLIN, _FIN = _P + "NULL input with N > 0", _P + "gain6, threshold, dt, Y, ks, km, ps, pi and damper_gain must be finite"
_SIZE, _POS, _NANLIM = _P + "size is not sizeof(rtbhip_mmc_args): built against another header", _P + "Y and ks must be positive (the QP must be strictly convex)", _P + "NaN in qlim or qdlim"
NAN, INF = float("nan"), float("inf")
# (id, the fields changed, (return code, message))
ROWS = [
    ("null-block", None, (EINVAL, _P + "NULL parameter block")),
    ("size-small", dict(size=C.sizeof(ARGS) - 8), (EINVAL, _SIZE)),
    ("size-rrmc", dict(size=C.sizeof(_lib.rtbhip_rrmc_args)), (EINVAL, _SIZE)),
    ("unknown", dict(chain=BAD), (EINVAL, _P + "unknown chain handle")),
    ("negN", dict(N=-1, nTep=-1), (EINVAL, _P + "negative N")),
    ("nTep", dict(nTep=2), (EINVAL, _P + "nTep must be N or 1")),
    ("nTep-zero", dict(nTep=0), (EINVAL, _P + "nTep must be N or 1")),
    ("nullq", dict(q=None), (EINVAL, _NULLIN)),
    ("nullTep", dict(Tep=None), (EINVAL, _NULLIN)),
    ("nullqlim", dict(qlim=None), (EINVAL, _NULLIN)),
    ("nullboth", dict(qd=None, q_out=None), (EINVAL, _P + "qd and q_out are both NULL: there is nothing to compute")),
    ("jindex", dict(chain="cols"), (EINVAL, _P + "chain must use jindex 0..n-1")),
    ("method-2", dict(method=2), (EINVAL, _P + "method must be 0 angle-axis or 1 rpy")),
    ("method-neg", dict(method=-1), (EINVAL, _P + "method must be 0 angle-axis or 1 rpy")),
    ("Y-zero", dict(Y=0.0), (EINVAL, _POS)),
    ("Y-negative", dict(Y=-0.01), (EINVAL, _POS)),
    ("ks-zero", dict(ks=0.0), (EINVAL, _POS)),
    ("km-negative", dict(km=-1.0), (EINVAL, _P + "km must be >= 0")),
    ("ps-negative", dict(ps=-0.01), (EINVAL, _P + "ps must be >= 0")),
    ("pi-equals-ps", dict(pi=0.05), (EINVAL, _P + "pi must be above ps")),
    ("pi-below-ps", dict(pi=0.01), (EINVAL, _P + "pi must be above ps")),
    ("gain-nan", dict(gain3=NAN), (EINVAL, _FIN)),
    ("threshold-nan", dict(threshold=NAN), (EINVAL, _FIN)),
    ("dt-inf", dict(dt=-INF), (EINVAL, _FIN)),
    ("Y-nan", dict(Y=NAN), (EINVAL, _FIN)),
    ("ks-inf", dict(ks=INF), (EINVAL, _FIN)),
    ("km-nan", dict(km=NAN), (EINVAL, _FIN)),
    ("ps-nan", dict(ps=NAN), (EINVAL, _FIN)),
    ("pi-inf", dict(pi=INF), (EINVAL, _FIN)),
    ("damper-gain-nan", dict(damper_gain=NAN), (EINVAL, _FIN)),
    ("qlim-lo-nan", dict(qlim="nanlo"), (EINVAL, _NANLIM)),
    ("qlim-hi-nan", dict(qlim="nanhi"), (EINVAL, _NANLIM)),
    ("qdlim-nan", dict(qdlim="nanv"), (EINVAL, _NANLIM)),
    ("qdlim-negative", dict(qdlim="negv"), (EINVAL, _P + "qdlim must be >= 0")),
    ("steps-zero", dict(steps=0), (EINVAL, _P + "steps must be at least 1")),
    ("steps-negative", dict(steps=-3), (EINVAL, _P + "steps must be at least 1")),
    ("five-joints", dict(chain="n5"), (ELIMIT, _P + "chains of 6..10 joints")),
    ("eleven-joints", dict(chain="n11"), (ELIMIT, _P + "chains of 6..10 joints")),
    ("steps-4097", dict(steps=4097), (ELIMIT, _P + "at most 4096 steps")),
    ("too-many-tiles", dict(N=64 * 2 ** 31, nTep=1), (ELIMIT, _P + "batch too large for one launch")),
    ("too-many-tiles-int64-max", dict(N=2 ** 63 - 1, nTep=1), (ELIMIT, _P + "batch too large for one launch")),
    ("steps-4096-empty", dict(steps=4096, N=0, nTep=0), (OK, None)),
    ("empty", dict(N=0, nTep=0), (OK, None)),
    ("empty-one-tep", dict(N=0, nTep=1), (OK, None)),
    ("empty-null", dict(N=0, nTep=0, q=None, Tep=None, qlim=None, qdlim=None, qd=None, q_out=None, arrived=None, its=None, status=None), (OK, None)),
]
# the refusals the header's comment names (parentheses dropped) -> the rows that hold them
HEADER = {
    "a NULL block or a wrong size": ["null-block", "size-small", "size-rrmc"], "unknown chain handle": ["unknown"], "negative N": ["negN"],
    "nTep neither N nor 1": ["nTep", "nTep-zero"], "a NULL input with N > 0": ["nullq", "nullTep", "nullqlim"], "qd and q_out both NULL": ["nullboth"],
    "a chain whose jindex is not 0..n-1": ["jindex"], "a method that is not 0 or 1": ["method-2", "method-neg"],
    "a Y or ks that is not positive": ["Y-zero", "Y-negative", "ks-zero"], "a negative km": ["km-negative"], "a negative ps": ["ps-negative"],
    "a pi that is not above ps": ["pi-equals-ps", "pi-below-ps"],
    "a non-finite scalar": ["gain-nan", "threshold-nan", "dt-inf", "Y-nan", "ks-inf", "km-nan", "ps-nan", "pi-inf", "damper-gain-nan"],
    "a NaN in qlim or qdlim": ["qlim-lo-nan", "qlim-hi-nan", "qdlim-nan"], "a negative qdlim": ["qdlim-negative"],
    "steps below 1": ["steps-zero", "steps-negative"],
    "fewer than 6 or more than 10 joints": ["five-joints", "eleven-joints"], "more than 4096 steps": ["steps-4097"],
    "a batch beyond one launch's tiles": ["too-many-tiles", "too-many-tiles-int64-max"],
}


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.mark.parametrize("rid,fields,want", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, fields, want):
    ctx._buf[:] = 0.0
    rc = getattr(_lib.lib(), FN)(None) if fields is None else getattr(_lib.lib(), FN)(C.byref(_block(ctx, **fields)))
    assert (rc, _lib.lib().rtbhip_last_error().decode() if rc != 0 else None) == want
    assert not ctx._buf.any()                    # a refusal and the empty batch touch nothing


def test_every_refusal_the_header_names_has_a_row():
    hdr = open(os.path.join(ROOT, "include", "rtbhip.h")).read()
    end = hdr.index("typedef struct rtbhip_mmc_args")
    comment = " ".join(l.strip(" *") for l in hdr[hdr.rindex("/*", 0, end):end].splitlines())
    comment = re.sub(r"\([^)]*\)", "", comment)
    m = re.search(r"RTBHIP_EINVAL: (.*?)\.\s+RTBHIP_ELIMIT: (.*?)\.", comment)
    assert m, comment
    named = [re.sub(r"\s+", " ", x).strip() for part in m.groups() for x in part.split(",")]
    assert sorted(named) == sorted(HEADER), named
    ids = {r[0] for r in ROWS}
    assert len(ids) == len(ROWS) and all(set(v) <= ids for v in HEADER.values())
    assert {r[0] for r in ROWS if r[2][0] != OK} == {i for v in HEADER.values() for i in v}
    limits = HEADER["fewer than 6 or more than 10 joints"] + HEADER["more than 4096 steps"] + HEADER["a batch beyond one launch's tiles"]
    assert {r[0] for r in ROWS if r[2][0] == ELIMIT} == set(limits)


# ------------------------------------------------------------------------------------------------ census (no GPU)
CENSUS = {6: "UR5", 7: "panda", 8: "n8", 9: "n9", 10: "n10"}


def test_every_instantiation_of_the_launcher_has_a_robot():
    src = open(os.path.join(ROOT, "robotics-toolbox-python_amd", "csrc", "mmc_kernels.hip")).read()
    body = src[src.index("int launch_mmc("):]
    labels = [int(x) for x in re.findall(r"\bcase (\d+): e = mmc_go<(?:\d+)>", body)]
    assert labels and labels == [int(x) for x in re.findall(r"mmc_go<(\d+)>\(grid", body)] and "default:" not in body
    assert sorted(labels) == sorted(CENSUS), "launch_mmc has a case no robot of tests/test_mmc.py is named for"
    for n, name in CENSUS.items():
        assert cases.model(name).n == n and name in cases.ROBOTS
    assert {cases.model(n).n for n in cases.ROBOTS} == set(CENSUS)          # and the device tests run every one of them


# ------------------------------------------------------------------------------------------------ joint_velocity_damper (no GPU)
def _damper_literal(qlim, q, ps, pi, n, gain):
    """robot/Robot.py:1404-1421, with the robot's q the q handed in"""
    Ain = np.zeros((n, n))
    Bin = np.zeros(n)
    for i in range(n):
        if q[i] - qlim[0, i] <= pi:
            Bin[i] = -gain * (((qlim[0, i] - q[i]) + ps) / (pi - ps))
            Ain[i, i] = -1
        if qlim[1, i] - q[i] <= pi:
            Bin[i] = gain * ((qlim[1, i] - q[i]) - ps) / (pi - ps)
            Ain[i, i] = 1
    return Ain, Bin


def test_joint_velocity_damper_is_the_references_function():
    rng = np.random.default_rng(5)
    for robot in (rtbhip.urdf.load("Panda"), rtbhip.urdf.load("UR5")):
        ets = robot.ets()
        qlim, n = np.asarray(ets.qlim), ets.n
        q = rng.uniform(qlim[0] - 0.05, qlim[1] + 0.05, (40, n))
        q[::3] = np.where(rng.uniform(size=(14, n)) < 0.5, qlim[0] + rng.uniform(0, 0.3, (14, n)), qlim[1] - rng.uniform(0, 0.3, (14, n)))
        for ps, pi, gain, k in ((0.05, 0.1, 1.0, None), (0.1, 0.9, 2.5, None), (0.05, 0.3, 1.0, 4)):
            A, B = rtbhip.servo.joint_velocity_damper(robot, q, ps=ps, pi=pi, n=k, gain=gain)
            m = n if k is None else k
            assert A.shape == (40, m, m) and B.shape == (40, m)
            active = 0
            for i in range(40):
                a, b = _damper_literal(qlim, q[i], ps, pi, m, gain)
                assert np.array_equal(A[i], a) and np.array_equal(B[i], b)
                a1, b1 = rtbhip.servo.joint_velocity_damper(ets, q[i], ps=ps, pi=pi, n=k, gain=gain)          # 1-D q: no batch axis
                assert np.array_equal(a1, a) and np.array_equal(b1, b)
                active += int(np.abs(a).sum())
            assert active > 20
    assert not hasattr(rtbhip.models.Panda(), "joint_velocity_damper")          # a function of rtbhip.servo, not a robot method


def test_joint_velocity_damper_on_the_panda_gives_the_references_expected_matrices():
    """the two matrices the reference's own test of Robot.joint_velocity_damper expects (tests/golden/mmc_velocity_damper_panda.json), at the
    configuration that test runs at: the Panda's default q, all zeros (at qr no joint is within 0.1 of a limit and both would be zero)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "mmc_velocity_damper_panda.json")))
    for panda in (rtbhip.urdf.load("Panda"), rtbhip.models.DH.Panda()):          # the URDF model is the reference's rtb.models.Panda()
        Ain, Bin = rtbhip.servo.joint_velocity_damper(panda, np.asarray(gold["q"]))
        np.testing.assert_almost_equal(Ain, np.asarray(gold["Ain"]), decimal=4)
        np.testing.assert_almost_equal(Bin, np.asarray(gold["Bin"]), decimal=4)
        assert np.abs(Ain).sum() == 2


# ------------------------------------------------------------------------------------------------ the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the reactive QP servo runs on the device only: not served by the CPU replay")(f))


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]          # (a copy: the cases are read-only)


def _p(x):
    return None if x is None else (x.ptr.value if hasattr(x, "ptr") else x.data_ptr())


def _call(torch, ets, q, Tep, su, method, gain6, threshold, dt, steps, qd, q_out, arrived, its, status, N=None, nTep=None):
    """the entry point on device buffers (tensors or flush_guard.Guarded), current stream; qlim and qdlim are the setup's host arrays"""
    a = ARGS()
    a.size, a.method, a.chain = C.sizeof(ARGS), method, ets._handle()
    a.N = q.shape[0] if N is None else N
    a.nTep = (Tep.reshape(-1, 16).shape[0] if nTep is None else nTep)
    qlim = np.ascontiguousarray(su.qlim)
    a.q, a.Tep, a.qlim, a.qdlim = _p(q), _p(Tep), qlim.ctypes.data, None if su.qdlim is None else su.qdlim.ctypes.data
    a.qd, a.q_out, a.arrived, a.its, a.status = _p(qd), _p(q_out), _p(arrived), _p(its), _p(status)
    a.gain6 = (C.c_double * 6)(*gain6)
    a.threshold, a.dt, a.steps = threshold, dt, steps
    a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = su.Y, su.ks, su.km, su.ps, su.pi, su.dgain
    a.stream = torch.cuda.current_stream().cuda_stream
    _lib.check(getattr(_lib.lib(), FN)(C.byref(a)))


def _raw(ets, q, Tep, su, method, gain6, threshold, dt, steps, want=(True, True)):
    """-> [qd, q_out, arrived (uint8), its (int32), status (uint8)] as device tensors; an output not wanted is None (handed over as NULL)"""
    torch = _torch()
    N, n = q.shape
    qd, qo = (torch.full((N, n), float("nan"), dtype=torch.float64, device=q.device) if w else None for w in want)
    arrived, its = torch.full((N,), 7, dtype=torch.uint8, device=q.device), torch.full((N,), -7, dtype=torch.int32, device=q.device)
    status = torch.full((N,), 77, dtype=torch.uint8, device=q.device)
    _call(torch, ets, q, Tep, su, method, gain6, threshold, dt, steps, qd, qo, arrived, its, status)
    return [qd, qo, arrived, its, status]


def _np(outs):
    return [None if x is None else x.cpu().numpy() for x in outs]


STEP = (cases.THRESHOLD, 0.0, 1)          # after cases.gain_of(case)
LOOP = (cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, cases.STEPS)
SIZES = (1, 63, 64, 65, 70)


def _tiled_ref(ref, N):
    rows = len(ref["first"])
    return {"qd": cases.tiled(ref["qd"], N), "first": [ref["first"][i % rows] for i in range(N)]}


@gpu
@pytest.mark.parametrize("case", cases.every_case(), ids=cases.case_id)
def test_single_step_equals_the_oracle_between_guard_rows(case):
    """1: every robot x method x km on / off x velocity box / none (and the narrow joint), N = 1, 63, 64, 65, 70, inputs and outputs between
    poisoned guard rows of one allocation each"""
    torch = _torch()
    from flush_guard import Guarded
    ets, q, Tep, su, ref, _, _ = cases.step_case(case)
    n, worst = ets.n, 0.0
    for N in SIZES:
        t = lambda a: cases.tiled(a, N)
        ins = [Guarded(torch, N, n, "float64").load(torch, t(q)), Guarded(torch, N, 16, "float64").load(torch, t(Tep).reshape(N, 16))]
        before = [g.bits.clone() for g in ins]
        outs = [Guarded(torch, N, n, "float64"), Guarded(torch, N, n, "float64"), Guarded(torch, N, 1, "uint8"), Guarded(torch, N, 1, "int32"),
                Guarded(torch, N, 1, "uint8")]
        _call(torch, ets, ins[0], ins[1], su, case[1], cases.gain_of(case), *STEP, *outs, N=N, nTep=N)
        torch.cuda.synchronize()
        assert all(torch.equal(g.bits, b) for g, b in zip(ins, before)), (case, N)
        for o in outs:
            assert o.guards_intact() and not bool((o.live_bits() == o.pattern).any()), (case, N)
        qd, qo, arrived, its, status = (o.live().cpu().numpy() for o in outs)
        worst = max(worst, float(cases.step_ratio(qd, _tiled_ref(ref, N)).max()))
        assert np.array_equal(arrived[:, 0] != 0, t(ref["arrived"])) and (its == 1).all() and not status.any(), (case, N)
        assert np.array_equal(qo, t(q)), (case, N)                                # dt = 0
    print("mmc device step %s: ratio %.3f (K %.1f, replay %.3f)" % (cases.case_id(case), worst, cases.K, cases.K_MEASURED))
    assert worst <= cases.K


@gpu
@pytest.mark.parametrize("method", cases.METHODS, ids=[cases.METHOD_NAMES[m] for m in cases.METHODS])
@pytest.mark.parametrize("name", cases.LOOP_ROBOTS)
def test_loop_equals_the_oracle(name, method):
    """2: steps = 8, three kinds of rows interleaved inside one wave (tests/test_mmc_emu.py asserts them on the oracle): arrived, its and status
    exactly, q_out within the loop bound"""
    torch = _torch()
    ets, q, Tep, su, ref, _ = cases.loop_case(name, method)
    N = 70
    t = lambda a: cases.tiled(a, N)
    qd, qo, arrived, its, status = _np(_raw(ets, *_dev(torch, t(q), t(Tep)), su, method, *LOOP))
    assert np.array_equal(arrived != 0, t(ref["arrived"])) and np.array_equal(its, t(ref["its"])) and np.array_equal(status, t(ref["status"]))
    r = cases.rc.ratio(qo, t(ref["q"]), t(ref["cond"])) / t(ref["amp"])
    print("mmc device loop %s/%s: ratio %.3f (K_LOOP %.1f, replay %.3f), its %s" % (name, cases.METHOD_NAMES[method], r.max(), cases.K_LOOP,
                                                                                  cases.K_LOOP_MEASURED, np.bincount(its).tolist()))
    assert r.max() <= cases.K_LOOP


N_DISTINCT = 70


@gpu
@pytest.mark.parametrize("name", ["UR5", "panda", "n10"])
def test_every_row_distinct(name):
    """3: 70 distinct rows -- a full tile and a ragged one -- against the oracle, between guard rows; and the comparison is one that a swap of two
    rows 2 or 8 apart fails"""
    torch = _torch()
    from flush_guard import Guarded
    N = N_DISTINCT
    case = (name, 1, True, True, "plain")
    ets, q, Tep, su, ref, _, _ = cases.step_case(case, rows=N)
    n = ets.n
    ins = [Guarded(torch, N, n, "float64").load(torch, np.array(q)), Guarded(torch, N, 16, "float64").load(torch, np.array(Tep).reshape(N, 16))]
    outs = [Guarded(torch, N, n, "float64"), Guarded(torch, N, n, "float64"), Guarded(torch, N, 1, "uint8"), Guarded(torch, N, 1, "int32"),
            Guarded(torch, N, 1, "uint8")]
    _call(torch, ets, ins[0], ins[1], su, 1, cases.gain_of(case), cases.THRESHOLD, 0.5, 1, *outs, N=N, nTep=N)
    torch.cuda.synchronize()
    for o in outs:
        assert o.guards_intact() and not bool((o.live_bits() == o.pattern).any())
    qd, qo, arrived, its, status = (o.live().cpu().numpy() for o in outs)
    r = cases.step_ratio(qd, ref)
    print("mmc device distinct %s: ratio %.3f (K %.1f)" % (name, r.max(), cases.K))
    assert r.max() <= cases.K and not status.any() and np.array_equal(qo, np.asarray(q) + 0.5 * qd)
    for gap in (2, 8):
        for i in (0, 31, 61, N - 1 - gap):
            swapped = np.array(qd)
            swapped[[i, i + gap]] = swapped[[i + gap, i]]
            assert cases.step_ratio(swapped, ref).max() > cases.K, (name, gap, i)


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@gpu
@pytest.mark.parametrize("steps", [1, cases.STEPS])
@pytest.mark.parametrize("name", ["UR5", "panda", "n10"])
def test_rows_are_independent_bit_for_bit(name, steps):
    """4: a row of a batch has the bits of that row computed alone and of that row in a permuted batch -- for the loop too, where the lanes of a
    wave stop at different iterations and their QPs at different rounds"""
    torch = _torch()
    ets, q, Tep, su, ref, _ = cases.loop_case(name, 1)
    N = 130
    t = lambda a: cases.tiled(a, N)
    q, Tep = np.array(t(q)), t(Tep)
    q += 1e-3 * np.arange(N)[:, None] / N                                         # distinct rows, the same kinds
    args = (su, 1, cases.GAIN_LOOP, cases.THRESHOLD, cases.DT, steps)
    base = _np(_raw(ets, *_dev(torch, q, Tep), *args))
    if steps > 1:
        assert len(set(base[3].tolist())) >= 3                                    # lanes of one wave stop at different iterations
    perm = np.random.default_rng(3).permutation(N)
    moved = _np(_raw(ets, *_dev(torch, q[perm], Tep[perm]), *args))
    assert all(_bits(m, b[perm]) for m, b in zip(moved, base))
    for k in (0, 1, 2, 63, 64, 129):
        alone = _np(_raw(ets, *_dev(torch, q[k:k + 1], Tep[k:k + 1]), *args))
        assert all(_bits(a[0], b[k]) for a, b in zip(alone, base)), (name, k)


@gpu
@pytest.mark.parametrize("name", ["UR5", "panda", "n9"])
def test_output_selection_and_one_tep(name):
    """5: qd-only, q_out-only and both return the same bits and leave the NULL side's buffer untouched (NULL flags too); nTep = 1 is the broadcast"""
    torch = _torch()
    from flush_guard import Guarded
    ets, q, Tep, su, ref, _, _ = cases.step_case((name, 0, True, True, "plain"))
    N, n = 70, ets.n
    t = lambda a: cases.tiled(a, N)
    dq, dT = _dev(torch, t(q), t(Tep))
    both = _raw(ets, dq, dT, su, 0, *LOOP)
    for want in ((True, False), (False, True)):
        outs = [Guarded(torch, N, n, "float64"), Guarded(torch, N, n, "float64"), Guarded(torch, N, 1, "uint8"), Guarded(torch, N, 1, "int32"),
                Guarded(torch, N, 1, "uint8")]
        _call(torch, ets, dq, dT, su, 0, *LOOP, outs[0] if want[0] else None, outs[1] if want[1] else None, outs[2], outs[3], outs[4], N=N, nTep=N)
        torch.cuda.synchronize()
        for o, w, b in zip(outs, want + (True, True, True), both):
            assert o.guards_intact()
            if w:
                assert torch.equal(o.live().reshape(b.shape), b)
            else:
                assert bool((o.live_bits() == o.pattern).all())
        got = torch.full((N, n), float("nan"), dtype=torch.float64, device="cuda")
        _call(torch, ets, dq, dT, su, 0, *LOOP, got if want[0] else None, got if want[1] else None, None, None, None, N=N, nTep=N)
        torch.cuda.synchronize()
        assert torch.equal(got, both[0] if want[0] else both[1])                    # arrived, its and status NULL as well: the same bits
    one = _raw(ets, dq, dT[4:5].contiguous(), su, 0, *LOOP)
    bc = _raw(ets, dq, dT[4:5].expand(N, 4, 4).contiguous(), su, 0, *LOOP)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(one, bc))


@gpu
@pytest.mark.parametrize("steps", [1, cases.STEPS])
def test_unsolvable_rows_keep_to_their_rows(steps):
    """6: a row whose box is empty and two rows whose q is not finite: status bit 0, rate and q non-finite, never arrived, its = steps (the loop
    leaves on time); their neighbours' bits and status are those of the batch without them.  Inputs the kernel is specified to handle."""
    torch = _torch()
    ets, q, Tep, su, ref = cases.unsolvable_case("panda")
    good = cases.step_case(("panda", 1, True, True, "plain"))[1]
    N = 70
    t = lambda a: cases.tiled(a, N)
    args = (su, 1, cases.gain_of(("panda", 1, True, True, "plain")), cases.THRESHOLD, 0.05, steps)
    base = _np(_raw(ets, *_dev(torch, t(good), t(Tep)), *args))
    q2 = np.array(t(good))
    q2[cases.UNSOLVABLE_ROW] = q[cases.UNSOLVABLE_ROW]
    q2[11, 3] = np.nan
    q2[66, 0] = np.inf
    got = _np(_raw(ets, *_dev(torch, q2, t(Tep)), *args))
    bad = [cases.UNSOLVABLE_ROW, 11, 66]
    others = np.delete(np.arange(N), bad)
    assert all(_bits(x[others], y[others]) for x, y in zip(got, base))
    assert not np.isfinite(got[0][bad]).any() and not np.isfinite(got[1][bad]).any()
    assert (got[2][bad] == 0).all() and (got[3][bad] == steps).all() and (got[4][bad] == 1).all() and not (base[4] & 1).any()
    if steps == 1:
        alone = _np(_raw(ets, *_dev(torch, q, Tep), *args))
        assert np.array_equal(alone[4], ref["status"])                            # the oracle's own verdict on the empty box


@gpu
def test_a_slack_beyond_ten_sets_status_bit_one():
    """6b: gains 40 times the case's: the oracle's slack is past 20 on some rows and clear of 10 on all; bit 1 is the oracle's on every row"""
    torch = _torch()
    ets, q, Tep, su, gain6, ref = cases.slack_case()
    N = 70
    t = lambda a: cases.tiled(a, N)
    qd, qo, arrived, its, status = _np(_raw(ets, *_dev(torch, t(q), t(Tep)), su, 1, gain6, cases.THRESHOLD, 0.0, 1))
    assert np.array_equal(status, t(ref["status"])) and (status == 2).any() and (status == 0).any()
    assert np.array_equal(arrived != 0, t(ref["arrived"])) and cases.step_ratio(qd, _tiled_ref(ref, N)).max() <= cases.K


@gpu
def test_one_captured_graph_replayed_twice():
    """7: one launch on the caller's stream under torch.cuda.graph, captured after one eager warm-up (the table's upload), replayed to the eager
    result and again on new inputs: everything the loop needs -- the host arrays qlim and qdlim too -- travels in the kernel's parameters"""
    torch = _torch()
    ets, q, Tep, su, ref, _ = cases.loop_case("panda", 1)
    N = 130
    t = lambda a: cases.tiled(a, N)
    dq, dT = _dev(torch, t(q), t(Tep))
    eager0 = [x.clone() for x in _raw(ets, dq, dT, su, 1, *LOOP)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _raw(ets, dq, dT, su, 1, *LOOP)          # (the host copies of qlim / qdlim made for this call are gone when it replays)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(outs, eager0))
    dq.copy_(dq.flip(0))
    dT.copy_(dT.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    eager1 = _raw(ets, dq, dT, su, 1, *LOOP)
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(first, eager1)) and not torch.equal(first[1], eager0[1])
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(outs, first))                      # and the same bits the second time


# ------------------------------------------------------------------------------------------------ the Python surface
@gpu
def test_the_python_surface():
    torch = _torch()
    case = ("panda", 1, True, True, "plain")
    ets, q, Tep, su, ref, _, _ = cases.step_case(case)
    panda = rtbhip.models.Panda()
    kw = dict(gain=cases.gain_of(case), qlim=su.qlim, qdlim=cases.QDLIM)
    dq, dT = _dev(torch, q, Tep)
    qd, arrived, status = rtbhip.servo.mmc(panda, dq, dT, **kw)
    raw = _raw(ets, dq, dT, su, 1, cases.gain_of(case), *STEP, want=(True, False))
    assert torch.equal(qd, raw[0]) and arrived.dtype == torch.bool and torch.equal(arrived, raw[2].bool()) and status.dtype == torch.uint8 and torch.equal(status, raw[4])
    hq, ha, hs = rtbhip.servo.mmc(panda, q, Tep, **kw)                            # NumPy in, NumPy out
    assert isinstance(hq, np.ndarray) and _bits(hq, qd.cpu().numpy()) and ha.dtype == bool and np.array_equal(ha, arrived.cpu().numpy())
    assert hs.dtype == np.uint8 and not hs.any()
    q1, a1, s1 = rtbhip.servo.mmc(ets, q[3], Tep[3], **kw)                         # a 1-D q: unbatched
    assert q1.shape == (7,) and isinstance(a1, bool) and isinstance(s1, int) and _bits(q1, hq[3])
    ets2, ql, Tl, sul, refl, _ = cases.loop_case("panda", 1)
    dql, dTl = _dev(torch, ql, Tl)
    dql.requires_grad_(True)                                                       # no gradients: as with a plain tensor
    kwl = dict(gain=2.0, qlim=sul.qlim, qdlim=sul.qdlim)
    qo, arr, its, st = rtbhip.servo.mmc_servo(panda, dql, dTl, cases.DT, cases.STEPS, **kwl)
    rawl = _raw(ets2, dql.detach(), dTl, sul, 1, *LOOP, want=(False, True))
    assert torch.equal(qo, rawl[1]) and not qo.requires_grad and its.dtype == torch.int32 and torch.equal(its, rawl[3]) and torch.equal(arr, rawl[2].bool())
    ho, har, hits, hst = rtbhip.servo.mmc_servo(panda, ql, Tl, cases.DT, cases.STEPS, method="rpy", **kwl)
    assert _bits(ho, qo.cpu().numpy()) and hits.dtype == np.int32 and np.array_equal(hits, refl["its"]) and np.array_equal(har, refl["arrived"]) and not hst.any()
    o1, r1, i1, s1 = rtbhip.servo.mmc_servo(panda, ql[1], Tl[1], cases.DT, cases.STEPS, **kwl)
    assert o1.shape == (7,) and isinstance(r1, bool) and isinstance(i1, int) and s1 == 0 and _bits(o1, ho[1]) and i1 == int(hits[1])
    # qlim=None: the chain's own limits; km = 0, no box, one (4, 4) target, angle-axis
    own = cases.Setup(7, km=0.0, box=False)
    own.qlim = np.asarray(panda.ets().qlim)
    inside = np.clip(q, own.qlim[0] + 0.2, own.qlim[1] - 0.2)
    di, = _dev(torch, inside)
    oneT = rtbhip.servo.mmc(panda, di, dT[2], method="angle-axis", km=0.0)[0]
    assert torch.equal(oneT, _raw(ets, di, dT[2:3].contiguous(), own, 0, (1.0,) * 6, 0.1, 0.0, 1, want=(True, False))[0])
    with pytest.raises(TypeError):
        rtbhip.servo.mmc(panda, dq.float(), dT.float())
    with pytest.raises(ValueError):
        rtbhip.servo.mmc(panda, dq, dT, method="euler")
    with pytest.raises(ValueError):
        rtbhip.servo.mmc(panda, dq, dT, qlim=np.zeros((2, 6)))
    with pytest.raises(ValueError):
        rtbhip.servo.mmc(panda, dq, Tep)                                           # a device q with a host Tep
    with pytest.raises(rtbhip.RtbHipError):
        rtbhip.servo.mmc_servo(panda, dq, dT, 0.1, 5000)
    with pytest.raises(rtbhip.RtbHipError):
        rtbhip.servo.mmc(cases.model("n5").ets, np.zeros(5), np.eye(4), qlim=np.array([[-3.0] * 5, [3.0] * 5]))          # fewer than six joints


def _readme_lines():
    text = open(os.path.join(ROOT, "README.md")).read()
    lines = [l for l in text.splitlines() if re.search(r"\bmmc(_servo)?\(", l) and " = " in l and not l.lstrip().startswith(("|", "-", "*"))]
    assert len(lines) == 2, lines
    imports = [l for l in text.splitlines() if l.strip().startswith("from rtbhip.servo import")]
    assert len(imports) == 1, imports
    return "\n".join(l.strip() for l in imports + lines)


def test_readme_example_lines_are_python():
    compile(_readme_lines(), "README.md", "exec")


@gpu
def test_readme_example_lines_run():
    torch = _torch()
    panda = rtbhip.models.Panda()
    q = torch.rand(256, 7, device="cuda", dtype=torch.float64) * 0.4 + torch.tensor([0.0, -0.5, 0.0, -2.2, 0.0, 2.0, 0.6], device="cuda", dtype=torch.float64)
    Tep = panda.fkine(q + 0.1)
    ns = {"torch": torch, "rtbhip": rtbhip, "panda": panda, "q": q, "Tep": Tep}
    exec(compile(_readme_lines(), "README.md", "exec"), ns)          # noqa: S102 -- our own README
    assert tuple(ns["qd"].shape) == (256, 7) and tuple(ns["q_out"].shape) == (256, 7) and ns["its"].dtype == torch.int32
    assert not bool(ns["status"].any()) and bool(torch.isfinite(ns["q_out"]).all())
