"""-m gpu: the STAGED RTBHIP_MEM_HOST path (csrc/api.cpp: stage the host arrays into cached device blocks, one launch, copy back) of the
entry points that are not row-pipelined.  Through the raw ABI, the host-array call must equal the device-pointer call BIT for bit: the
same kernel runs on the same rows, so any difference is a wrong byte count or a swapped buffer.  N = 1 is one lane of one wave, N = 65 a
full tile plus a one-row tail.  (The pipelined entries -- fkine / jacob / hessian / rne -- are tests/test_host_path.py's.)"""
import ctypes as C

import numpy as np
import numpy.testing as nt
import pytest

import rtbhip
from flush_guard import Out, both_ways

pytestmark = pytest.mark.gpu

SIZES = [1, 65]


@pytest.fixture(scope="module")
def panda():
    return rtbhip.models.Panda().ets()


def _q(N, n, seed=0):
    return np.random.default_rng(100 * N + seed).uniform(-2.0, 2.0, (N, n))


@pytest.mark.parametrize("N", SIZES)
def test_from_jacobian_entries(N, panda):
    J = np.asarray(panda.jacob0(_q(N, 7))).reshape(N, 6, 7)
    (H,) = both_ways("rtbhip_hessian_from_jacobian", lambda p, mem, s: (p(J), N, 7, p(Out(N, 7, 6, 7)), mem, s))
    for method in (0, 1, 2):
        both_ways("rtbhip_manipulability_from_jacobian", lambda p, mem, s: (p(J), N, 7, 63, method, p(Out(N)), mem, s))
    both_ways("rtbhip_jacobm_from_jacobian", lambda p, mem, s: (p(J), None, N, 7, 63, p(Out(N, 7)), mem, s))
    both_ways("rtbhip_jacobm_from_jacobian", lambda p, mem, s: (p(J), p(H), N, 7, 7, p(Out(N, 7)), mem, s))


@pytest.mark.parametrize("N", SIZES)
def test_pose_error_and_p_servo(N, panda):
    Te = np.asarray(panda.eval(_q(N, 7))).reshape(N, 4, 4)
    Tep = np.asarray(panda.eval(_q(N, 7, 1))).reshape(N, 4, 4)
    gain = np.array([1.0, 2.0, 3.0, 0.5, 0.25, 4.0])
    for a, na, b, nb in ((Te, N, Tep, N), (Te[:1], 1, Tep, N), (Te, N, Tep[:1], 1)):           # equal counts and both broadcasts
        both_ways("rtbhip_angle_axis", lambda p, mem, s: (p(a), na, p(b), nb, p(Out(N, 6)), mem, s))
        for method in (0, 1):
            both_ways("rtbhip_p_servo_error", lambda p, mem, s: (p(a), na, p(b), nb, method, p(Out(N, 6)), mem, s))
            v, arrived = both_ways("rtbhip_p_servo", lambda p, mem, s: (p(a), na, p(b), nb, method, gain.ctypes.data, 2.5, p(Out(N, 6)),
                                                                        p(Out(N, dtype=np.uint8)), mem, s))
            assert set(np.unique(arrived)) <= {0, 1}


@pytest.mark.parametrize("N", SIZES)
def test_differential_kinematics_of_a_chain(N, panda):
    h, q, qd = panda._handle(), _q(N, 7), _q(N, 7, 1)
    for frame in (0, 1):
        both_ways("rtbhip_jacob_dot", lambda p, mem, s: (h, p(q), p(qd), N, None, frame, p(Out(N, 6, 7)), mem, s))
    for rep in (0, 3):
        both_ways("rtbhip_jacob0_analytical", lambda p, mem, s: (h, p(q), N, None, rep, p(Out(N, 6, 7)), mem, s))
        both_ways("rtbhip_jacob0_dot_analytical", lambda p, mem, s: (h, p(q), p(qd), N, None, rep, p(Out(N, 6, 7)), mem, s))
    for method in (0, 1, 2):
        both_ways("rtbhip_manipulability", lambda p, mem, s: (h, p(q), N, None, 63, method, p(Out(N)), mem, s))
    both_ways("rtbhip_jacobm", lambda p, mem, s: (h, p(q), N, None, 7, p(Out(N, 7)), mem, s))


@pytest.mark.parametrize("N", SIZES)
def test_link_frames_and_partial_fkine0(N, panda):
    h, q = panda._handle(), _q(N, 7)
    marks = np.array([3, 10, 22], dtype=np.int32)
    base = np.eye(4)
    base[:3, 3] = [0.1, -0.2, 0.3]
    both_ways("rtbhip_link_frames", lambda p, mem, s: (h, p(q), N, base.ctypes.data, marks.ctypes.data, 3, p(Out(N, 3, 4, 4)), mem, s))
    both_ways("rtbhip_partial_fkine0", lambda p, mem, s: (h, p(q), N, None, 3, p(Out(N, 7, 7, 6, 7)), mem, s))
    both_ways("rtbhip_partial_fkine0", lambda p, mem, s: (h, p(q), N, None, 4, p(Out(N, 7, 7, 7, 6, 7)), mem, s))


@pytest.mark.parametrize("N", SIZES)
def test_ik_lm_from_a_supplied_start(N, panda):
    """q0 given and slimit = 1: no restart vector is drawn, all five outputs are deterministic"""
    h = panda._handle()
    qgoal = np.random.default_rng(N).uniform(-1.0, 1.0, (N, 7)) + np.array([0, 0.3, 0, -1.8, 0, 2.0, 0.6])
    Tep = np.asarray(panda.eval(qgoal)).reshape(N, 4, 4)
    q0 = qgoal + np.random.default_rng(N + 1).uniform(-0.2, 0.2, (N, 7))
    q, ok, it, se, res = both_ways("rtbhip_ik_lm", lambda p, mem, s: (
        h, p(Tep), N, p(q0), 30, 1, 1e-6, 0, None, 1.0, 0, 0, 0, p(Out(N, 7)), p(Out(N, dtype=np.int32)), p(Out(N, dtype=np.int32)),
        p(Out(N, dtype=np.int32)), p(Out(N)), mem, s))
    assert ok.min() >= 0 and ok.max() == 1 and it.min() >= 1 and it.max() <= 30 and np.isfinite(q).all() and np.isfinite(res).all()


@pytest.mark.parametrize("N", SIZES)
def test_dynamics_terms_of_a_dh_arm(N):
    arm = rtbhip.models.DH.Panda()
    h, q, qd, tq = arm._dyn_handle(), _q(N, 7), _q(N, 7, 1), _q(N, 7, 2)
    g = np.array([0.5, -0.3, -9.81])
    both_ways("rtbhip_inertia", lambda p, mem, s: (h, p(q), N, p(Out(N, 7, 7)), mem, s))
    both_ways("rtbhip_coriolis", lambda p, mem, s: (h, p(q), p(qd), N, p(Out(N, 7, 7)), mem, s))
    both_ways("rtbhip_accel", lambda p, mem, s: (h, p(q), p(qd), p(tq), N, g.ctypes.data, p(Out(N, 7)), mem, s))


@pytest.mark.parametrize("N", SIZES)
def test_dynamics_of_a_link_tree(N):
    rob = rtbhip.urdf.load("Panda").erobot()
    n = rob.n
    h, q, qd, tq = rob._handle(), _q(N, n), _q(N, n, 1), _q(N, n, 2)
    g = np.array([0.5, -0.3, -9.81])
    both_ways("rtbhip_tree_rne", lambda p, mem, s: (h, p(q), p(qd), p(tq), N, g.ctypes.data, p(Out(N, n)), mem, s))
    both_ways("rtbhip_tree_rne", lambda p, mem, s: (h, p(q), None, None, N, g.ctypes.data, p(Out(N, n)), mem, s))       # NULL qd / qdd: zeros
    both_ways("rtbhip_tree_inertia", lambda p, mem, s: (h, p(q), N, p(Out(N, n, n)), mem, s))
    both_ways("rtbhip_tree_coriolis", lambda p, mem, s: (h, p(q), p(qd), N, p(Out(N, n, n)), mem, s))
    both_ways("rtbhip_tree_accel", lambda p, mem, s: (h, p(q), p(qd), p(tq), N, g.ctypes.data, p(Out(N, n)), mem, s))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("packed", [False, True])
def test_fleet_of_two_chains_around_an_empty_one(N, packed, panda):
    """chains of 7 and 6 joints with a chain of N = 0 (NULL buffers) between them"""
    puma = rtbhip.models.DH.Puma560().ets()
    handles = (C.c_uint64 * 3)(panda._handle(), panda._handle(), puma._handle())
    Ns = (C.c_int64 * 3)(N, 0, N + 2)
    qa, qb = _q(N, 7), _q(N + 2, 6)

    def args(p, mem, s):
        qs = (C.c_void_p * 3)(p(qa), None, p(qb))
        if packed:
            TJ = (C.c_void_p * 3)(p(Out(N, 16 + 42)), None, p(Out(N + 2, 16 + 36)))
            return (handles, 3, qs, Ns, 0, TJ, mem, s)
        T = (C.c_void_p * 3)(p(Out(N, 4, 4)), None, p(Out(N + 2, 4, 4)))
        J = (C.c_void_p * 3)(p(Out(N, 6, 7)), None, p(Out(N + 2, 6, 6)))
        return (handles, 3, qs, Ns, 0, T, J, mem, s)
    outs = both_ways("rtbhip_fleet_fkine_jacob_packed" if packed else "rtbhip_fleet_fkine_jacob", args)
    Ta = np.asarray(panda.eval(qa)).reshape(N, 16)
    got = outs[0][:, :16] if packed else outs[0].reshape(N, 16)
    nt.assert_allclose(got, Ta, rtol=0, atol=1e-12)
