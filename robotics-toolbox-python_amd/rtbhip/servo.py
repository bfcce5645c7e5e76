"""Resolved-rate motion control: the loop the reference's README opens with,

    v, arrived = rtb.p_servo(panda.fkine(panda.q), Tep, 1)
    panda.qd = np.linalg.pinv(panda.jacobe(panda.q)) @ v

as ONE launch of rtbhip_rrmc per call, for N arms at once:

    qd, arrived         = rtbhip.servo.rrmc(robot, q, Tep, gain=1.0, threshold=0.1, method="rpy", damping=0.0, qnull=None)
    q_out, arrived, its = rtbhip.servo.servo(robot, q, Tep, dt, steps, gain=1.0, threshold=0.1, method="rpy", damping=0.0, qnull=None)

rrmc is the single step: qd = qnull + pinv(J(q)) (gain * e - J qnull) with e and `arrived` exactly rtbhip.p_servo's, J = jacobe for the "rpy"
error (seen from the end-effector frame) and jacob0 for the "angle-axis" error (in the base frame).  servo iterates q <- q + dt * qd on the device,
at most `steps` times; a row stops after the step of the iteration in which it arrives (as the README loop does), `its` counts its iterations.
pinv(J) is applied as solves (include/rtbhip.h has the rule); at a rank-deficient J numpy's truncated pinv is not reproduced -- the row comes back
non-finite, and `damping` is the remedy.  Chains of 1..10 joints.

`robot` is an ETS or anything with .ets() (DHRobot, ERobot, the models, PoERobot).  CUDA float64 tensors in give tensors out on the current stream
(`arrived` torch.bool, `its` torch.int32).  NumPy in gives NumPy out, staged through the ABI's own device-memory helpers as rtbhip/opspace.py
does: correct, not fast.  float32 tensors are refused as elsewhere.  No gradients: under requires_grad the call behaves as with a plain tensor.
A 1-D q returns unbatched results.

The REACTIVE QP SERVO (rtbhip_mmc; the controller of the reference's examples/mmc.py): p_servo's error, a slack on the task, the manipulability
Jacobian as the linear cost, Robot.joint_velocity_damper's rows and the joint-velocity box as constraints, solved per row on the device:

    qd, arrived, status         = rtbhip.servo.mmc(robot, q, Tep, gain=1.0, threshold=0.1, method="rpy", Y=0.01, ks=1.0, km=1.0, ps=0.05, pi=0.9,
                                                   damper_gain=1.0, qlim=None, qdlim=None)
    q_out, arrived, its, status = rtbhip.servo.mmc_servo(robot, q, Tep, dt, steps, ...)
    Ain, Bin                    = rtbhip.servo.joint_velocity_damper(robot, q, ps=0.05, pi=0.1, n=None, gain=1.0)

qlim=None takes the chain's own limits, qdlim=None leaves the rate unboxed; both are host arrays whatever memory q lives in.  status (uint8):
bit 0 the row's QP was unsolvable (qd / q_out non-finite), bit 1 its slack went beyond 10.  Chains of 6..10 joints.  include/rtbhip.h has the
definition and the deviations from the example.  joint_velocity_damper is the reference's function on the host, for callers with a QP solver
of their own.  These are functions, not robot methods."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, as_numeric, is_torch
from .opspace import _Staged

METHODS = {"angle-axis": 0, "rpy": 1}


def _ets(robot):
    from .et import ETS
    if isinstance(robot, ETS):
        return robot
    if hasattr(robot, "ets"):
        return robot.ets()
    raise TypeError("%s is neither an ETS nor a robot with .ets()" % type(robot).__name__)


def _method(method):
    if method not in METHODS:
        raise ValueError("method must be \"rpy\" or \"angle-axis\"")
    return METHODS[method]


def _gain6(gain):
    g = np.asarray(gain, dtype=np.float64).reshape(-1)
    if g.size == 1:
        g = np.full(6, float(g[0]))
    if g.size != 6:
        raise ValueError("gain must be a scalar or six values")
    return g


def _shape(ets, q, Tep, qnull):
    """-> (q (N, n), Tep (N or 1, 4, 4), qnull (N, n) | None, single, torch?), all contiguous and in one kind of memory"""
    n = ets.n
    things = [x for x in (q, Tep, qnull) if x is not None]
    tm = is_torch(q) and q.is_cuda
    if tm:
        if not all(is_torch(x) and x.is_cuda for x in things):
            raise ValueError("q, Tep and qnull must all be host arrays or all be CUDA tensors")
        _lib.device_dtype(things)
        single = q.dim() == 1
        q2 = q.detach().reshape(-1, n).contiguous()
        T3 = Tep.detach().reshape(-1, 4, 4).contiguous()
        qn = None if qnull is None else qnull.detach().reshape(-1, n)
        if qn is not None and qn.shape[0] == 1 and q2.shape[0] > 1:
            qn = qn.expand(q2.shape[0], n)
        qn = None if qn is None else qn.contiguous()
    else:
        if any(is_torch(x) and x.is_cuda for x in things):
            raise ValueError("q, Tep and qnull must all be host arrays or all be CUDA tensors")
        host = lambda x: x.detach().numpy() if is_torch(x) else x
        a = as_numeric(host(q))
        single = a.ndim == 1
        q2 = np.ascontiguousarray(a.reshape(-1, n))
        T3 = np.ascontiguousarray(as_numeric(host(Tep), "Tep").reshape(-1, 4, 4))
        qn = None if qnull is None else as_numeric(host(qnull), "qnull").reshape(-1, n)
        if qn is not None and qn.shape[0] == 1 and q2.shape[0] > 1:
            qn = np.broadcast_to(qn, q2.shape)
        qn = None if qn is None else np.ascontiguousarray(qn)
    N = q2.shape[0]
    if T3.shape[0] not in (1, N):
        raise ValueError("Tep must be (4, 4) or (%d, 4, 4)" % N)
    if qn is not None and tuple(qn.shape) != (N, n):
        raise ValueError("qnull must be (%d,) or (%d, %d)" % (n, N, n))
    return q2, T3, qn, single, tm


def _block(ets, N, nTep, method, gain, threshold, damping, dt, steps):
    a = _lib.rtbhip_rrmc_args()
    a.size = C.sizeof(_lib.rtbhip_rrmc_args)
    a.method, a.chain, a.N, a.nTep = _method(method), ets._handle(), N, nTep
    a.gain6 = (C.c_double * 6)(*_gain6(gain))
    a.threshold, a.damping, a.dt, a.steps = float(threshold), float(damping), float(dt), int(steps)
    return a


def launch(ets, q2, T3, qn, tm, method, gain, threshold, damping, dt, steps, want_qd, want_q):
    """one launch -> (qd | None, q_out | None, arrived, its) in the memory q2 lives in"""
    N, n = q2.shape
    a = _block(ets, N, T3.shape[0], method, gain, threshold, damping, dt, steps)
    if tm:
        import torch
        _lib.note_device(q2)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=q2.device)
        qd, qo = (new((N, n), torch.float64) if w else None for w in (want_qd, want_q))
        arrived, its = new((N,), torch.uint8), new((N,), torch.int32)
        ptr = lambda x: None if x is None else x.data_ptr()
        a.q, a.Tep, a.qnull, a.qd, a.q_out, a.arrived, a.its = ptr(q2), ptr(T3), ptr(qn), ptr(qd), ptr(qo), ptr(arrived), ptr(its)
        a.stream = _lib.current_stream_ptr().value
        check(lib().rtbhip_rrmc(C.byref(a)))
        return qd, qo, arrived.bool(), its
    if N == 0:
        check(lib().rtbhip_rrmc(C.byref(a)))
        return (np.empty((0, n)) if want_qd else None, np.empty((0, n)) if want_q else None, np.empty(0, dtype=bool), np.empty(0, dtype=np.int32))
    st = _Staged()
    try:
        a.q, a.Tep = st.put(q2).value, st.put(T3).value
        a.qnull = None if qn is None else st.put(qn).value
        pairs = [st.out((N, n)) if w else (None, None) for w in (want_qd, want_q)]
        flags = st.out((N + 7) // 8 + (N + 1) // 2)          # arrived (N bytes) and its (N int32) share one block of doubles
        base = flags[1].value
        a.qd, a.q_out = (None if p is None else p.value for _, p in pairs)
        a.its, a.arrived = base, base + 8 * ((N + 1) // 2)
        check(lib().rtbhip_rrmc(C.byref(a)))
        st.fetch()                                   # (a synchronous copy on the null stream: it waits for the launch)
    finally:
        st.free()
    raw = flags[0].view(np.uint8)
    its = raw[:4 * N].view(np.int32).copy()
    arrived = raw[8 * ((N + 1) // 2):8 * ((N + 1) // 2) + N] != 0
    return pairs[0][0], pairs[1][0], arrived, its


def rrmc(robot, q, Tep, gain=1.0, threshold=0.1, method="rpy", damping=0.0, qnull=None):
    """One resolved-rate step: (qd, arrived) with qd = qnull + pinv(J(q)) (gain * e - J qnull), e and arrived as rtbhip.p_servo(fkine(q), Tep, gain,
    threshold, method).  (n,) and a bool for a 1-D q, (N, n) and (N,) booleans otherwise."""
    ets = _ets(robot)
    q2, T3, qn, single, tm = _shape(ets, q, Tep, qnull)
    qd, _, arrived, _ = launch(ets, q2, T3, qn, tm, method, gain, threshold, damping, 0.0, 1, True, False)
    if single:
        return qd[0], (arrived[0] if tm else bool(arrived[0]))
    return qd, arrived


def servo(robot, q, Tep, dt, steps, gain=1.0, threshold=0.1, method="rpy", damping=0.0, qnull=None):
    """The resolved-rate loop on the device: (q_out, arrived, its) after at most `steps` iterations of q <- q + dt * qd; a row stops after the
    step of the iteration in which it arrives.  Unbatched results for a 1-D q."""
    ets = _ets(robot)
    q2, T3, qn, single, tm = _shape(ets, q, Tep, qnull)
    _, qo, arrived, its = launch(ets, q2, T3, qn, tm, method, gain, threshold, damping, dt, steps, False, True)
    if single:
        return qo[0], (arrived[0] if tm else bool(arrived[0])), (its[0] if tm else int(its[0]))
    return qo, arrived, its


# ------------------------------------------------------------------------------------------------ the reactive QP servo (rtbhip_mmc)
def _limits(ets, qlim, qdlim):
    """-> (qlim (2, n), qdlim (n,) | None) as contiguous host float64"""
    n = ets.n
    host = lambda x: x.detach().cpu().numpy() if is_torch(x) else x
    ql = np.ascontiguousarray(np.asarray(ets.qlim if qlim is None else host(qlim), dtype=np.float64))
    if ql.shape != (2, n):
        raise ValueError("qlim must be (2, %d)" % n)
    qv = None
    if qdlim is not None:
        qv = np.asarray(host(qdlim), dtype=np.float64).reshape(-1)
        if qv.size == 1:
            qv = np.full(n, float(qv[0]))
        if qv.shape != (n,):
            raise ValueError("qdlim must be a scalar or (%d,)" % n)
        qv = np.ascontiguousarray(qv)
    return ql, qv


def launch_mmc(ets, q2, T3, tm, method, gain, threshold, dt, steps, Y, ks, km, ps, pi, damper_gain, qlim, qdlim, want_qd, want_q):
    """one launch -> (qd | None, q_out | None, arrived, its, status) in the memory q2 lives in"""
    N, n = q2.shape
    ql, qv = _limits(ets, qlim, qdlim)
    a = _lib.rtbhip_mmc_args()
    a.size = C.sizeof(_lib.rtbhip_mmc_args)
    a.method, a.chain, a.N, a.nTep = _method(method), ets._handle(), N, T3.shape[0]
    a.gain6 = (C.c_double * 6)(*_gain6(gain))
    a.threshold, a.dt, a.steps = float(threshold), float(dt), int(steps)
    a.Y, a.ks, a.km, a.ps, a.pi, a.damper_gain = float(Y), float(ks), float(km), float(ps), float(pi), float(damper_gain)
    a.qlim, a.qdlim = ql.ctypes.data, None if qv is None else qv.ctypes.data
    if tm:
        import torch
        _lib.note_device(q2)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=q2.device)
        qd, qo = (new((N, n), torch.float64) if w else None for w in (want_qd, want_q))
        arrived, its, status = new((N,), torch.uint8), new((N,), torch.int32), new((N,), torch.uint8)
        ptr = lambda x: None if x is None else x.data_ptr()
        a.q, a.Tep, a.qd, a.q_out, a.arrived, a.its, a.status = ptr(q2), ptr(T3), ptr(qd), ptr(qo), ptr(arrived), ptr(its), ptr(status)
        a.stream = _lib.current_stream_ptr().value
        check(lib().rtbhip_mmc(C.byref(a)))
        return qd, qo, arrived.bool(), its, status
    if N == 0:
        check(lib().rtbhip_mmc(C.byref(a)))
        return (np.empty((0, n)) if want_qd else None, np.empty((0, n)) if want_q else None, np.empty(0, dtype=bool), np.empty(0, dtype=np.int32),
                np.empty(0, dtype=np.uint8))
    st = _Staged()
    try:
        a.q, a.Tep = st.put(q2).value, st.put(T3).value
        pairs = [st.out((N, n)) if w else (None, None) for w in (want_qd, want_q)]
        words, bytes8 = (N + 1) // 2, (N + 7) // 8
        flags = st.out(words + 2 * bytes8)           # its (N int32), arrived and status (N bytes each) share one block of doubles
        base = flags[1].value
        a.qd, a.q_out = (None if p is None else p.value for _, p in pairs)
        a.its, a.arrived, a.status = base, base + 8 * words, base + 8 * (words + bytes8)
        check(lib().rtbhip_mmc(C.byref(a)))
        st.fetch()                                   # (a synchronous copy on the null stream: it waits for the launch)
    finally:
        st.free()
    raw = flags[0].view(np.uint8)
    its = raw[:4 * N].view(np.int32).copy()
    arrived = raw[8 * words:8 * words + N] != 0
    status = raw[8 * (words + bytes8):8 * (words + bytes8) + N].copy()
    return pairs[0][0], pairs[1][0], arrived, its, status


def mmc(robot, q, Tep, gain=1.0, threshold=0.1, method="rpy", Y=0.01, ks=1.0, km=1.0, ps=0.05, pi=0.9, damper_gain=1.0, qlim=None, qdlim=None):
    """One step of the reactive QP controller: (qd, arrived, status).  (n,), a bool and an int for a 1-D q; (N, n), (N,) booleans and (N,) uint8
    otherwise."""
    ets = _ets(robot)
    q2, T3, _, single, tm = _shape(ets, q, Tep, None)
    qd, _, arrived, _, status = launch_mmc(ets, q2, T3, tm, method, gain, threshold, 0.0, 1, Y, ks, km, ps, pi, damper_gain, qlim, qdlim, True, False)
    if single:
        return qd[0], (arrived[0] if tm else bool(arrived[0])), (status[0] if tm else int(status[0]))
    return qd, arrived, status


def mmc_servo(robot, q, Tep, dt, steps, gain=1.0, threshold=0.1, method="rpy", Y=0.01, ks=1.0, km=1.0, ps=0.05, pi=0.9, damper_gain=1.0, qlim=None,
              qdlim=None):
    """The reactive QP loop on the device: (q_out, arrived, its, status) after at most `steps` iterations of q <- q + dt * qd; a row stops after
    the step of the iteration in which it arrives.  Unbatched results for a 1-D q."""
    ets = _ets(robot)
    q2, T3, _, single, tm = _shape(ets, q, Tep, None)
    _, qo, arrived, its, status = launch_mmc(ets, q2, T3, tm, method, gain, threshold, dt, steps, Y, ks, km, ps, pi, damper_gain, qlim, qdlim, False, True)
    if single:
        return qo[0], (arrived[0] if tm else bool(arrived[0])), (its[0] if tm else int(its[0])), (status[0] if tm else int(status[0]))
    return qo, arrived, its, status


def joint_velocity_damper(robot, q, ps=0.05, pi=0.1, n=None, gain=1.0):
    """Robot.joint_velocity_damper (robot/Robot.py:1366-1421) restated on the host: (Ain (n, n), Bin (n,)) with Ain qd <= Bin -- one row per joint,
    the lower-limit test first and the upper-limit test second and overriding, as the reference has them.  A 2-D q gives a leading batch axis.
    (rtbhip.servo.mmc applies both sides of a joint instead: include/rtbhip.h.)"""
    ets = _ets(robot)
    n = ets.n if n is None else int(n)
    qlim = np.asarray(ets.qlim, dtype=np.float64)
    qa = np.asarray(q.detach().cpu().numpy() if is_torch(q) else q, dtype=np.float64)
    single = qa.ndim == 1
    qa = qa.reshape(-1, qa.shape[-1])
    Ain, Bin = np.zeros((qa.shape[0], n, n)), np.zeros((qa.shape[0], n))
    for r, qr in enumerate(qa):
        for i in range(n):
            if qr[i] - qlim[0, i] <= pi:
                Bin[r, i] = -gain * (((qlim[0, i] - qr[i]) + ps) / (pi - ps))
                Ain[r, i, i] = -1
            if qlim[1, i] - qr[i] <= pi:
                Bin[r, i] = gain * ((qlim[1, i] - qr[i]) - ps) / (pi - ps)
                Ain[r, i, i] = 1
    return (Ain[0], Bin[0]) if single else (Ain, Bin)
