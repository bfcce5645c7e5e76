"""Operational-space dynamics of a robot with inertial parameters (DHRobot, ERobot and the models built on them): the reference's
Dynamics.inertia_x and gravload_x (robot/Dynamics.py:924-1025, 1173-1290) and Asada's manipulability measure (robot/Robot.py:871-881), each ONE
launch of rtbhip_opspace / rtbhip_tree_opspace on the Jacobian the existing jacob0 / jacob0_analytical launch returned:

    rtbhip.opspace.inertia_x(robot, q, pinv=False, representation="rpy/xyz", Ji=None)
    rtbhip.opspace.gravload_x(robot, q, gravity=None, pinv=False, representation="rpy/xyz", Ji=None)
    rtbhip.opspace.manipulability(robot, q, J=None, method="asada", axes="all")

The arguments after `robot` are the reference methods' own.  They are functions of this module, not yet methods of the robot classes: the
reference's own test files run against those classes with a ledger of the tests that must NOT pass (tests/test_reference_suite.py), and its
test_inertia_x / test_asada are in it; binding the functions as methods goes with the ledger change.  A robot class provides
`_opspace_call()` -> (entry point, handle), `_opspace_gravity(gravity)` -> the host gravity vector its rne hands the library and
`_opspace_ets(end)` -> the end-effector chain; DHRobot and ERobot do.

CUDA float64 tensors in give tensors out on the current stream.  NumPy in gives NumPy out, staged through the ABI's own device-memory helpers
(rtbhip_device_alloc / _copy / _free; synchronous copies): correct, not fast.  float32 tensors are refused as elsewhere.  No gradients: under
requires_grad the call behaves as with a plain tensor."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, as_numeric, host_ptr, is_torch

MX, GX, ASADA = 1, 2, 4


def shape_q(robot, q):
    """-> (q as (N, n) contiguous, single, torch?)"""
    if not hasattr(robot, "_opspace_call"):
        raise TypeError("%s has no dynamics: the operational-space quantities need a robot with inertial parameters (DHRobot, ERobot)" % type(robot).__name__)
    n = robot.n
    if q is None:
        q = getattr(robot, "q", None)
        if q is None:
            raise ValueError("q must be supplied")
    if is_torch(q) and q.is_cuda:
        _lib.device_dtype([q])
        q = q.detach()
        single = q.dim() == 1
        q2 = q.reshape(-1, n).contiguous()
        return q2, single or q2.shape[0] == 1, True
    if is_torch(q):
        q = q.detach().numpy()
    a = as_numeric(q)
    q2 = np.ascontiguousarray(a.reshape(-1, n))
    return q2, a.ndim == 1 or q2.shape[0] == 1, False


def _shape_J(J, N, n, tm):
    if tm:
        if not (is_torch(J) and J.is_cuda):
            raise ValueError("q and J must both be host arrays or both be CUDA tensors")
        _lib.device_dtype([J])
        J3 = J.detach().reshape(-1, 6, n)
        if J3.shape[0] == 1 and N > 1:
            J3 = J3.expand(N, 6, n)
        J3 = J3.contiguous()
    else:
        if is_torch(J):
            if J.is_cuda:
                raise ValueError("q and J must both be host arrays or both be CUDA tensors")
            J = J.detach().numpy()
        J3 = as_numeric(J, "J").reshape(-1, 6, n)
        if J3.shape[0] == 1 and N > 1:
            J3 = np.broadcast_to(J3, (N, 6, n))
        J3 = np.ascontiguousarray(J3)
    if tuple(J3.shape) != (N, 6, n):
        raise ValueError("J must be (6, %d) or (%d, 6, %d)" % (n, N, n))
    return J3


class _Staged:
    """host arrays on the device for one call: rtbhip_device_alloc / _copy / _free"""

    def __init__(self):
        self.dev, self.blocks, self.outs = 0, [], []
        try:
            import torch
            if torch.cuda.is_available():
                self.dev = torch.cuda.current_device()
        except ImportError:
            pass

    def _alloc(self, nbytes):
        p = C.c_void_p()
        check(lib().rtbhip_device_alloc(self.dev, int(nbytes), C.byref(p)))
        self.blocks.append(p)
        return p

    def put(self, a):
        p = self._alloc(a.nbytes)
        check(lib().rtbhip_device_copy(p, host_ptr(a), a.nbytes, 1, None))
        return p

    def out(self, shape):
        a = np.empty(shape, dtype=np.float64)
        p = self._alloc(a.nbytes)
        self.outs.append((a, p))
        return a, p

    def fetch(self):
        for a, p in self.outs:
            check(lib().rtbhip_device_copy(host_ptr(a), p, a.nbytes, 2, None))

    def free(self):
        for p in self.blocks:
            lib().rtbhip_device_free(p)
        self.blocks = []


def launch(robot, q2, J3, tm, gravity, axes_mask, want):
    """one launch -> (Mx (N, 6, 6) | None, Gx (N, 6) | None, asada (N,) | None) in the memory q2 / J3 live in"""
    fn, handle = robot._opspace_call()
    N = q2.shape[0]
    g = np.ascontiguousarray(robot._opspace_gravity(gravity), dtype=np.float64) if want & GX else None
    shapes = [(N, 6, 6) if want & MX else None, (N, 6) if want & GX else None, (N,) if want & ASADA else None]
    if tm:
        import torch
        _lib.note_device(q2)
        outs = [None if s is None else torch.empty(s, dtype=torch.float64, device=q2.device) for s in shapes]
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        check(fn(handle, ptr(q2), ptr(J3), N, host_ptr(g), axes_mask, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), _lib.current_stream_ptr()))
        return outs
    st = _Staged()
    try:
        dq, dJ = st.put(q2), st.put(J3)
        pairs = [(None, None) if s is None else st.out(s) for s in shapes]
        check(fn(handle, dq, dJ, N, host_ptr(g), axes_mask, pairs[0][1], pairs[1][1], pairs[2][1], None))
        st.fetch()                               # (a synchronous copy on the null stream: it waits for the launch)
    finally:
        st.free()
    return [a for a, _ in pairs]


def _transpose(x):
    return x.transpose(-1, -2) if is_torch(x) else np.swapaxes(x, -1, -2)


def _jacobian(robot, q, representation, end):
    ets = robot._opspace_ets(end)
    if ets.n != robot.n:
        raise ValueError("the end-effector path moves %d of the robot's %d joints: the operational-space quantities need all of them" % (ets.n, robot.n))
    if representation is None:                   # the geometric Jacobian, as in the reference's test
        return ets.jacob0(q, tool=robot._kin_tool())
    return ets.jacob0_analytical(q, representation=representation, tool=robot._kin_tool())


def inertia_x(robot, q=None, pinv=False, representation="rpy/xyz", Ji=None, end=None):
    """Operational-space inertia matrix Mx = J^-T M(q) J^-1: (6,6), or (N,6,6) for a 2-D q (Dynamics.inertia_x, robot/Dynamics.py:924-1025).
    J is jacob0_analytical(q, representation) -- representation=None: the geometric jacob0, as in the reference's test -- inverted for six
    joints, pseudo-inverted otherwise; `pinv=True` is the same matrix at full rank, and a six-joint arm is served by the inverse (pivoted LU)
    either way.  With Ji= (the caller's inverse, (n,6)) the result is Ji.T @ inertia(q) @ Ji on the host or in torch.  A rank-deficient J gives a
    non-finite or huge row: numpy's truncated pinv is not reproduced.  `end` (link trees): the end-effector link; its path must move all n
    joints, ValueError otherwise."""
    if Ji is not None:
        M = robot.inertia(q.detach() if is_torch(q) else q)
        Ji = Ji if is_torch(M) else as_numeric(Ji.detach().cpu().numpy() if is_torch(Ji) else Ji, "Ji")
        return _transpose(Ji) @ M @ Ji
    q2, single, tm = shape_q(robot, q)
    J3 = _shape_J(_jacobian(robot, q2, representation, end), q2.shape[0], robot.n, tm)
    Mx = launch(robot, q2, J3, tm, None, 63, MX)[0]
    return Mx[0] if single else Mx


def gravload_x(robot, q=None, gravity=None, pinv=False, representation="rpy/xyz", Ji=None, end=None):
    """Operational-space gravity wrench Gx = J^-T g(q): (6,), or (N,6) for a 2-D q and any n (Dynamics.gravload_x, robot/Dynamics.py:1173-1290,
    whose trajectory branch allocates (m,n) and so only runs at n = 6).  Arguments as inertia_x; `gravity` as gravload's.  With Ji= the result is
    Ji.T @ gravload(q, gravity)."""
    if Ji is not None:
        G = robot.gravload(q.detach() if is_torch(q) else q, gravity=gravity)
        Ji = Ji if is_torch(G) else as_numeric(Ji.detach().cpu().numpy() if is_torch(Ji) else Ji, "Ji")
        return (_transpose(Ji) @ G[..., None])[..., 0]
    q2, single, tm = shape_q(robot, q)
    J3 = _shape_J(_jacobian(robot, q2, representation, end), q2.shape[0], robot.n, tm)
    Gx = launch(robot, q2, J3, tm, gravity, 63, GX)[1]
    return Gx[0] if single else Gx


def manipulability(robot, q=None, J=None, end=None, start=None, method="asada", axes="all"):
    """Asada's measure (robot/Robot.py:871-881): lambda_min / lambda_max of the rows and columns of pinv(J)^T M(q) pinv(J) that `axes` selects
    ("all" / "trans" / "rot" / six booleans; "both": the pair), 0 where J has not full rank (always below six joints): a scalar, or (N,) for a
    2-D q.  J is the geometric jacob0 of the path -- or the caller's J= ((6,n) or (N,6,n)), with q for M(q)."""
    if not (isinstance(method, str) and method.lower().startswith("asa")):
        raise ValueError("rtbhip.opspace.manipulability serves method=\"asada\"; the other measures are robot.manipulability's")
    from .et import ETS
    if isinstance(axes, str) and axes == "both":
        return (manipulability(robot, q, J, end, start, method, "trans"), manipulability(robot, q, J, end, start, method, "rot"))
    if q is None:
        raise ValueError("Asada's measure needs q for the inertia matrix, also when J is supplied")
    mask = ETS._axes_mask(axes)
    if mask == 0:
        raise ValueError("axes selects no task-space row")
    q2, single, tm = shape_q(robot, q)
    if J is None:
        ets = robot._opspace_ets(end) if start is None else robot._path(start, end)
        if ets.n != robot.n:
            raise ValueError("the path moves %d of the robot's %d joints: Asada's measure needs all of them" % (ets.n, robot.n))
        J = ets.jacob0(q2, tool=robot._kin_tool())
    J3 = _shape_J(J, q2.shape[0], robot.n, tm)
    w = launch(robot, q2, J3, tm, None, mask, ASADA)[2]
    return (w[0] if tm else float(w[0])) if single else w
