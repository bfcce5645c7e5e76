"""Gradients of ETS.eval / fkine, ETS.jacob0 and the two-array ETS.fkine_jacob0 with respect to a CUDA q, and of DHRobot.rne (gravload, itorque) and
DHRobot.accel with respect to their CUDA inputs (torch.autograd).

Imported by rtbhip/et.py only when a call's q is a CUDA tensor with requires_grad while gradients are enabled (`_lib.wants_grad`), so torch is a
dependency of this module alone.  One Function: its forward is the ordinary call (gradients are off inside a Function's forward, so the
front end takes the path it always took), its backward one launch of rtbhip_fkine_jacob_vjp(_f32) on the current stream -- for fkine_jacob0
both outputs hang off one node, so a loss on T and J costs one backward launch.  The backward is not itself differentiable (no double
backward).  Not differentiable at all, and unchanged: jacobe, frame=1, packed=True, out=, hessian0, the ikine_* / IK_QP / IK_* class solvers.

Every link frame (rtbhip/et.py routes ETS.link_frames here, and with it the fkine_all of every robot class): _FramesVJP's backward is one launch of
rtbhip_link_frames_vjp for all the frames of the walk, float64.

The dynamics (rtbhip/dh.py routes here for all-revolute DH chains, never with base_wrench=True): _RneVJP's backward is one launch of
rtbhip_rne_vjp(_f32), which returns the gradients autograd asks for (ctx.needs_input_grad) and no others.  _AccelVJP needs no kernel of its
own: with qdd = accel(q, qd, torque) and g its incoming gradient, lambda = M^-1 g is one more accel call (qd = 0, no gravity; M is symmetric for
an all-revolute chain), the gradient of torque is lambda and those of q and qd are rne_vjp's at (q, qd, qdd) for gtau = -lambda (the implicit
function theorem on  rne(q, qd, qdd) = torque).

The dynamics of ETS / URDF robots (rtbhip/erobot.py routes here): _TreeRneVJP's backward is one launch of rtbhip_tree_rne_vjp -- every joint kind
the forward kernel serves, float64 -- and _TreeAccelVJP is _AccelVJP's construction on it, for robots numbered in group order (M symmetric).

The inertia matrix (rtbhip/dh.py and rtbhip/erobot.py route `inertia(q)` here: all-revolute DH chains, link trees numbered in group order; float64):
_InertiaVJP / _TreeInertiaVJP's backward is one launch of rtbhip_inertia_vjp / rtbhip_tree_inertia_vjp, which reads q and the incoming (N, n, n)
gradient once and writes gq once.

The Coriolis matrix (`coriolis(q, qd)`, the same robots, float64): _CoriolisVJP / _TreeCoriolisVJP's backward is one launch of rtbhip_coriolis_vjp /
rtbhip_tree_coriolis_vjp, which returns the gradients of q and qd that autograd asks for (ctx.needs_input_grad) and no others.

The inverse kinematics (rtbhip/et.py routes ETS.ik_LM / ik_GN / ik_NR here for a float64 Tep that asks for a gradient, when the mask uses no more
rows than the chain has joints): _IkVJP's forward is the ordinary solve, its backward one launch of rtbhip_ik_vjp -- the implicit-function
theorem at the returned q, J_a dq = nu_a, so  g_nu_a = (J_a J_a^T + d^2 I)^-1 J_a g_q  -- which returns the tangent-space gradient at Tep.
Rows that did not converge get zero; q0, the joint limits and the solver's own settings play no part."""
import torch
from torch.autograd.function import once_differentiable

from ._lib import check, lib, small, host_ptr, MEM_DEVICE, current_stream_ptr
import ctypes as C


def _ordinary(ets, what, q, base, tool):
    if what == "T":
        return ets.eval(q, base=base, tool=tool)
    if what == "J":
        return ets.jacob0(q, tool=tool)
    return ets.fkine_jacob0(q, base=base, tool=tool)


class _KinVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, ets, what, base, tool):
        ctx.set_materialize_grads(False)             # an output the loss does not use arrives as None: its pointer is NULL, nothing is read for it
        ctx.save_for_backward(q)
        ctx.ets, ctx.what, ctx.base, ctx.tool = ets, what, base, tool
        return _ordinary(ets, what, q, base, tool)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        (q,) = ctx.saved_tensors
        ets = ctx.ets
        gT = grads[0] if ctx.what in ("T", "TJ") else None
        gJ = grads[-1] if ctx.what in ("J", "TJ") else None
        if gT is None and gJ is None:
            return None, None, None, None, None
        q2, single, _ = ets._shape_q(q.detach(), f32_ok=True)          # the rows the forward read: (N, q_width), contiguous
        N, n = q2.shape[0], ets.n
        rows = lambda g, w: None if g is None else g.to(q2.dtype).reshape(N, w).contiguous()
        gT, gJ = rows(gT, 16), rows(gJ, 6 * n)
        gq = torch.empty_like(q2)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        fn = lib().rtbhip_fkine_jacob_vjp_f32 if q2.element_size() == 4 else lib().rtbhip_fkine_jacob_vjp
        check(fn(ets._handle(), ptr(q2), N, host_ptr(ctx.base), host_ptr(ctx.tool), ptr(gT), ptr(gJ), ptr(gq), MEM_DEVICE, current_stream_ptr()))
        if tuple(q.shape) != tuple(gq.shape):                          # q was one configuration, or rows wider than the chain reads
            full = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
            (full.reshape(1, -1) if single else full)[:, :q2.shape[1]] = gq
            gq = full
        return gq, None, None, None, None


def differentiable(ets, what, q, base, tool):
    """what: "T" (eval / fkine), "J" (jacob0) or "TJ" (fkine_jacob0): the call's result(s), attached to the autograd graph of q"""
    if ets.n == 0:                                   # a chain of constants: nothing depends on q, the ordinary call is the answer
        with torch.no_grad():
            return _ordinary(ets, what, q, base, tool)
    return _KinVJP.apply(q, ets, what, small(base, 16), small(tool, 16))


# ---------------------------------------------------------------- every link frame of a chain (ETS.link_frames, fkine_all)
class _FramesVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, ets, marks, base):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q)
        ctx.ets, ctx.marks, ctx.base = ets, marks, base
        return ets.link_frames(q, marks, base=base)

    @staticmethod
    @once_differentiable
    def backward(ctx, gF):
        (q,) = ctx.saved_tensors
        if gF is None:
            return None, None, None, None
        ets, marks = ctx.ets, ctx.marks
        q2, single, _ = ets._shape_q(q.detach())                       # the rows the forward read: (N, q_width), contiguous
        N = q2.shape[0]
        gF = gF.to(q2.dtype).reshape(N, len(marks), 16).contiguous()   # (a .sum() loss delivers a stride-0 expanded tensor)
        gq = torch.empty_like(q2)
        check(lib().rtbhip_link_frames_vjp(ets._handle(), C.c_void_p(q2.data_ptr()), N, host_ptr(ctx.base), host_ptr(marks), len(marks),
                                           C.c_void_p(gF.data_ptr()), C.c_void_p(gq.data_ptr()), MEM_DEVICE, current_stream_ptr()))
        if tuple(q.shape) != tuple(gq.shape):                          # q was one configuration, or rows wider than the chain reads
            full = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
            (full.reshape(1, -1) if single else full)[:, :q2.shape[1]] = gq
            gq = full
        return gq, None, None, None


def differentiable_link_frames(ets, q, marks, base):
    """ETS.link_frames(q, marks, base=) attached to the autograd graph of q: the backward pass is one launch of rtbhip_link_frames_vjp for all frames"""
    import numpy as np
    return _FramesVJP.apply(q, ets, np.ascontiguousarray(marks, dtype=np.int32).reshape(-1), small(base, 16))


# ---------------------------------------------------------------- the dynamics of a DH robot
def _rne_vjp(robot, q, qd, qdd, gtau, gravity, fext, want):
    """rtbhip_rne_vjp(_f32) on the current stream: the gradients named by `want` (three booleans), each shaped like its input; None for the others"""
    n = robot.n
    rows = lambda x: None if x is None else x.detach().reshape(-1, n).contiguous()
    q2, qd2, qdd2 = rows(q), rows(qd), rows(qdd)
    g2 = gtau.detach().to(q2.dtype).reshape(-1, n).contiguous()
    N = q2.shape[0]
    outs = [torch.empty_like(q2) if w else None for w in want]
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    fn = lib().rtbhip_rne_vjp_f32 if q2.element_size() == 4 else lib().rtbhip_rne_vjp
    f = None if fext is None else small(fext, 6)
    check(fn(robot._dyn_handle(), ptr(q2), ptr(qd2), ptr(qdd2), N, host_ptr(robot._gravity_c(gravity)), host_ptr(f), ptr(g2),
             ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), MEM_DEVICE, current_stream_ptr()))
    return [None if o is None else o.reshape(x.shape) for o, x in zip(outs, (q, qd, qdd))]


class _RneVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, qdd, robot, gravity, fext):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, qd, qdd)
        ctx.robot, ctx.gravity, ctx.fext = robot, gravity, fext
        return robot.rne(q, qd, qdd, gravity=gravity, fext=fext)

    @staticmethod
    @once_differentiable
    def backward(ctx, gtau):
        q, qd, qdd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:3]]
        if gtau is None or not any(want):
            return None, None, None, None, None, None
        gq, gqd, gqdd = _rne_vjp(ctx.robot, q, qd, qdd, gtau, ctx.gravity, ctx.fext, want)
        return gq, gqd, gqdd, None, None, None


class _AccelVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, torque, robot, gravity):
        ctx.set_materialize_grads(False)
        qdd = robot.accel(q, qd, torque, gravity=gravity)
        ctx.save_for_backward(q, qd, qdd)
        ctx.robot, ctx.gravity = robot, gravity
        return qdd

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, qd, qdd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:3]]
        if g is None or not any(want):
            return None, None, None, None, None
        lam = ctx.robot.accel(q.detach(), torch.zeros_like(qd), g.to(q.dtype).reshape(q.shape).contiguous(), gravity=[0.0, 0.0, 0.0])       # M^-1 g
        gq = gqd = None
        if want[0] or want[1]:
            gq, gqd, _ = _rne_vjp(ctx.robot, q, qd, qdd, -lam, ctx.gravity, None, [want[0], want[1], False])
        return gq, gqd, (lam.reshape(q.shape) if want[2] else None), None, None


def differentiable_rne(robot, q, qd, qdd, gravity, fext):
    """DHRobot.rne(q, qd, qdd, gravity=, fext=) attached to the autograd graph of its tensor inputs (qd / qdd may be None)"""
    return _RneVJP.apply(q, qd, qdd, robot, gravity, fext)


def differentiable_accel(robot, q, qd, torque, gravity):
    """DHRobot.accel(q, qd, torque, gravity=) attached to the autograd graph of its inputs"""
    return _AccelVJP.apply(q, qd, torque, robot, gravity)


# ---------------------------------------------------------------- the dynamics of an ETS / URDF robot (link tree)
def _tree_rne_vjp(robot, q, qd, qdd, gtau, gravity, want):
    """rtbhip_tree_rne_vjp on the current stream: the gradients named by `want` (three booleans), each shaped like its input; None for the others"""
    import numpy as np
    n = robot.n
    rows = lambda x: None if x is None else x.detach().reshape(-1, n).contiguous()
    q2, qd2, qdd2 = rows(q), rows(qd), rows(qdd)
    g2 = gtau.detach().to(q2.dtype).reshape(-1, n).contiguous()
    N = q2.shape[0]
    outs = [torch.empty_like(q2) if w else None for w in want]
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    g = np.ascontiguousarray(robot.gravity if gravity is None else np.asarray(gravity, dtype=np.float64).reshape(3))
    check(lib().rtbhip_tree_rne_vjp(robot._handle(), ptr(q2), ptr(qd2), ptr(qdd2), N, host_ptr(g), ptr(g2), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                    MEM_DEVICE, current_stream_ptr()))
    return [None if o is None else o.reshape(x.shape) for o, x in zip(outs, (q, qd, qdd))]


class _TreeRneVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, qdd, robot, gravity):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, qd, qdd)
        ctx.robot, ctx.gravity = robot, gravity
        return robot.rne(q, qd, qdd, gravity=gravity)

    @staticmethod
    @once_differentiable
    def backward(ctx, gtau):
        q, qd, qdd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:3]]
        if gtau is None or not any(want):
            return None, None, None, None, None
        gq, gqd, gqdd = _tree_rne_vjp(ctx.robot, q, qd, qdd, gtau, ctx.gravity, want)
        return gq, gqd, gqdd, None, None


class _TreeAccelVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, torque, robot, gravity):
        ctx.set_materialize_grads(False)
        qdd = robot.accel(q, qd, torque, gravity=gravity)
        ctx.save_for_backward(q, qd, qdd)
        ctx.robot, ctx.gravity = robot, gravity
        return qdd

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, qd, qdd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:3]]
        if g is None or not any(want):
            return None, None, None, None, None
        lam = ctx.robot.accel(q.detach(), torch.zeros_like(qd), g.to(q.dtype).reshape(q.shape).contiguous(), gravity=[0.0, 0.0, 0.0])       # M^-1 g
        gq = gqd = None
        if want[0] or want[1]:
            gq, gqd, _ = _tree_rne_vjp(ctx.robot, q, qd, qdd, -lam, ctx.gravity, [want[0], want[1], False])
        return gq, gqd, (lam.reshape(q.shape) if want[2] else None), None, None


def differentiable_tree_rne(robot, q, qd, qdd, gravity):
    """ERobot.rne(q, qd, qdd, gravity=) attached to the autograd graph of its tensor inputs (qd / qdd may be None)"""
    return _TreeRneVJP.apply(q, qd, qdd, robot, gravity)


def differentiable_tree_accel(robot, q, qd, torque, gravity):
    """ERobot.accel(q, qd, torque, gravity=) attached to the autograd graph of its inputs (robots numbered in group order)"""
    return _TreeAccelVJP.apply(q, qd, torque, robot, gravity)


# ---------------------------------------------------------------- the joint-space inertia matrix, DH robots and link trees
def _inertia_vjp(fn, handle, n, q, gM):
    """rtbhip_inertia_vjp / rtbhip_tree_inertia_vjp on the current stream: the gradient of q, shaped like q"""
    q2 = q.detach().reshape(-1, n).contiguous()
    N = q2.shape[0]
    g2 = gM.detach().to(q2.dtype).reshape(N, n, n).contiguous()          # (a .sum() loss delivers a stride-0 expanded tensor)
    gq = torch.empty_like(q2)
    check(fn(handle, C.c_void_p(q2.data_ptr()), N, C.c_void_p(g2.data_ptr()), C.c_void_p(gq.data_ptr()), MEM_DEVICE, current_stream_ptr()))
    return gq.reshape(q.shape)


class _InertiaVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, robot):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q)
        ctx.robot = robot
        return robot.inertia(q)

    @staticmethod
    @once_differentiable
    def backward(ctx, gM):
        (q,) = ctx.saved_tensors
        if gM is None:
            return None, None
        return _inertia_vjp(lib().rtbhip_inertia_vjp, ctx.robot._dyn_handle(), ctx.robot.n, q, gM), None


class _TreeInertiaVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, robot):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q)
        ctx.robot = robot
        return robot.inertia(q)

    @staticmethod
    @once_differentiable
    def backward(ctx, gM):
        (q,) = ctx.saved_tensors
        if gM is None:
            return None, None
        return _inertia_vjp(lib().rtbhip_tree_inertia_vjp, ctx.robot._handle(), ctx.robot.n, q, gM), None


def differentiable_inertia(robot, q):
    """DHRobot.inertia(q) attached to the autograd graph of q (all-revolute chains): the backward pass is one launch of rtbhip_inertia_vjp"""
    return _InertiaVJP.apply(q, robot)


def differentiable_tree_inertia(robot, q):
    """ERobot.inertia(q) attached to the autograd graph of q (robots numbered in group order): the backward pass is one launch of rtbhip_tree_inertia_vjp"""
    return _TreeInertiaVJP.apply(q, robot)


# ---------------------------------------------------------------- the Coriolis / centripetal matrix, DH robots and link trees
def _coriolis_vjp(fn, handle, n, q, qd, gC, want):
    """rtbhip_coriolis_vjp / rtbhip_tree_coriolis_vjp on the current stream: the gradients of q and qd named by `want`, each shaped like its input"""
    q2 = q.detach().reshape(-1, n).contiguous()
    qd2 = qd.detach().to(q2.dtype).reshape(-1, n).contiguous()
    N = q2.shape[0]
    g2 = gC.detach().to(q2.dtype).reshape(N, n, n).contiguous()          # (a .sum() loss delivers a stride-0 expanded tensor)
    outs = [torch.empty_like(q2) if w else None for w in want]
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    check(fn(handle, ptr(q2), ptr(qd2), N, ptr(g2), ptr(outs[0]), ptr(outs[1]), MEM_DEVICE, current_stream_ptr()))
    return [None if o is None else o.reshape(x.shape) for o, x in zip(outs, (q, qd))]


class _CoriolisVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, robot):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, qd)
        ctx.robot = robot
        return robot.coriolis(q, qd)

    @staticmethod
    @once_differentiable
    def backward(ctx, gC):
        q, qd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:2]]
        if gC is None or not any(want):
            return None, None, None
        gq, gqd = _coriolis_vjp(lib().rtbhip_coriolis_vjp, ctx.robot._dyn_handle(), ctx.robot.n, q, qd, gC, want)
        return gq, gqd, None


class _TreeCoriolisVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qd, robot):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, qd)
        ctx.robot = robot
        return robot.coriolis(q, qd)

    @staticmethod
    @once_differentiable
    def backward(ctx, gC):
        q, qd = ctx.saved_tensors
        want = [bool(w) for w in ctx.needs_input_grad[:2]]
        if gC is None or not any(want):
            return None, None, None
        gq, gqd = _coriolis_vjp(lib().rtbhip_tree_coriolis_vjp, ctx.robot._handle(), ctx.robot.n, q, qd, gC, want)
        return gq, gqd, None


def differentiable_coriolis(robot, q, qd):
    """DHRobot.coriolis(q, qd) attached to the autograd graph of q and qd (all-revolute chains): the backward pass is one launch of rtbhip_coriolis_vjp"""
    return _CoriolisVJP.apply(q, qd, robot)


def differentiable_tree_coriolis(robot, q, qd):
    """ERobot.coriolis(q, qd) attached to the autograd graph of q and qd (robots numbered in group order): the backward pass is one launch of
    rtbhip_tree_coriolis_vjp"""
    return _TreeCoriolisVJP.apply(q, qd, robot)


# ---------------------------------------------------------------- the inverse kinematics (ETS.ik_LM / ik_GN / ik_NR)
class _IkVJP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Tep, ets, args, mask, damping):
        ctx.set_materialize_grads(False)
        _, q, ok, it, se, E = ets._ik(Tep, *args)          # the ordinary call (gradients are off in here), flavour 0
        ctx.mark_non_differentiable(ok, it, se, E)
        ctx.save_for_backward(q, Tep, ok)
        ctx.ets, ctx.mask, ctx.damping = ets, mask, damping
        return q, ok, it, se, E

    @staticmethod
    @once_differentiable
    def backward(ctx, gq, *_):
        q, Tep, ok = ctx.saved_tensors
        if gq is None:
            return None, None, None, None, None
        N, n = q.shape
        Tq = Tep.detach().reshape(N, 16).contiguous()
        g = gq.to(q.dtype).reshape(N, n).contiguous()      # (a .sum() loss delivers a stride-0 expanded tensor)
        gT = torch.empty_like(Tq)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        check(lib().rtbhip_ik_vjp(ctx.ets._handle(), ptr(q), N, ptr(Tq), ptr(ok), host_ptr(ctx.mask), ctx.damping, ptr(g), ptr(gT), None,
                                  current_stream_ptr()))
        return gT.reshape(Tep.shape), None, None, None, None


def differentiable_ik(ets, Tep, args, grad_damping):
    """ets._ik(Tep, *args) of the three C-loop solvers attached to the autograd graph of Tep -> (single, q, success, iterations, searches,
    residual): the backward pass is one launch of rtbhip_ik_vjp; args[4] is the mask"""
    return (Tep.dim() == 2,) + _IkVJP.apply(Tep, ets, args, small(args[4], 6), float(grad_damping))
