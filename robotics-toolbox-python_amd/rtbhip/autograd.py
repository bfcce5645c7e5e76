"""Gradients of ETS.eval / fkine, ETS.jacob0 and the two-array ETS.fkine_jacob0 with respect to a CUDA q (torch.autograd).

Imported by rtbhip/et.py only when a call's q is a CUDA tensor with requires_grad while gradients are enabled (`_lib.wants_grad`), so torch is a
dependency of this module alone.  One Function: its forward is the ordinary call (gradients are off inside a Function's forward, so the
front end takes the path it always took), its backward one launch of rtbhip_fkine_jacob_vjp(_f32) on the current stream -- for fkine_jacob0
both outputs hang off one node, so a loss on T and J costs one backward launch.  The backward is not itself differentiable (no double
backward).  Not differentiable at all, and unchanged: jacobe, frame=1, packed=True, out=, hessian0, the IK solvers, the dynamics."""
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
