"""-m "not gpu": what the C ABI REFUSES, call by call, through the raw library (rtbhip._lib.lib()): the return code and the FULL text of
rtbhip_last_error() of every compute entry point include/rtbhip.h declares, and RTBHIP_OK for an empty batch.  The order of the checks
is behaviour: the rows with two wrong arguments pin which refusal comes first.  The expected texts were recorded from the library, not
derived from its source; nothing here dereferences a buffer (every refusal, and the empty batch, returns before the device is touched),
so no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib

OK, EINVAL, ELIMIT = 0, -1, -3
HOST, DEV = 0, 1
BAD = 987654321            # no such handle of any kind
A, MIS = 0x1000, 0x1008    # "device" addresses for the alignment refusals, which come before any dereference: 16-byte aligned / not


class Ctx:
    """Handles and host buffers the rows refer to by name."""

    def __init__(self):
        ET = rtbhip.ET
        self._keep = [rtbhip.models.Panda().ets(), ET.Rz(jindex=2) * ET.tx(1.0) * ET.Ry(jindex=0), ET.tx(0.5) * ET.Rx(0.25),
                      rtbhip.models.DH.Panda(), rtbhip.urdf.load("Panda").erobot()]
        self.c = self._keep[0]._handle()          # Panda: n = q_width = 7
        self.cw = self._keep[1]._handle()         # n = 2, q_width = 3
        self.c0 = self._keep[2]._handle()         # a chain of constants: n = 0
        self._long = [rtbhip.ETS([ET.Rz() if j % 2 else ET.Ry() for j in range(n)]) for n in (15, 16, 32)]
        self.c15, self.c16, self.c32 = (e._handle() for e in self._long)      # chains of 15, 16 and 32 joints
        self.d = self._keep[3]._dyn_handle()
        self.t = self._keep[4]._handle()
        self._buf = np.zeros(4096)
        self.B = self._buf.ctypes.data            # a valid host address wherever a pointer must not be NULL
        self._ones = np.ones(32)
        self.one = self._ones.ctypes.data         # gains / influence distances: all 1.0
        self._marks = (C.c_int32 * 2)(0, 1)
        self.marks = C.addressof(self._marks)
        # fleet arguments: two Panda chains
        self.h2 = (C.c_uint64 * 2)(self.c, self.c)
        self.hbad = (C.c_uint64 * 2)(self.c, BAD)
        self.p2 = (C.c_void_p * 2)(self.B, self.B)
        self.pnull = (C.c_void_p * 2)(self.B, None)
        self.n0 = (C.c_int64 * 2)(0, 0)
        self.n2 = (C.c_int64 * 2)(2, 2)
        self.nneg = (C.c_int64 * 2)(2, -1)
        self.hbad0 = (C.c_uint64 * 2)(BAD, self.c)
        self.nneg0 = (C.c_int64 * 2)(-1, 2)
        self.n20 = (C.c_int64 * 2)(2, 0)
        self.pnull0 = (C.c_void_p * 2)(None, self.B)


# (id, entry point, arguments given the Ctx, return code, rtbhip_last_error() -- None: not looked at, the call succeeds)
def _kin_rows():
    rows = []
    # name -> arguments from (handle, q, N, frame, outputs..., mem)
    forms = {
        "fkine": lambda h, q, N, fr, o, mem: (h, q, N, None, None, o, mem, None),
        "jacob": lambda h, q, N, fr, o, mem: (h, q, N, None, fr, o, mem, None),
        "fkine_jacob": lambda h, q, N, fr, o, mem: (h, q, N, None, None, fr, o, o, mem, None),
        "fkine_jacob_packed": lambda h, q, N, fr, o, mem: (h, q, N, None, None, fr, o, mem, None),
        "fkine_jacob_f32": lambda h, q, N, fr, o, mem: (h, q, N, None, None, fr, o, o, mem, None),
        "fkine_jacob_packed_f32": lambda h, q, N, fr, o, mem: (h, q, N, None, None, fr, o, mem, None),
        "hessian": lambda h, q, N, fr, o, mem: (h, q, N, None, fr, o, mem, None),
    }
    for name, f in forms.items():
        m = DEV if name.endswith("f32") else HOST
        add = lambda tag, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
        add("unknown", lambda x, f=f, m=m: f(BAD, x.B, 4, 0, x.B, m))
        add("negN", lambda x, f=f, m=m: f(x.c, x.B, -1, 0, x.B, m))
        add("nullq", lambda x, f=f, m=m: f(x.c, None, 4, 0, x.B, m))
        add("mem7", lambda x, f=f: f(x.c, x.B, 4, 0, x.B, 7))
        add("nullout", lambda x, f=f, m=m: f(x.c, x.B, 4, 0, None, m))
        if name != "fkine":
            add("frame3", lambda x, f=f, m=m: f(x.c, x.B, 4, 3, x.B, m))
            add("frame3+nullout", lambda x, f=f, m=m: f(x.c, x.B, 4, 3, None, m))
        add("unknown+negN", lambda x, f=f, m=m: f(BAD, x.B, -1, 0, x.B, m))
        add("mem7+nullq", lambda x, f=f: f(x.c, None, 4, 0, x.B, 7))
        if name.endswith("f32"):
            add("hostmem", lambda x, f=f: f(x.c, x.B, 4, 0, x.B, HOST))
            add("hostmem+frame3", lambda x, f=f: f(x.c, x.B, 4, 3, x.B, HOST))
            add("hostmem-empty", lambda x, f=f: f(x.c, x.B, 0, 0, x.B, HOST))
        add("empty", lambda x, f=f, m=m: f(x.c, x.B, 0, 0, x.B, m))
        add("empty-null", lambda x, f=f, m=m: f(x.c, None, 0, 0, None, m))
    return rows


def _diff_rows():
    rows = []
    forms = {       # (handle, q, qd, N, frame, sel (axes / representation / method), out, mem)
        "jacob_dot": lambda h, q, qd, N, fr, sel, o, mem: (h, q, qd, N, None, fr, o, mem, None),
        "jacob0_analytical": lambda h, q, qd, N, fr, sel, o, mem: (h, q, N, None, sel, o, mem, None),
        "jacob0_dot_analytical": lambda h, q, qd, N, fr, sel, o, mem: (h, q, qd, N, None, sel, o, mem, None),
        "manipulability": lambda h, q, qd, N, fr, sel, o, mem: (h, q, N, None, 63, sel, o, mem, None),
        "jacobm": lambda h, q, qd, N, fr, sel, o, mem: (h, q, N, None, sel if sel else 63, o, mem, None),
    }
    for name, f in forms.items():
        add = lambda tag, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
        add("unknown", lambda x, f=f: f(BAD, x.B, x.B, 4, 0, 0, x.B, HOST))
        add("negN", lambda x, f=f: f(x.c, x.B, x.B, -1, 0, 0, x.B, HOST))
        add("nullq", lambda x, f=f: f(x.c, None, x.B, 4, 0, 0, x.B, HOST))
        add("mem7", lambda x, f=f: f(x.c, x.B, x.B, 4, 0, 0, x.B, 7))
        add("nullout", lambda x, f=f: f(x.c, x.B, x.B, 4, 0, 0, None, HOST))
        add("unknown+mem7", lambda x, f=f: f(BAD, x.B, x.B, 4, 0, 0, x.B, 7))
        add("negN+nullout", lambda x, f=f: f(x.c, x.B, x.B, -1, 0, 0, None, HOST))
        add("empty", lambda x, f=f: f(x.c, x.B, x.B, 0, 0, 0, x.B, HOST))
        add("empty-dev", lambda x, f=f: f(x.c, None, None, 0, 0, 0, None, DEV))
    add = lambda tag, name, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
    add("frame3", "jacob_dot", lambda x: (x.c, x.B, x.B, 4, None, 3, x.B, HOST, None))
    add("nullqd", "jacob_dot", lambda x: (x.c, x.B, None, 4, None, 0, x.B, HOST, None))
    add("frame3+nullqd", "jacob_dot", lambda x: (x.c, x.B, None, 4, None, 3, x.B, HOST, None))
    add("nullqd", "jacob0_dot_analytical", lambda x: (x.c, x.B, None, 4, None, 0, x.B, HOST, None))
    for nm in ("jacob0_analytical", "jacob0_dot_analytical"):
        for rep in (-1, 4):
            if nm == "jacob0_analytical":
                add("rep%d" % rep, nm, lambda x, rep=rep: (x.c, x.B, 4, None, rep, x.B, HOST, None))
                add("rep%d+unknown" % rep, nm, lambda x, rep=rep: (BAD, x.B, 4, None, rep, x.B, HOST, None))
            else:
                add("rep%d" % rep, nm, lambda x, rep=rep: (x.c, x.B, x.B, 4, None, rep, x.B, HOST, None))
    for meth in (-1, 3):
        add("method%d" % meth, "manipulability", lambda x, meth=meth: (x.c, x.B, 4, None, 63, meth, x.B, HOST, None))
    add("method3+unknown", "manipulability", lambda x: (BAD, x.B, 4, None, 63, 3, x.B, HOST, None))
    add("noaxes", "manipulability", lambda x: (x.c, x.B, 4, None, 0, 0, x.B, HOST, None))
    add("noaxes64", "manipulability", lambda x: (x.c, x.B, 4, None, 64, 0, x.B, HOST, None))
    add("noaxes", "jacobm", lambda x: (x.c, x.B, 4, None, 0, x.B, HOST, None))
    add("noaxes+nullout", "jacobm", lambda x: (x.c, x.B, 4, None, 0, None, HOST, None))
    return rows


def _from_jacobian_rows():
    rows = []
    add = lambda tag, name, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
    hj = "hessian_from_jacobian"          # (J, N, n, H, mem, stream)
    add("negN", hj, lambda x: (x.B, -1, 7, x.B, HOST, None))
    add("nullJ", hj, lambda x: (None, 4, 7, x.B, HOST, None))
    add("mem7", hj, lambda x: (x.B, 4, 7, x.B, 7, None))
    add("n0", hj, lambda x: (x.B, 4, 0, x.B, HOST, None))
    add("n33", hj, lambda x: (x.B, 4, 33, x.B, HOST, None))
    add("nullH", hj, lambda x: (x.B, 4, 7, None, HOST, None))
    add("misaligned-J", hj, lambda x: (MIS, 4, 7, A, DEV, None))
    add("misaligned-H", hj, lambda x: (A, 4, 7, MIS, DEV, None))
    add("negN+n0", hj, lambda x: (x.B, -1, 0, x.B, HOST, None))
    add("n0+nullH", hj, lambda x: (x.B, 4, 0, None, HOST, None))
    add("empty", hj, lambda x: (x.B, 0, 7, x.B, HOST, None))
    add("empty-dev", hj, lambda x: (None, 0, 7, None, DEV, None))
    mj = "manipulability_from_jacobian"   # (J, N, n, axes, method, m, mem, stream)
    add("negN", mj, lambda x: (x.B, -1, 7, 63, 0, x.B, HOST, None))
    add("nullJ", mj, lambda x: (None, 4, 7, 63, 0, x.B, HOST, None))
    add("mem7", mj, lambda x: (x.B, 4, 7, 63, 0, x.B, 7, None))
    add("n0", mj, lambda x: (x.B, 4, 0, 63, 0, x.B, HOST, None))
    add("n17", mj, lambda x: (x.B, 4, 17, 63, 0, x.B, HOST, None))
    add("noaxes", mj, lambda x: (x.B, 4, 7, 0, 0, x.B, HOST, None))
    add("method-1", mj, lambda x: (x.B, 4, 7, 63, -1, x.B, HOST, None))
    add("method3", mj, lambda x: (x.B, 4, 7, 63, 3, x.B, HOST, None))
    add("nullout", mj, lambda x: (x.B, 4, 7, 63, 0, None, HOST, None))
    add("misaligned", mj, lambda x: (MIS, 4, 7, 63, 0, A, DEV, None))
    add("method3+n0", mj, lambda x: (x.B, 4, 0, 63, 3, x.B, HOST, None))
    add("n0+noaxes", mj, lambda x: (x.B, 4, 0, 0, 0, x.B, HOST, None))
    add("noaxes+negN", mj, lambda x: (x.B, -1, 7, 0, 0, x.B, HOST, None))
    add("nullout+mem7", mj, lambda x: (x.B, 4, 7, 63, 0, None, 7, None))
    add("empty", mj, lambda x: (x.B, 0, 7, 63, 0, x.B, HOST, None))
    jj = "jacobm_from_jacobian"           # (J, H, N, n, axes, Jm, mem, stream)
    add("negN", jj, lambda x: (x.B, None, -1, 7, 63, x.B, HOST, None))
    add("nullJ", jj, lambda x: (None, None, 4, 7, 63, x.B, HOST, None))
    add("mem7", jj, lambda x: (x.B, None, 4, 7, 63, x.B, 7, None))
    add("n17", jj, lambda x: (x.B, None, 4, 17, 63, x.B, HOST, None))
    add("noaxes", jj, lambda x: (x.B, None, 4, 7, 64, x.B, HOST, None))
    add("nullout", jj, lambda x: (x.B, None, 4, 7, 63, None, HOST, None))
    add("misaligned-J", jj, lambda x: (MIS, None, 4, 7, 63, A, DEV, None))
    add("misaligned-H", jj, lambda x: (A, MIS, 4, 7, 63, A, DEV, None))
    add("n17+nullJ", jj, lambda x: (None, None, 4, 17, 63, x.B, HOST, None))
    add("empty", jj, lambda x: (x.B, x.B, 0, 7, 63, x.B, HOST, None))
    return rows


def _pose_rows():
    rows = []
    forms = {       # (Te, nTe, Tep, nTep, method, out, mem); p_servo: out is both v and arrived
        "angle_axis": lambda a, na, b, nb, meth, o, mem: (a, na, b, nb, o, mem, None),
        "p_servo_error": lambda a, na, b, nb, meth, o, mem: (a, na, b, nb, meth, o, mem, None),
        "p_servo": lambda a, na, b, nb, meth, o, mem: (a, na, b, nb, meth, ONE, 0.01, o, (o if o in (None, MIS) else o + 512), mem, None),
    }
    for name, f in forms.items():
        add = lambda tag, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
        add("mem7", lambda x, f=f: f(x.B, 3, x.B, 3, 0, x.B, 7))
        add("negcount", lambda x, f=f: f(x.B, -1, x.B, 3, 0, x.B, HOST))
        add("negcount2", lambda x, f=f: f(x.B, 3, x.B, -2, 0, x.B, HOST))
        add("counts-2-3", lambda x, f=f: f(x.B, 2, x.B, 3, 0, x.B, HOST))
        add("counts-3-2", lambda x, f=f: f(x.B, 3, x.B, 2, 0, x.B, HOST))
        add("nullTe", lambda x, f=f: f(None, 3, x.B, 3, 0, x.B, HOST))
        add("nullTep", lambda x, f=f: f(x.B, 3, None, 1, 0, x.B, HOST))
        add("nullout", lambda x, f=f: f(x.B, 1, x.B, 3, 0, None, HOST))
        add("misaligned-Te", lambda x, f=f: f(MIS, 3, A, 3, 0, A, DEV))
        add("misaligned-Tep", lambda x, f=f: f(A, 3, MIS, 3, 0, A, DEV))
        add("misaligned-out", lambda x, f=f: f(A, 3, A, 3, 0, MIS, DEV))
        add("mem7+negcount", lambda x, f=f: f(x.B, -1, x.B, 3, 0, x.B, 7))
        add("counts-2-3+nullout", lambda x, f=f: f(x.B, 2, x.B, 3, 0, None, HOST))
        add("negcount+nullTe", lambda x, f=f: f(None, -1, x.B, 3, 0, x.B, HOST))
        add("empty", lambda x, f=f: f(x.B, 0, x.B, 0, 0, x.B, HOST))
        add("empty-one-side", lambda x, f=f: f(None, 0, None, 5, 0, None, DEV))
        if name != "angle_axis":
            add("method2", lambda x, f=f: f(x.B, 3, x.B, 3, 2, x.B, HOST))
            add("method-1+mem7", lambda x, f=f: f(x.B, 3, x.B, 3, -1, x.B, 7))
    add = lambda tag, g: rows.append(("p_servo-" + tag, "rtbhip_p_servo", g))
    add("nullgain", lambda x: (x.B, 3, x.B, 3, 0, None, 0.01, x.B, x.B, HOST, None))
    add("nullgain+empty", lambda x: (x.B, 0, x.B, 0, 0, None, 0.01, x.B, x.B, HOST, None))
    add("nullgain+counts", lambda x: (x.B, 2, x.B, 3, 0, None, 0.01, x.B, x.B, HOST, None))
    add("negcount+nullgain", lambda x: (x.B, -1, x.B, 3, 0, None, 0.01, x.B, x.B, HOST, None))
    add("nullarrived", lambda x: (x.B, 3, x.B, 3, 0, x.one, 0.01, x.B, None, HOST, None))
    add("misaligned-arrived-is-fine-but-v-is-not", lambda x: (A, 3, A, 3, 0, x.one, 0.01, MIS, A + 1, DEV, None))
    return rows


ONE = object()      # stands for Ctx.one (the gain vector) in the shared pose rows


def _frames_partial_rows():
    rows = []
    add = lambda tag, name, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
    lf = "link_frames"                    # (chain, q, N, base16, marks, nmarks, out, mem, stream)
    add("unknown", lf, lambda x: (BAD, x.B, 4, None, x.marks, 2, x.B, HOST, None))
    add("mem7", lf, lambda x: (x.c, x.B, 4, None, x.marks, 2, x.B, 7, None))
    add("negN", lf, lambda x: (x.c, x.B, -1, None, x.marks, 2, x.B, HOST, None))
    add("nullmarks", lf, lambda x: (x.c, x.B, 4, None, None, 2, x.B, HOST, None))
    add("nullq", lf, lambda x: (x.c, None, 4, None, x.marks, 2, x.B, HOST, None))
    add("nullout", lf, lambda x: (x.c, x.B, 4, None, x.marks, 2, None, HOST, None))
    add("unknown+mem7", lf, lambda x: (BAD, x.B, 4, None, x.marks, 2, x.B, 7, None))
    add("mem7+negN", lf, lambda x: (x.c, x.B, -1, None, x.marks, 2, x.B, 7, None))
    add("negN+nullmarks", lf, lambda x: (x.c, x.B, -1, None, None, 2, x.B, HOST, None))
    add("empty", lf, lambda x: (x.c, x.B, 0, None, x.marks, 2, x.B, HOST, None))
    add("nomarks", lf, lambda x: (x.c, x.B, 4, None, None, 0, x.B, HOST, None))
    pf = "partial_fkine0"                 # (chain, q, N, tool16, order, out, mem, stream)
    add("unknown", pf, lambda x: (BAD, x.B, 4, None, 3, x.B, HOST, None))
    add("negN", pf, lambda x: (x.c, x.B, -1, None, 3, x.B, HOST, None))
    add("nullq", pf, lambda x: (x.c, None, 4, None, 3, x.B, HOST, None))
    add("mem7", pf, lambda x: (x.c, x.B, 4, None, 3, x.B, 7, None))
    add("order2", pf, lambda x: (x.c, x.B, 4, None, 2, x.B, HOST, None))
    add("order99", pf, lambda x: (x.c, x.B, 4, None, 99, x.B, HOST, None))
    add("nojoints", pf, lambda x: (x.c0, x.B, 4, None, 3, x.B, HOST, None))
    add("nullout", pf, lambda x: (x.c, x.B, 4, None, 3, None, HOST, None))
    add("mem7+order2", pf, lambda x: (x.c, x.B, 4, None, 2, x.B, 7, None))
    add("order2+nojoints", pf, lambda x: (x.c0, x.B, 4, None, 2, x.B, HOST, None))
    add("nojoints+nullout", pf, lambda x: (x.c0, x.B, 4, None, 3, None, HOST, None))
    add("empty", pf, lambda x: (x.c, x.B, 0, None, 3, x.B, HOST, None))
    add("empty4", pf, lambda x: (x.c, None, 0, None, 4, None, DEV, None))
    # n^order >= 2^24: refused by the entry point itself, before the output (far larger than x.B) is staged or touched
    add("16joints-order6", pf, lambda x: (x.c16, x.B, 1, None, 6, x.B, HOST, None))
    add("32joints-order5", pf, lambda x: (x.c32, x.B, 1, None, 5, x.B, HOST, None))
    add("32joints-order5+nullout", pf, lambda x: (x.c32, x.B, 1, None, 5, None, HOST, None))
    add("15joints-order6-empty", pf, lambda x: (x.c15, x.B, 0, None, 6, x.B, HOST, None))
    return rows


def _ik_rows():
    rows = []
    add = lambda tag, name, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))

    def lm(h, Tep, N, out, mem, ilimit=30, slimit=10, method=0, flavour=0, q0=None):
        return (h, Tep, N, q0, ilimit, slimit, 1e-6, 0, None, 1.0, method, flavour, 0, out, out, out, out, out, mem, None)

    def ns(h, Tep, N, out, mem, ilimit=30, slimit=10, method=0, flavour=1, kq=0.0, ps=0.1, pi=None):
        return (h, Tep, N, None, ilimit, slimit, 1e-6, 0, None, 1.0, method, flavour, 0, kq, 0.0, ps, pi, out, out, out, out, out, mem, None)

    def qp(h, Tep, N, out, mem, kj=1.0, ks=1.0, ilimit=30, kq=0.0):
        return (h, Tep, N, None, ilimit, 10, 1e-6, 0, None, 0, kj, ks, kq, 0.0, 0.1, None, out, out, out, out, out, mem, None)

    il = "ik_lm"
    add("unknown", il, lambda x: lm(BAD, x.B, 4, x.B, HOST))
    add("negN", il, lambda x: lm(x.c, x.B, -1, x.B, HOST))
    add("nullTep", il, lambda x: lm(x.c, None, 4, x.B, HOST))
    add("mem7", il, lambda x: lm(x.c, x.B, 4, x.B, 7))
    add("method-1", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, method=-1))
    add("method5", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, method=5))
    add("flavour2", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, flavour=2))
    add("ilimit0", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, ilimit=0))
    add("slimit0", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, slimit=0))
    add("nojoints", il, lambda x: lm(x.c0, x.B, 4, x.B, HOST))
    add("qwidth", il, lambda x: lm(x.cw, x.B, 4, x.B, HOST))
    add("nullout", il, lambda x: lm(x.c, x.B, 4, None, HOST))
    add("method5+unknown", il, lambda x: lm(BAD, x.B, 4, x.B, HOST, method=5))
    add("unknown+mem7", il, lambda x: lm(BAD, x.B, 4, x.B, 7))
    add("mem7+flavour2", il, lambda x: lm(x.c, x.B, 4, x.B, 7, flavour=2))
    add("flavour2+ilimit0", il, lambda x: lm(x.c, x.B, 4, x.B, HOST, flavour=2, ilimit=0))
    add("ilimit0+qwidth", il, lambda x: lm(x.cw, x.B, 4, x.B, HOST, ilimit=0))
    add("qwidth+nullout", il, lambda x: lm(x.cw, x.B, 4, None, HOST))
    add("empty", il, lambda x: lm(x.c, x.B, 0, x.B, HOST))
    add("empty-dev", il, lambda x: lm(x.c, None, 0, None, DEV))
    nn = "ik_lm_nullspace"
    add("unknown", nn, lambda x: ns(BAD, x.B, 4, x.B, HOST))
    add("method5", nn, lambda x: ns(x.c, x.B, 4, x.B, HOST, method=5))
    add("kq-flavour0", nn, lambda x: ns(x.c, x.B, 4, x.B, HOST, flavour=0, kq=0.5))
    add("ps-equals-pi", nn, lambda x: ns(x.c, x.B, 4, x.B, HOST, kq=0.5, ps=0.3))
    add("ps-equals-given-pi", nn, lambda x: ns(x.c, x.B, 4, x.B, HOST, kq=0.5, ps=1.0, pi=x.one))
    add("nullout+kq-flavour0", nn, lambda x: ns(x.c, x.B, 4, None, HOST, flavour=0, kq=0.5))
    add("ilimit0+kq-flavour0", nn, lambda x: ns(x.c, x.B, 4, x.B, HOST, ilimit=0, flavour=0, kq=0.5))
    add("empty", nn, lambda x: ns(x.c, x.B, 0, x.B, HOST))
    add("empty+kq-flavour0", nn, lambda x: ns(x.c, x.B, 0, x.B, HOST, flavour=0, kq=0.5))
    iq = "ik_qp"
    add("unknown", iq, lambda x: qp(BAD, x.B, 4, x.B, HOST))
    add("kj0", iq, lambda x: qp(x.c, x.B, 4, x.B, HOST, kj=0.0))
    add("kj-1", iq, lambda x: qp(x.c, x.B, 4, x.B, HOST, kj=-1.0))
    add("ks0", iq, lambda x: qp(x.c, x.B, 4, x.B, HOST, ks=0.0))
    add("kjnan", iq, lambda x: qp(x.c, x.B, 4, x.B, HOST, kj=float("nan")))
    add("kj0+unknown", iq, lambda x: qp(BAD, x.B, 4, x.B, HOST, kj=0.0))
    add("negN", iq, lambda x: qp(x.c, x.B, -1, x.B, HOST))
    add("mem7", iq, lambda x: qp(x.c, x.B, 4, x.B, 7))
    add("ilimit0", iq, lambda x: qp(x.c, x.B, 4, x.B, HOST, ilimit=0))
    add("qwidth", iq, lambda x: qp(x.cw, x.B, 4, x.B, HOST))
    add("nullout", iq, lambda x: qp(x.c, x.B, 4, None, HOST))
    add("empty", iq, lambda x: qp(x.c, x.B, 0, x.B, HOST))
    add("bad", "ik_restart", lambda x: (BAD, 1, 0, 0, x.B))
    add("nullout", "ik_restart", lambda x: (x.c, 1, 0, 0, None))
    add("negative", "ik_target_base", lambda x: (-1,))
    return rows


def _dyn_rows():
    rows = []
    add = lambda tag, name, g: rows.append((name + "-" + tag, "rtbhip_" + name, g))
    for nm in ("rne", "rne_f32", "rne_base_wrench"):
        m = DEV if nm == "rne_f32" else HOST

        def f(h, q, N, grav, tau, mem, nm=nm, wb=True):
            if nm == "rne_base_wrench":
                return (h, q, None, None, N, grav, None, tau, tau if wb else None, mem, None)
            return (h, q, None, None, N, grav, None, tau, mem, None)
        add("unknown", nm, lambda x, f=f, m=m: f(BAD, x.B, 4, x.B, x.B, m))
        add("negN", nm, lambda x, f=f, m=m: f(x.d, x.B, -1, x.B, x.B, m))
        add("nullq", nm, lambda x, f=f, m=m: f(x.d, None, 4, x.B, x.B, m))
        add("mem7", nm, lambda x, f=f: f(x.d, x.B, 4, x.B, x.B, 7))
        add("nullgrav", nm, lambda x, f=f, m=m: f(x.d, x.B, 4, None, x.B, m))
        add("nulltau", nm, lambda x, f=f, m=m: f(x.d, x.B, 4, x.B, None, m))
        add("unknown+negN", nm, lambda x, f=f, m=m: f(BAD, x.B, -1, x.B, x.B, m))
        add("mem7+nullgrav", nm, lambda x, f=f: f(x.d, x.B, 4, None, x.B, 7))
        add("nullgrav+nulltau", nm, lambda x, f=f, m=m: f(x.d, x.B, 4, None, None, m))
        add("empty+nullgrav", nm, lambda x, f=f, m=m: f(x.d, x.B, 0, None, x.B, m))
        add("empty", nm, lambda x, f=f, m=m: f(x.d, None, 0, x.B, None, m))
        add("treehandle", nm, lambda x, f=f, m=m: f(x.t, x.B, 4, x.B, x.B, m))
        if nm == "rne_f32":
            add("hostmem", nm, lambda x, f=f: f(x.d, x.B, 4, x.B, x.B, HOST))
            add("hostmem+nullgrav", nm, lambda x, f=f: f(x.d, x.B, 4, None, x.B, HOST))
            add("hostmem-empty", nm, lambda x, f=f: f(x.d, x.B, 0, x.B, x.B, HOST))
        if nm == "rne_base_wrench":
            add("nullwbase", nm, lambda x, f=f: f(x.d, x.B, 4, x.B, x.B, HOST, wb=False))
    for kind, hname in (("", "d"), ("tree_", "t")):
        other = "t" if hname == "d" else "d"
        forms = {   # (handle, q, qd, tq, N, grav, out, mem)
            kind + "inertia": lambda h, q, qd, tq, N, g, o, mem: (h, q, N, o, mem, None),
            kind + "coriolis": lambda h, q, qd, tq, N, g, o, mem: (h, q, qd, N, o, mem, None),
            kind + "accel": lambda h, q, qd, tq, N, g, o, mem: (h, q, qd, tq, N, g, o, mem, None),
        }
        for nm, f in forms.items():
            H = lambda x, hname=hname: getattr(x, hname)
            add("unknown", nm, lambda x, f=f: f(BAD, x.B, x.B, x.B, 4, x.B, x.B, HOST))
            add("otherkind", nm, lambda x, f=f, other=other: f(getattr(x, other), x.B, x.B, x.B, 4, x.B, x.B, HOST))
            add("negN", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, -1, x.B, x.B, HOST))
            add("nullq", nm, lambda x, f=f, H=H: f(H(x), None, x.B, x.B, 4, x.B, x.B, HOST))
            add("mem7", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, 4, x.B, x.B, 7))
            add("nullout", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, 4, x.B, None, HOST))
            add("unknown+mem7", nm, lambda x, f=f: f(BAD, x.B, x.B, x.B, 4, x.B, x.B, 7))
            add("mem7+nullout", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, 4, x.B, None, 7))
            if not nm.endswith("inertia"):
                add("nullqd", nm, lambda x, f=f, H=H: f(H(x), x.B, None, x.B, 4, x.B, x.B, HOST))
                add("nullout+nullqd", nm, lambda x, f=f, H=H: f(H(x), x.B, None, x.B, 4, x.B, None, HOST))
            if nm.endswith("accel"):
                add("nulltorque", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, None, 4, x.B, x.B, HOST))
                add("nullgrav", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, 4, None, x.B, HOST))
                add("nullqd+nulltorque", nm, lambda x, f=f, H=H: f(H(x), x.B, None, None, 4, x.B, x.B, HOST))
            add("empty", nm, lambda x, f=f, H=H: f(H(x), x.B, x.B, x.B, 0, x.B, x.B, HOST))
            add("empty-dev", nm, lambda x, f=f, H=H: f(H(x), None, None, None, 0, None, None, DEV))
    tr = "tree_rne"                       # (tree, q, qd, qdd, N, gravity3, tau, mem, stream)
    add("unknown", tr, lambda x: (BAD, x.B, None, None, 4, x.B, x.B, HOST, None))
    add("dynhandle", tr, lambda x: (x.d, x.B, None, None, 4, x.B, x.B, HOST, None))
    add("negN", tr, lambda x: (x.t, x.B, None, None, -1, x.B, x.B, HOST, None))
    add("nullq", tr, lambda x: (x.t, None, None, None, 4, x.B, x.B, HOST, None))
    add("mem7", tr, lambda x: (x.t, x.B, None, None, 4, x.B, x.B, 7, None))
    add("nullgrav", tr, lambda x: (x.t, x.B, None, None, 4, None, x.B, HOST, None))
    add("nulltau", tr, lambda x: (x.t, x.B, None, None, 4, x.B, None, HOST, None))
    add("unknown+negN", tr, lambda x: (BAD, x.B, None, None, -1, x.B, x.B, HOST, None))
    add("mem7+nullgrav", tr, lambda x: (x.t, x.B, None, None, 4, None, x.B, 7, None))
    add("nullgrav+nulltau", tr, lambda x: (x.t, x.B, None, None, 4, None, None, HOST, None))
    add("empty+nullgrav", tr, lambda x: (x.t, x.B, None, None, 0, None, x.B, HOST, None))
    add("empty", tr, lambda x: (x.t, None, None, None, 0, x.B, None, DEV, None))
    return rows


def _fleet_rows():
    rows = []
    for nm in ("fleet_fkine_jacob", "fleet_fkine_jacob_packed"):
        packed = nm.endswith("packed")

        def f(h, nch, q, N, frame, T, J, mem, packed=packed):
            return (h, nch, q, N, frame, T, mem, None) if packed else (h, nch, q, N, frame, T, J, mem, None)
        add = lambda tag, g: rows.append((nm + "-" + tag, "rtbhip_" + nm, g))
        add("negchains", lambda x, f=f: f(x.h2, -1, x.p2, x.n2, 0, x.p2, x.p2, HOST))
        add("nullchains", lambda x, f=f: f(None, 2, x.p2, x.n2, 0, x.p2, x.p2, HOST))
        add("nullq", lambda x, f=f: f(x.h2, 2, None, x.n2, 0, x.p2, x.p2, HOST))
        add("nullN", lambda x, f=f: f(x.h2, 2, x.p2, None, 0, x.p2, x.p2, HOST))
        add("nullT", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 0, None, x.p2, HOST))
        if not packed:
            add("nullJ", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 0, x.p2, None, HOST))
        add("frame3", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 3, x.p2, x.p2, HOST))
        add("mem7", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 0, x.p2, x.p2, 7))
        add("unknown", lambda x, f=f: f(x.hbad, 2, x.p2, x.n0, 0, x.p2, x.p2, HOST))
        add("negN", lambda x, f=f: f(x.h2, 2, x.p2, x.nneg0, 0, x.p2, x.p2, HOST))
        add("nullbuffer-q", lambda x, f=f: f(x.h2, 2, x.pnull0, x.n20, 0, x.p2, x.p2, HOST))
        add("nullbuffer-T", lambda x, f=f: f(x.h2, 2, x.p2, x.n20, 0, x.pnull0, x.p2, HOST))
        if not packed:
            add("nullbuffer-J", lambda x, f=f: f(x.h2, 2, x.p2, x.n20, 0, x.p2, x.pnull0, HOST))
        add("nullT+frame3", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 3, None, x.p2, HOST))
        add("frame3+mem7", lambda x, f=f: f(x.h2, 2, x.p2, x.n2, 3, x.p2, x.p2, 7))
        add("mem7+unknown", lambda x, f=f: f(x.hbad, 2, x.p2, x.n0, 0, x.p2, x.p2, 7))
        add("unknown-first+negN", lambda x, f=f: f(x.hbad0, 2, x.p2, x.nneg, 0, x.p2, x.p2, HOST))
        add("negN-first+unknown", lambda x, f=f: f(x.hbad, 2, x.p2, x.nneg0, 0, x.p2, x.p2, HOST))
        add("nochains", lambda x, f=f: f(None, 0, None, None, 0, None, None, HOST))
        add("empty", lambda x, f=f: f(x.h2, 2, x.p2, x.n0, 0, x.p2, x.p2, HOST))
        add("empty-dev-null", lambda x, f=f: f(x.h2, 2, x.pnull0, x.n0, 0, x.pnull0, x.pnull0, DEV))
    rows.append(("stream_probe-negread", "rtbhip_stream_probe", lambda x: (x.B, -1, x.B, 1, None)))
    rows.append(("stream_probe-nullsrc", "rtbhip_stream_probe", lambda x: (None, 4, x.B, 1, None)))
    rows.append(("stream_probe-nulldst", "rtbhip_stream_probe", lambda x: (x.B, 4, None, 1, None)))
    return rows


ROWS = _kin_rows() + _diff_rows() + _from_jacobian_rows() + _pose_rows() + _frames_partial_rows() + _ik_rows() + _dyn_rows() + _fleet_rows()

EXPECTED = {
    'fkine-unknown': (EINVAL, 'fkine: unknown chain handle'),
    'fkine-negN': (EINVAL, 'fkine: negative N'),
    'fkine-nullq': (EINVAL, 'fkine: NULL input with N > 0'),
    'fkine-mem7': (EINVAL, 'fkine: bad mem kind'),
    'fkine-nullout': (EINVAL, 'fkine: NULL T'),
    'fkine-unknown+negN': (EINVAL, 'fkine: unknown chain handle'),
    'fkine-mem7+nullq': (EINVAL, 'fkine: NULL input with N > 0'),
    'fkine-empty': (OK, None),
    'fkine-empty-null': (OK, None),
    'jacob-unknown': (EINVAL, 'jacob: unknown chain handle'),
    'jacob-negN': (EINVAL, 'jacob: negative N'),
    'jacob-nullq': (EINVAL, 'jacob: NULL input with N > 0'),
    'jacob-mem7': (EINVAL, 'jacob: bad mem kind'),
    'jacob-nullout': (EINVAL, 'jacob: NULL J'),
    'jacob-frame3': (EINVAL, 'jacob: frame must be 0 (jacob0) or 1 (jacobe)'),
    'jacob-frame3+nullout': (EINVAL, 'jacob: NULL J'),
    'jacob-unknown+negN': (EINVAL, 'jacob: unknown chain handle'),
    'jacob-mem7+nullq': (EINVAL, 'jacob: NULL input with N > 0'),
    'jacob-empty': (OK, None),
    'jacob-empty-null': (OK, None),
    'fkine_jacob-unknown': (EINVAL, 'fkine_jacob: unknown chain handle'),
    'fkine_jacob-negN': (EINVAL, 'fkine_jacob: negative N'),
    'fkine_jacob-nullq': (EINVAL, 'fkine_jacob: NULL input with N > 0'),
    'fkine_jacob-mem7': (EINVAL, 'fkine_jacob: bad mem kind'),
    'fkine_jacob-nullout': (EINVAL, 'fkine_jacob: NULL T or J'),
    'fkine_jacob-frame3': (EINVAL, 'fkine_jacob: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob-frame3+nullout': (EINVAL, 'fkine_jacob: NULL T or J'),
    'fkine_jacob-unknown+negN': (EINVAL, 'fkine_jacob: unknown chain handle'),
    'fkine_jacob-mem7+nullq': (EINVAL, 'fkine_jacob: NULL input with N > 0'),
    'fkine_jacob-empty': (OK, None),
    'fkine_jacob-empty-null': (OK, None),
    'fkine_jacob_packed-unknown': (EINVAL, 'fkine_jacob_packed: unknown chain handle'),
    'fkine_jacob_packed-negN': (EINVAL, 'fkine_jacob_packed: negative N'),
    'fkine_jacob_packed-nullq': (EINVAL, 'fkine_jacob_packed: NULL input with N > 0'),
    'fkine_jacob_packed-mem7': (EINVAL, 'fkine_jacob_packed: bad mem kind'),
    'fkine_jacob_packed-nullout': (EINVAL, 'fkine_jacob_packed: no output buffer'),
    'fkine_jacob_packed-frame3': (EINVAL, 'fkine_jacob_packed: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob_packed-frame3+nullout': (EINVAL, 'fkine_jacob_packed: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob_packed-unknown+negN': (EINVAL, 'fkine_jacob_packed: unknown chain handle'),
    'fkine_jacob_packed-mem7+nullq': (EINVAL, 'fkine_jacob_packed: NULL input with N > 0'),
    'fkine_jacob_packed-empty': (OK, None),
    'fkine_jacob_packed-empty-null': (OK, None),
    'fkine_jacob_f32-unknown': (EINVAL, 'fkine_jacob_f32: unknown chain handle'),
    'fkine_jacob_f32-negN': (EINVAL, 'fkine_jacob_f32: negative N'),
    'fkine_jacob_f32-nullq': (EINVAL, 'fkine_jacob_f32: NULL input with N > 0'),
    'fkine_jacob_f32-mem7': (EINVAL, 'fkine_jacob_f32: bad mem kind'),
    'fkine_jacob_f32-nullout': (EINVAL, 'fkine_jacob_f32: no output buffer'),
    'fkine_jacob_f32-frame3': (EINVAL, 'fkine_jacob_f32: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob_f32-frame3+nullout': (EINVAL, 'fkine_jacob_f32: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob_f32-unknown+negN': (EINVAL, 'fkine_jacob_f32: unknown chain handle'),
    'fkine_jacob_f32-mem7+nullq': (EINVAL, 'fkine_jacob_f32: NULL input with N > 0'),
    'fkine_jacob_f32-hostmem': (EINVAL, 'fkine_jacob_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_f32-hostmem+frame3': (EINVAL, 'fkine_jacob_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_f32-hostmem-empty': (EINVAL, 'fkine_jacob_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_f32-empty': (OK, None),
    'fkine_jacob_f32-empty-null': (OK, None),
    'fkine_jacob_packed_f32-unknown': (EINVAL, 'fkine_jacob_packed_f32: unknown chain handle'),
    'fkine_jacob_packed_f32-negN': (EINVAL, 'fkine_jacob_packed_f32: negative N'),
    'fkine_jacob_packed_f32-nullq': (EINVAL, 'fkine_jacob_packed_f32: NULL input with N > 0'),
    'fkine_jacob_packed_f32-mem7': (EINVAL, 'fkine_jacob_packed_f32: bad mem kind'),
    'fkine_jacob_packed_f32-nullout': (EINVAL, 'fkine_jacob_packed_f32: no output buffer'),
    'fkine_jacob_packed_f32-frame3': (EINVAL, 'fkine_jacob_packed_f32: frame must be 0 (jacob0) or 1 (jacobe)'),
    'fkine_jacob_packed_f32-frame3+nullout': (EINVAL, 'fkine_jacob_packed_f32: no output buffer'),
    'fkine_jacob_packed_f32-unknown+negN': (EINVAL, 'fkine_jacob_packed_f32: unknown chain handle'),
    'fkine_jacob_packed_f32-mem7+nullq': (EINVAL, 'fkine_jacob_packed_f32: NULL input with N > 0'),
    'fkine_jacob_packed_f32-hostmem': (EINVAL, 'fkine_jacob_packed_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_packed_f32-hostmem+frame3': (EINVAL, 'fkine_jacob_packed_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_packed_f32-hostmem-empty': (EINVAL, 'fkine_jacob_packed_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'fkine_jacob_packed_f32-empty': (OK, None),
    'fkine_jacob_packed_f32-empty-null': (OK, None),
    'hessian-unknown': (EINVAL, 'hessian: unknown chain handle'),
    'hessian-negN': (EINVAL, 'hessian: negative N'),
    'hessian-nullq': (EINVAL, 'hessian: NULL input with N > 0'),
    'hessian-mem7': (EINVAL, 'hessian: bad mem kind'),
    'hessian-nullout': (EINVAL, 'hessian: NULL H'),
    'hessian-frame3': (EINVAL, 'hessian: frame must be 0 (jacob0) or 1 (jacobe)'),
    'hessian-frame3+nullout': (EINVAL, 'hessian: NULL H'),
    'hessian-unknown+negN': (EINVAL, 'hessian: unknown chain handle'),
    'hessian-mem7+nullq': (EINVAL, 'hessian: NULL input with N > 0'),
    'hessian-empty': (OK, None),
    'hessian-empty-null': (OK, None),
    'jacob_dot-unknown': (EINVAL, 'jacob_dot: unknown chain handle'),
    'jacob_dot-negN': (EINVAL, 'jacob_dot: negative N'),
    'jacob_dot-nullq': (EINVAL, 'jacob_dot: NULL input with N > 0'),
    'jacob_dot-mem7': (EINVAL, 'jacob_dot: bad mem kind'),
    'jacob_dot-nullout': (EINVAL, 'jacob_dot: NULL qd/output'),
    'jacob_dot-unknown+mem7': (EINVAL, 'jacob_dot: unknown chain handle'),
    'jacob_dot-negN+nullout': (EINVAL, 'jacob_dot: negative N'),
    'jacob_dot-empty': (OK, None),
    'jacob_dot-empty-dev': (OK, None),
    'jacob0_analytical-unknown': (EINVAL, 'jacob0_analytical: unknown chain handle'),
    'jacob0_analytical-negN': (EINVAL, 'jacob0_analytical: negative N'),
    'jacob0_analytical-nullq': (EINVAL, 'jacob0_analytical: NULL input with N > 0'),
    'jacob0_analytical-mem7': (EINVAL, 'jacob0_analytical: bad mem kind'),
    'jacob0_analytical-nullout': (EINVAL, 'jacob0_analytical: NULL qd/output'),
    'jacob0_analytical-unknown+mem7': (EINVAL, 'jacob0_analytical: unknown chain handle'),
    'jacob0_analytical-negN+nullout': (EINVAL, 'jacob0_analytical: negative N'),
    'jacob0_analytical-empty': (OK, None),
    'jacob0_analytical-empty-dev': (OK, None),
    'jacob0_dot_analytical-unknown': (EINVAL, 'jacob0_dot_analytical: unknown chain handle'),
    'jacob0_dot_analytical-negN': (EINVAL, 'jacob0_dot_analytical: negative N'),
    'jacob0_dot_analytical-nullq': (EINVAL, 'jacob0_dot_analytical: NULL input with N > 0'),
    'jacob0_dot_analytical-mem7': (EINVAL, 'jacob0_dot_analytical: bad mem kind'),
    'jacob0_dot_analytical-nullout': (EINVAL, 'jacob0_dot_analytical: NULL qd/output'),
    'jacob0_dot_analytical-unknown+mem7': (EINVAL, 'jacob0_dot_analytical: unknown chain handle'),
    'jacob0_dot_analytical-negN+nullout': (EINVAL, 'jacob0_dot_analytical: negative N'),
    'jacob0_dot_analytical-empty': (OK, None),
    'jacob0_dot_analytical-empty-dev': (OK, None),
    'manipulability-unknown': (EINVAL, 'manipulability: unknown chain handle'),
    'manipulability-negN': (EINVAL, 'manipulability: negative N'),
    'manipulability-nullq': (EINVAL, 'manipulability: NULL input with N > 0'),
    'manipulability-mem7': (EINVAL, 'manipulability: bad mem kind'),
    'manipulability-nullout': (EINVAL, 'manipulability: NULL qd/output'),
    'manipulability-unknown+mem7': (EINVAL, 'manipulability: unknown chain handle'),
    'manipulability-negN+nullout': (EINVAL, 'manipulability: negative N'),
    'manipulability-empty': (OK, None),
    'manipulability-empty-dev': (OK, None),
    'jacobm-unknown': (EINVAL, 'jacobm: unknown chain handle'),
    'jacobm-negN': (EINVAL, 'jacobm: negative N'),
    'jacobm-nullq': (EINVAL, 'jacobm: NULL input with N > 0'),
    'jacobm-mem7': (EINVAL, 'jacobm: bad mem kind'),
    'jacobm-nullout': (EINVAL, 'jacobm: NULL qd/output'),
    'jacobm-unknown+mem7': (EINVAL, 'jacobm: unknown chain handle'),
    'jacobm-negN+nullout': (EINVAL, 'jacobm: negative N'),
    'jacobm-empty': (OK, None),
    'jacobm-empty-dev': (OK, None),
    'jacob_dot-frame3': (EINVAL, 'jacob_dot: frame must be 0 or 1'),
    'jacob_dot-nullqd': (EINVAL, 'jacob_dot: NULL qd/output'),
    'jacob_dot-frame3+nullqd': (EINVAL, 'jacob_dot: frame must be 0 or 1'),
    'jacob0_dot_analytical-nullqd': (EINVAL, 'jacob0_dot_analytical: NULL qd/output'),
    'jacob0_analytical-rep-1': (EINVAL, 'jacob0_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'jacob0_analytical-rep-1+unknown': (EINVAL, 'jacob0_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'jacob0_analytical-rep4': (EINVAL, 'jacob0_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'jacob0_analytical-rep4+unknown': (EINVAL, 'jacob0_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'jacob0_dot_analytical-rep-1': (EINVAL, 'jacob0_dot_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'jacob0_dot_analytical-rep4': (EINVAL, 'jacob0_dot_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp'),
    'manipulability-method-1': (EINVAL, 'manipulability: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability-method3': (EINVAL, 'manipulability: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability-method3+unknown': (EINVAL, 'manipulability: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability-noaxes': (EINVAL, 'manipulability: empty axes mask'),
    'manipulability-noaxes64': (EINVAL, 'manipulability: empty axes mask'),
    'jacobm-noaxes': (EINVAL, 'jacobm: empty axes mask'),
    'jacobm-noaxes+nullout': (EINVAL, 'jacobm: empty axes mask'),
    'hessian_from_jacobian-negN': (EINVAL, 'hessian_from_jacobian: negative N'),
    'hessian_from_jacobian-nullJ': (EINVAL, 'hessian_from_jacobian: NULL input with N > 0'),
    'hessian_from_jacobian-mem7': (EINVAL, 'hessian_from_jacobian: bad mem kind'),
    'hessian_from_jacobian-n0': (ELIMIT, 'hessian_from_jacobian: n must be 1..RTBHIP_MAX_JOINTS'),
    'hessian_from_jacobian-n33': (ELIMIT, 'hessian_from_jacobian: n must be 1..RTBHIP_MAX_JOINTS'),
    'hessian_from_jacobian-nullH': (EINVAL, 'hessian_from_jacobian: NULL H'),
    'hessian_from_jacobian-misaligned-J': (EINVAL, 'hessian_from_jacobian: device buffers must be 16-byte aligned'),
    'hessian_from_jacobian-misaligned-H': (EINVAL, 'hessian_from_jacobian: device buffers must be 16-byte aligned'),
    'hessian_from_jacobian-negN+n0': (EINVAL, 'hessian_from_jacobian: negative N'),
    'hessian_from_jacobian-n0+nullH': (ELIMIT, 'hessian_from_jacobian: n must be 1..RTBHIP_MAX_JOINTS'),
    'hessian_from_jacobian-empty': (OK, None),
    'hessian_from_jacobian-empty-dev': (OK, None),
    'manipulability_from_jacobian-negN': (EINVAL, 'manipulability_from_jacobian: negative N'),
    'manipulability_from_jacobian-nullJ': (EINVAL, 'manipulability_from_jacobian: NULL input with N > 0'),
    'manipulability_from_jacobian-mem7': (EINVAL, 'manipulability_from_jacobian: bad mem kind'),
    'manipulability_from_jacobian-n0': (ELIMIT, 'manipulability_from_jacobian: n must be 1..16'),
    'manipulability_from_jacobian-n17': (ELIMIT, 'manipulability_from_jacobian: n must be 1..16'),
    'manipulability_from_jacobian-noaxes': (EINVAL, 'manipulability_from_jacobian: empty axes mask'),
    'manipulability_from_jacobian-method-1': (EINVAL, 'manipulability_from_jacobian: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability_from_jacobian-method3': (EINVAL, 'manipulability_from_jacobian: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability_from_jacobian-nullout': (EINVAL, 'manipulability_from_jacobian: NULL output'),
    'manipulability_from_jacobian-misaligned': (EINVAL, 'manipulability_from_jacobian: device buffers must be 16-byte aligned'),
    'manipulability_from_jacobian-method3+n0': (EINVAL, 'manipulability_from_jacobian: method must be 0 yoshikawa, 1 minsingular, 2 invcondition'),
    'manipulability_from_jacobian-n0+noaxes': (ELIMIT, 'manipulability_from_jacobian: n must be 1..16'),
    'manipulability_from_jacobian-noaxes+negN': (EINVAL, 'manipulability_from_jacobian: empty axes mask'),
    'manipulability_from_jacobian-nullout+mem7': (EINVAL, 'manipulability_from_jacobian: NULL output'),
    'manipulability_from_jacobian-empty': (OK, None),
    'jacobm_from_jacobian-negN': (EINVAL, 'jacobm_from_jacobian: negative N'),
    'jacobm_from_jacobian-nullJ': (EINVAL, 'jacobm_from_jacobian: NULL input with N > 0'),
    'jacobm_from_jacobian-mem7': (EINVAL, 'jacobm_from_jacobian: bad mem kind'),
    'jacobm_from_jacobian-n17': (ELIMIT, 'jacobm_from_jacobian: n must be 1..16'),
    'jacobm_from_jacobian-noaxes': (EINVAL, 'jacobm_from_jacobian: empty axes mask'),
    'jacobm_from_jacobian-nullout': (EINVAL, 'jacobm_from_jacobian: NULL output'),
    'jacobm_from_jacobian-misaligned-J': (EINVAL, 'jacobm_from_jacobian: device buffers must be 16-byte aligned'),
    'jacobm_from_jacobian-misaligned-H': (EINVAL, 'jacobm_from_jacobian: device buffers must be 16-byte aligned'),
    'jacobm_from_jacobian-n17+nullJ': (ELIMIT, 'jacobm_from_jacobian: n must be 1..16'),
    'jacobm_from_jacobian-empty': (OK, None),
    'angle_axis-mem7': (EINVAL, 'angle_axis: bad mem kind'),
    'angle_axis-negcount': (EINVAL, 'angle_axis: negative count'),
    'angle_axis-negcount2': (EINVAL, 'angle_axis: negative count'),
    'angle_axis-counts-2-3': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'angle_axis-counts-3-2': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'angle_axis-nullTe': (EINVAL, 'angle_axis: NULL buffer'),
    'angle_axis-nullTep': (EINVAL, 'angle_axis: NULL buffer'),
    'angle_axis-nullout': (EINVAL, 'angle_axis: NULL buffer'),
    'angle_axis-misaligned-Te': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'angle_axis-misaligned-Tep': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'angle_axis-misaligned-out': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'angle_axis-mem7+negcount': (EINVAL, 'angle_axis: bad mem kind'),
    'angle_axis-counts-2-3+nullout': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'angle_axis-negcount+nullTe': (EINVAL, 'angle_axis: negative count'),
    'angle_axis-empty': (OK, None),
    'angle_axis-empty-one-side': (OK, None),
    'p_servo_error-mem7': (EINVAL, 'angle_axis: bad mem kind'),
    'p_servo_error-negcount': (EINVAL, 'angle_axis: negative count'),
    'p_servo_error-negcount2': (EINVAL, 'angle_axis: negative count'),
    'p_servo_error-counts-2-3': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'p_servo_error-counts-3-2': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'p_servo_error-nullTe': (EINVAL, 'angle_axis: NULL buffer'),
    'p_servo_error-nullTep': (EINVAL, 'angle_axis: NULL buffer'),
    'p_servo_error-nullout': (EINVAL, 'angle_axis: NULL buffer'),
    'p_servo_error-misaligned-Te': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'p_servo_error-misaligned-Tep': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'p_servo_error-misaligned-out': (EINVAL, 'angle_axis: device buffers must be 16-byte aligned'),
    'p_servo_error-mem7+negcount': (EINVAL, 'angle_axis: bad mem kind'),
    'p_servo_error-counts-2-3+nullout': (EINVAL, 'angle_axis: the pose counts must be equal, or one of them 1'),
    'p_servo_error-negcount+nullTe': (EINVAL, 'angle_axis: negative count'),
    'p_servo_error-empty': (OK, None),
    'p_servo_error-empty-one-side': (OK, None),
    'p_servo_error-method2': (EINVAL, 'p_servo_error: method must be 0 angle-axis or 1 rpy'),
    'p_servo_error-method-1+mem7': (EINVAL, 'p_servo_error: method must be 0 angle-axis or 1 rpy'),
    'p_servo-mem7': (EINVAL, 'p_servo: bad mem kind'),
    'p_servo-negcount': (EINVAL, 'p_servo: negative count'),
    'p_servo-negcount2': (EINVAL, 'p_servo: negative count'),
    'p_servo-counts-2-3': (EINVAL, 'p_servo: the pose counts must be equal, or one of them 1'),
    'p_servo-counts-3-2': (EINVAL, 'p_servo: the pose counts must be equal, or one of them 1'),
    'p_servo-nullTe': (EINVAL, 'p_servo: NULL buffer'),
    'p_servo-nullTep': (EINVAL, 'p_servo: NULL buffer'),
    'p_servo-nullout': (EINVAL, 'p_servo: NULL buffer'),
    'p_servo-misaligned-Te': (EINVAL, 'p_servo: device buffers must be 16-byte aligned'),
    'p_servo-misaligned-Tep': (EINVAL, 'p_servo: device buffers must be 16-byte aligned'),
    'p_servo-misaligned-out': (EINVAL, 'p_servo: device buffers must be 16-byte aligned'),
    'p_servo-mem7+negcount': (EINVAL, 'p_servo: bad mem kind'),
    'p_servo-counts-2-3+nullout': (EINVAL, 'p_servo: the pose counts must be equal, or one of them 1'),
    'p_servo-negcount+nullTe': (EINVAL, 'p_servo: negative count'),
    'p_servo-empty': (OK, None),
    'p_servo-empty-one-side': (OK, None),
    'p_servo-method2': (EINVAL, 'p_servo: method must be 0 angle-axis or 1 rpy'),
    'p_servo-method-1+mem7': (EINVAL, 'p_servo: method must be 0 angle-axis or 1 rpy'),
    'p_servo-nullgain': (EINVAL, 'p_servo: NULL gain'),
    'p_servo-nullgain+empty': (EINVAL, 'p_servo: NULL gain'),
    'p_servo-nullgain+counts': (EINVAL, 'p_servo: NULL gain'),
    'p_servo-negcount+nullgain': (EINVAL, 'p_servo: negative count'),
    'p_servo-nullarrived': (EINVAL, 'p_servo: NULL buffer'),
    'p_servo-misaligned-arrived-is-fine-but-v-is-not': (EINVAL, 'p_servo: device buffers must be 16-byte aligned'),
    'link_frames-unknown': (EINVAL, 'link_frames: unknown chain handle'),
    'link_frames-mem7': (EINVAL, 'link_frames: bad mem kind'),
    'link_frames-negN': (EINVAL, 'link_frames: negative N'),
    'link_frames-nullmarks': (EINVAL, 'link_frames: NULL marks'),
    'link_frames-nullq': (EINVAL, 'link_frames: NULL q / output'),
    'link_frames-nullout': (EINVAL, 'link_frames: NULL q / output'),
    'link_frames-unknown+mem7': (EINVAL, 'link_frames: unknown chain handle'),
    'link_frames-mem7+negN': (EINVAL, 'link_frames: bad mem kind'),
    'link_frames-negN+nullmarks': (EINVAL, 'link_frames: negative N'),
    'link_frames-empty': (OK, None),
    'link_frames-nomarks': (OK, None),
    'partial_fkine0-unknown': (EINVAL, 'partial_fkine0: unknown chain handle'),
    'partial_fkine0-negN': (EINVAL, 'partial_fkine0: negative N'),
    'partial_fkine0-nullq': (EINVAL, 'partial_fkine0: NULL input with N > 0'),
    'partial_fkine0-mem7': (EINVAL, 'partial_fkine0: bad mem kind'),
    'partial_fkine0-order2': (EINVAL, 'partial_fkine0: order must be 3..6'),
    'partial_fkine0-order99': (EINVAL, 'partial_fkine0: order must be 3..6'),
    'partial_fkine0-nojoints': (EINVAL, 'partial_fkine0: chain has no joints'),
    'partial_fkine0-nullout': (EINVAL, 'partial_fkine0: NULL output'),
    'partial_fkine0-mem7+order2': (EINVAL, 'partial_fkine0: bad mem kind'),
    'partial_fkine0-order2+nojoints': (EINVAL, 'partial_fkine0: order must be 3..6'),
    'partial_fkine0-nojoints+nullout': (EINVAL, 'partial_fkine0: chain has no joints'),
    'partial_fkine0-empty': (OK, None),
    'partial_fkine0-empty4': (OK, None),
    'partial_fkine0-16joints-order6': (ELIMIT, 'partial_fkine0: tensor too large (n^order must stay below 2^24)'),
    'partial_fkine0-32joints-order5': (ELIMIT, 'partial_fkine0: tensor too large (n^order must stay below 2^24)'),
    'partial_fkine0-32joints-order5+nullout': (EINVAL, 'partial_fkine0: NULL output'),
    'partial_fkine0-15joints-order6-empty': (OK, None),
    'ik_lm-unknown': (EINVAL, 'ik_lm: unknown chain handle'),
    'ik_lm-negN': (EINVAL, 'ik_lm: negative N'),
    'ik_lm-nullTep': (EINVAL, 'ik_lm: NULL input with N > 0'),
    'ik_lm-mem7': (EINVAL, 'ik_lm: bad mem kind'),
    'ik_lm-method-1': (EINVAL, 'ik_lm: method must be 0 chan, 1 wampler, 2 sugihara, 3 gauss-newton, 4 newton-raphson'),
    'ik_lm-method5': (EINVAL, 'ik_lm: method must be 0 chan, 1 wampler, 2 sugihara, 3 gauss-newton, 4 newton-raphson'),
    'ik_lm-flavour2': (EINVAL, 'ik_lm: flavour must be 0 (ik_LM) or 1 (ikine_LM)'),
    'ik_lm-ilimit0': (EINVAL, 'ik_lm: ilimit and slimit must be >= 1'),
    'ik_lm-slimit0': (EINVAL, 'ik_lm: ilimit and slimit must be >= 1'),
    'ik_lm-nojoints': (EINVAL, 'ik_lm: chain has no joints'),
    'ik_lm-qwidth': (EINVAL, 'ik_lm: chain must use jindex 0..n-1 (reference ik.cpp:34-37 assumes the same)'),
    'ik_lm-nullout': (EINVAL, 'ik_lm: NULL output'),
    'ik_lm-method5+unknown': (EINVAL, 'ik_lm: method must be 0 chan, 1 wampler, 2 sugihara, 3 gauss-newton, 4 newton-raphson'),
    'ik_lm-unknown+mem7': (EINVAL, 'ik_lm: unknown chain handle'),
    'ik_lm-mem7+flavour2': (EINVAL, 'ik_lm: bad mem kind'),
    'ik_lm-flavour2+ilimit0': (EINVAL, 'ik_lm: flavour must be 0 (ik_LM) or 1 (ikine_LM)'),
    'ik_lm-ilimit0+qwidth': (EINVAL, 'ik_lm: ilimit and slimit must be >= 1'),
    'ik_lm-qwidth+nullout': (EINVAL, 'ik_lm: chain must use jindex 0..n-1 (reference ik.cpp:34-37 assumes the same)'),
    'ik_lm-empty': (OK, None),
    'ik_lm-empty-dev': (OK, None),
    'ik_lm_nullspace-unknown': (EINVAL, 'ik_lm: unknown chain handle'),
    'ik_lm_nullspace-method5': (EINVAL, 'ik_lm: method must be 0 chan, 1 wampler, 2 sugihara, 3 gauss-newton, 4 newton-raphson'),
    'ik_lm_nullspace-kq-flavour0': (EINVAL, 'ik_lm: null-space terms belong to the Python solvers (flavour 1)'),
    'ik_lm_nullspace-ps-equals-pi': (EINVAL, 'ik_lm: ps must differ from pi'),
    'ik_lm_nullspace-ps-equals-given-pi': (EINVAL, 'ik_lm: ps must differ from pi'),
    'ik_lm_nullspace-nullout+kq-flavour0': (EINVAL, 'ik_lm: NULL output'),
    'ik_lm_nullspace-ilimit0+kq-flavour0': (EINVAL, 'ik_lm: ilimit and slimit must be >= 1'),
    'ik_lm_nullspace-empty': (OK, None),
    'ik_lm_nullspace-empty+kq-flavour0': (OK, None),
    'ik_qp-unknown': (EINVAL, 'ik_lm: unknown chain handle'),
    'ik_qp-kj0': (EINVAL, 'ik_qp: kj and ks must be positive (Q must be positive definite)'),
    'ik_qp-kj-1': (EINVAL, 'ik_qp: kj and ks must be positive (Q must be positive definite)'),
    'ik_qp-ks0': (EINVAL, 'ik_qp: kj and ks must be positive (Q must be positive definite)'),
    'ik_qp-kjnan': (EINVAL, 'ik_qp: kj and ks must be positive (Q must be positive definite)'),
    'ik_qp-kj0+unknown': (EINVAL, 'ik_qp: kj and ks must be positive (Q must be positive definite)'),
    'ik_qp-negN': (EINVAL, 'ik_lm: negative N'),
    'ik_qp-mem7': (EINVAL, 'ik_lm: bad mem kind'),
    'ik_qp-ilimit0': (EINVAL, 'ik_lm: ilimit and slimit must be >= 1'),
    'ik_qp-qwidth': (EINVAL, 'ik_lm: chain must use jindex 0..n-1 (reference ik.cpp:34-37 assumes the same)'),
    'ik_qp-nullout': (EINVAL, 'ik_lm: NULL output'),
    'ik_qp-empty': (OK, None),
    'ik_restart-bad': (EINVAL, 'ik_restart: bad argument'),
    'ik_restart-nullout': (EINVAL, 'ik_restart: bad argument'),
    'ik_target_base-negative': (EINVAL, 'ik_target_base: negative base'),
    'rne-unknown': (EINVAL, 'rne: unknown dyn handle'),
    'rne-negN': (EINVAL, 'rne: negative N'),
    'rne-nullq': (EINVAL, 'rne: NULL input with N > 0'),
    'rne-mem7': (EINVAL, 'rne: bad mem kind'),
    'rne-nullgrav': (EINVAL, 'rne: NULL gravity'),
    'rne-nulltau': (EINVAL, 'rne: NULL tau'),
    'rne-unknown+negN': (EINVAL, 'rne: unknown dyn handle'),
    'rne-mem7+nullgrav': (EINVAL, 'rne: bad mem kind'),
    'rne-nullgrav+nulltau': (EINVAL, 'rne: NULL gravity'),
    'rne-empty+nullgrav': (EINVAL, 'rne: NULL gravity'),
    'rne-empty': (OK, None),
    'rne-treehandle': (EINVAL, 'rne: unknown dyn handle'),
    'rne_f32-unknown': (EINVAL, 'rne_f32: unknown dyn handle'),
    'rne_f32-negN': (EINVAL, 'rne_f32: negative N'),
    'rne_f32-nullq': (EINVAL, 'rne_f32: NULL input with N > 0'),
    'rne_f32-mem7': (EINVAL, 'rne_f32: bad mem kind'),
    'rne_f32-nullgrav': (EINVAL, 'rne_f32: NULL gravity'),
    'rne_f32-nulltau': (EINVAL, 'rne_f32: NULL tau'),
    'rne_f32-unknown+negN': (EINVAL, 'rne_f32: unknown dyn handle'),
    'rne_f32-mem7+nullgrav': (EINVAL, 'rne_f32: bad mem kind'),
    'rne_f32-nullgrav+nulltau': (EINVAL, 'rne_f32: NULL gravity'),
    'rne_f32-empty+nullgrav': (EINVAL, 'rne_f32: NULL gravity'),
    'rne_f32-empty': (OK, None),
    'rne_f32-treehandle': (EINVAL, 'rne_f32: unknown dyn handle'),
    'rne_f32-hostmem': (EINVAL, 'rne_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'rne_f32-hostmem+nullgrav': (EINVAL, 'rne_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'rne_f32-hostmem-empty': (EINVAL, 'rne_f32: float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)'),
    'rne_base_wrench-unknown': (EINVAL, 'rne_base_wrench: unknown dyn handle'),
    'rne_base_wrench-negN': (EINVAL, 'rne_base_wrench: negative N'),
    'rne_base_wrench-nullq': (EINVAL, 'rne_base_wrench: NULL input with N > 0'),
    'rne_base_wrench-mem7': (EINVAL, 'rne_base_wrench: bad mem kind'),
    'rne_base_wrench-nullgrav': (EINVAL, 'rne_base_wrench: NULL gravity'),
    'rne_base_wrench-nulltau': (EINVAL, 'rne_base_wrench: NULL tau'),
    'rne_base_wrench-unknown+negN': (EINVAL, 'rne_base_wrench: unknown dyn handle'),
    'rne_base_wrench-mem7+nullgrav': (EINVAL, 'rne_base_wrench: bad mem kind'),
    'rne_base_wrench-nullgrav+nulltau': (EINVAL, 'rne_base_wrench: NULL gravity'),
    'rne_base_wrench-empty+nullgrav': (EINVAL, 'rne_base_wrench: NULL gravity'),
    'rne_base_wrench-empty': (OK, None),
    'rne_base_wrench-treehandle': (EINVAL, 'rne_base_wrench: unknown dyn handle'),
    'rne_base_wrench-nullwbase': (EINVAL, 'rne_base_wrench: NULL wbase'),
    'inertia-unknown': (EINVAL, 'inertia: unknown dyn handle'),
    'inertia-otherkind': (EINVAL, 'inertia: unknown dyn handle'),
    'inertia-negN': (EINVAL, 'inertia: negative N'),
    'inertia-nullq': (EINVAL, 'inertia: NULL input with N > 0'),
    'inertia-mem7': (EINVAL, 'inertia: bad mem kind'),
    'inertia-nullout': (EINVAL, 'inertia: NULL output'),
    'inertia-unknown+mem7': (EINVAL, 'inertia: unknown dyn handle'),
    'inertia-mem7+nullout': (EINVAL, 'inertia: bad mem kind'),
    'inertia-empty': (OK, None),
    'inertia-empty-dev': (OK, None),
    'coriolis-unknown': (EINVAL, 'coriolis: unknown dyn handle'),
    'coriolis-otherkind': (EINVAL, 'coriolis: unknown dyn handle'),
    'coriolis-negN': (EINVAL, 'coriolis: negative N'),
    'coriolis-nullq': (EINVAL, 'coriolis: NULL input with N > 0'),
    'coriolis-mem7': (EINVAL, 'coriolis: bad mem kind'),
    'coriolis-nullout': (EINVAL, 'coriolis: NULL output'),
    'coriolis-unknown+mem7': (EINVAL, 'coriolis: unknown dyn handle'),
    'coriolis-mem7+nullout': (EINVAL, 'coriolis: bad mem kind'),
    'coriolis-nullqd': (EINVAL, 'coriolis: NULL qd'),
    'coriolis-nullout+nullqd': (EINVAL, 'coriolis: NULL output'),
    'coriolis-empty': (OK, None),
    'coriolis-empty-dev': (OK, None),
    'accel-unknown': (EINVAL, 'accel: unknown dyn handle'),
    'accel-otherkind': (EINVAL, 'accel: unknown dyn handle'),
    'accel-negN': (EINVAL, 'accel: negative N'),
    'accel-nullq': (EINVAL, 'accel: NULL input with N > 0'),
    'accel-mem7': (EINVAL, 'accel: bad mem kind'),
    'accel-nullout': (EINVAL, 'accel: NULL output'),
    'accel-unknown+mem7': (EINVAL, 'accel: unknown dyn handle'),
    'accel-mem7+nullout': (EINVAL, 'accel: bad mem kind'),
    'accel-nullqd': (EINVAL, 'accel: NULL qd'),
    'accel-nullout+nullqd': (EINVAL, 'accel: NULL output'),
    'accel-nulltorque': (EINVAL, 'accel: NULL torque/gravity'),
    'accel-nullgrav': (EINVAL, 'accel: NULL torque/gravity'),
    'accel-nullqd+nulltorque': (EINVAL, 'accel: NULL qd'),
    'accel-empty': (OK, None),
    'accel-empty-dev': (OK, None),
    'tree_inertia-unknown': (EINVAL, 'tree_inertia: unknown tree handle'),
    'tree_inertia-otherkind': (EINVAL, 'tree_inertia: unknown tree handle'),
    'tree_inertia-negN': (EINVAL, 'tree_inertia: negative N'),
    'tree_inertia-nullq': (EINVAL, 'tree_inertia: NULL input with N > 0'),
    'tree_inertia-mem7': (EINVAL, 'tree_inertia: bad mem kind'),
    'tree_inertia-nullout': (EINVAL, 'tree_inertia: NULL output'),
    'tree_inertia-unknown+mem7': (EINVAL, 'tree_inertia: unknown tree handle'),
    'tree_inertia-mem7+nullout': (EINVAL, 'tree_inertia: bad mem kind'),
    'tree_inertia-empty': (OK, None),
    'tree_inertia-empty-dev': (OK, None),
    'tree_coriolis-unknown': (EINVAL, 'tree_coriolis: unknown tree handle'),
    'tree_coriolis-otherkind': (EINVAL, 'tree_coriolis: unknown tree handle'),
    'tree_coriolis-negN': (EINVAL, 'tree_coriolis: negative N'),
    'tree_coriolis-nullq': (EINVAL, 'tree_coriolis: NULL input with N > 0'),
    'tree_coriolis-mem7': (EINVAL, 'tree_coriolis: bad mem kind'),
    'tree_coriolis-nullout': (EINVAL, 'tree_coriolis: NULL output'),
    'tree_coriolis-unknown+mem7': (EINVAL, 'tree_coriolis: unknown tree handle'),
    'tree_coriolis-mem7+nullout': (EINVAL, 'tree_coriolis: bad mem kind'),
    'tree_coriolis-nullqd': (EINVAL, 'tree_coriolis: NULL qd'),
    'tree_coriolis-nullout+nullqd': (EINVAL, 'tree_coriolis: NULL output'),
    'tree_coriolis-empty': (OK, None),
    'tree_coriolis-empty-dev': (OK, None),
    'tree_accel-unknown': (EINVAL, 'tree_accel: unknown tree handle'),
    'tree_accel-otherkind': (EINVAL, 'tree_accel: unknown tree handle'),
    'tree_accel-negN': (EINVAL, 'tree_accel: negative N'),
    'tree_accel-nullq': (EINVAL, 'tree_accel: NULL input with N > 0'),
    'tree_accel-mem7': (EINVAL, 'tree_accel: bad mem kind'),
    'tree_accel-nullout': (EINVAL, 'tree_accel: NULL output'),
    'tree_accel-unknown+mem7': (EINVAL, 'tree_accel: unknown tree handle'),
    'tree_accel-mem7+nullout': (EINVAL, 'tree_accel: bad mem kind'),
    'tree_accel-nullqd': (EINVAL, 'tree_accel: NULL qd'),
    'tree_accel-nullout+nullqd': (EINVAL, 'tree_accel: NULL output'),
    'tree_accel-nulltorque': (EINVAL, 'tree_accel: NULL torque/gravity'),
    'tree_accel-nullgrav': (EINVAL, 'tree_accel: NULL torque/gravity'),
    'tree_accel-nullqd+nulltorque': (EINVAL, 'tree_accel: NULL qd'),
    'tree_accel-empty': (OK, None),
    'tree_accel-empty-dev': (OK, None),
    'tree_rne-unknown': (EINVAL, 'tree_rne: unknown tree handle'),
    'tree_rne-dynhandle': (EINVAL, 'tree_rne: unknown tree handle'),
    'tree_rne-negN': (EINVAL, 'tree_rne: negative N'),
    'tree_rne-nullq': (EINVAL, 'tree_rne: NULL input with N > 0'),
    'tree_rne-mem7': (EINVAL, 'tree_rne: bad mem kind'),
    'tree_rne-nullgrav': (EINVAL, 'tree_rne: NULL gravity'),
    'tree_rne-nulltau': (EINVAL, 'tree_rne: NULL tau'),
    'tree_rne-unknown+negN': (EINVAL, 'tree_rne: unknown tree handle'),
    'tree_rne-mem7+nullgrav': (EINVAL, 'tree_rne: bad mem kind'),
    'tree_rne-nullgrav+nulltau': (EINVAL, 'tree_rne: NULL gravity'),
    'tree_rne-empty+nullgrav': (EINVAL, 'tree_rne: NULL gravity'),
    'tree_rne-empty': (OK, None),
    'fleet_fkine_jacob-negchains': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-nullchains': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-nullq': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-nullN': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-nullT': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-nullJ': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-frame3': (EINVAL, 'fleet: frame must be 0 or 1'),
    'fleet_fkine_jacob-mem7': (EINVAL, 'fleet: bad mem kind'),
    'fleet_fkine_jacob-unknown': (EINVAL, 'fleet: unknown chain handle'),
    'fleet_fkine_jacob-negN': (EINVAL, 'fleet: negative N'),
    'fleet_fkine_jacob-nullbuffer-q': (EINVAL, 'fleet: NULL buffer'),
    'fleet_fkine_jacob-nullbuffer-T': (EINVAL, 'fleet: NULL buffer'),
    'fleet_fkine_jacob-nullbuffer-J': (EINVAL, 'fleet: NULL buffer'),
    'fleet_fkine_jacob-nullT+frame3': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob-frame3+mem7': (EINVAL, 'fleet: frame must be 0 or 1'),
    'fleet_fkine_jacob-mem7+unknown': (EINVAL, 'fleet: bad mem kind'),
    'fleet_fkine_jacob-unknown-first+negN': (EINVAL, 'fleet: unknown chain handle'),
    'fleet_fkine_jacob-negN-first+unknown': (EINVAL, 'fleet: negative N'),
    'fleet_fkine_jacob-nochains': (OK, None),
    'fleet_fkine_jacob-empty': (OK, None),
    'fleet_fkine_jacob-empty-dev-null': (OK, None),
    'fleet_fkine_jacob_packed-negchains': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-nullchains': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-nullq': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-nullN': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-nullT': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-frame3': (EINVAL, 'fleet: frame must be 0 or 1'),
    'fleet_fkine_jacob_packed-mem7': (EINVAL, 'fleet: bad mem kind'),
    'fleet_fkine_jacob_packed-unknown': (EINVAL, 'fleet: unknown chain handle'),
    'fleet_fkine_jacob_packed-negN': (EINVAL, 'fleet: negative N'),
    'fleet_fkine_jacob_packed-nullbuffer-q': (EINVAL, 'fleet: NULL buffer'),
    'fleet_fkine_jacob_packed-nullbuffer-T': (EINVAL, 'fleet: NULL buffer'),
    'fleet_fkine_jacob_packed-nullT+frame3': (EINVAL, 'fleet: bad argument'),
    'fleet_fkine_jacob_packed-frame3+mem7': (EINVAL, 'fleet: frame must be 0 or 1'),
    'fleet_fkine_jacob_packed-mem7+unknown': (EINVAL, 'fleet: bad mem kind'),
    'fleet_fkine_jacob_packed-unknown-first+negN': (EINVAL, 'fleet: unknown chain handle'),
    'fleet_fkine_jacob_packed-negN-first+unknown': (EINVAL, 'fleet: negative N'),
    'fleet_fkine_jacob_packed-nochains': (OK, None),
    'fleet_fkine_jacob_packed-empty': (OK, None),
    'fleet_fkine_jacob_packed-empty-dev-null': (OK, None),
    'stream_probe-negread': (EINVAL, 'stream_probe: bad argument'),
    'stream_probe-nullsrc': (EINVAL, 'stream_probe: bad argument'),
    'stream_probe-nulldst': (EINVAL, 'stream_probe: bad argument'),
}


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def call(x, fn, make):
    """-> (return code, rtbhip_last_error() after a refusal)."""
    args = tuple(x.one if a is ONE else a for a in make(x))
    rc = getattr(_lib.lib(), fn)(*args)
    return rc, (_lib.lib().rtbhip_last_error().decode() if rc != 0 else None)


def test_the_table_names_every_compute_entry_point():
    """every symbol of include/rtbhip.h that computes on a batch has rows here, an empty-batch row among them"""
    compute = {n for n, (_, a) in _lib.SIGNATURES.items() if len(a) >= 2 and a[-1] == _lib._vp and a[-2] == _lib._i32 and n not in ("rtbhip_device_copy", "rtbhip_ik_restart")}     # (..., mem, stream) by shape, not batch calls
    assert len(compute) >= 35, sorted(compute)
    covered = {fn for _, fn, _ in ROWS}
    assert compute <= covered, sorted(compute - covered)
    ok = {fn for rid, fn, _ in ROWS if EXPECTED[rid][0] == OK}
    assert compute <= ok, sorted(compute - ok)
    assert len({rid for rid, _, _ in ROWS}) == len(ROWS) == len(EXPECTED)


@pytest.mark.parametrize("rid,fn,make", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, rid, fn, make):
    assert call(ctx, fn, make) == EXPECTED[rid]
