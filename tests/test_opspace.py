"""Operational-space dynamics on the device: rtbhip_opspace / rtbhip_tree_opspace and the functions of rtbhip/opspace.py.

The oracle and its bound are those of tests/opspace_cases.py: oracle.inertia_dh / erobot_inertia, oracle.rne_dh / erobot_rne, oracle.jacob0 and
numpy.linalg.inv / pinv / eig restating the reference's single-q formulas; per row K eps cond(J)^2 max|ref| (1 for the Asada ratio), K = 8 x
the CPU replay's largest ratio (tests/test_opspace_emu.py).

No GPU is needed for the exports and for the refusals that look at arguments only."""
import ctypes as C
import os

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib, opspace
from helpers import replaying
import opspace_cases as cases

OK, EINVAL, ELIMIT = 0, -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "opspace_reference.npz")
N = 129          # two full tiles and a row


def _torch():
    return pytest.importorskip("torch")


def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the operational-space kernels run on the device only: not served by the CPU replay")(f))


def _handle(name):
    rb = cases.robot(name)
    return ("rtbhip_tree_opspace", rb._handle()) if cases.is_tree(name) else ("rtbhip_opspace", rb._dyn_handle())


# ------------------------------------------------------------------------------------------------ exports and refusals (no GPU)
@pytest.mark.parametrize("fn", ["rtbhip_opspace", "rtbhip_tree_opspace"])
def test_symbols_are_exported_and_declared(fn):
    hdr = open(os.path.join(ROOT, "include", "rtbhip.h")).read()
    assert hasattr(_lib.lib(), fn) and fn in _lib.SIGNATURES and ("int %s(" % fn) in hdr
    res, args = _lib.SIGNATURES[fn]
    assert res is C.c_int and len(args) == 10 and args[0] is _lib._u64 and args[3] is _lib._i64 and args[5] is _lib._i32
    assert args[-1] is _lib._vp and args[-2] is _lib._vp          # outputs last, then stream: no mem argument
    for cite in ("robot/Dynamics.py:924-1025", "robot/Dynamics.py:1173-1290", "robot/Robot.py:871-881", "max(6, n) eps lambda_max", "(N, 6) for any n",
                 "NOT REPRODUCED"):
        assert cite in hdr, cite


def _refused(fn, args, rc, msg):
    got = getattr(_lib.lib(), fn)(*args)
    assert got == rc, (got, _lib.lib().rtbhip_last_error())
    if msg is not None:
        assert _lib.lib().rtbhip_last_error().decode() == msg


def test_argument_refusals():
    buf = np.zeros(4096)
    B = buf.ctypes.data
    g = np.zeros(3).ctypes.data
    for name in ("puma560", "UR5"):
        fn, h = _handle(name)
        P = fn[len("rtbhip_"):] + ": "
        _refused(fn, (987654321, B, B, 4, g, 63, B, B, B, None), EINVAL, P + "unknown %s handle" % ("tree" if "tree" in fn else "dyn"))
        _refused(fn, (h, B, B, -1, g, 63, B, B, B, None), EINVAL, P + "negative N")
        _refused(fn, (h, B, B, 4, g, 63, None, None, None, None), EINVAL, P + "Mx, Gx and asada are all NULL: there is nothing to compute")
        _refused(fn, (h, B, B, 0, g, 63, None, None, None, None), EINVAL, P + "Mx, Gx and asada are all NULL: there is nothing to compute")
        _refused(fn, (h, None, B, 4, g, 63, B, B, B, None), EINVAL, P + "NULL input with N > 0")
        _refused(fn, (h, B, None, 4, g, 63, B, B, B, None), EINVAL, P + "NULL input with N > 0")
        _refused(fn, (h, B, B, 4, None, 63, B, B, B, None), EINVAL, P + "NULL gravity with a Gx output")
        _refused(fn, (h, B, B, 4, g, 64, B, B, B, None), EINVAL, P + "axes_mask selects no task-space row")
        _refused(fn, (h, B, B, 8 * 2 ** 31, g, 63, B, B, B, None), ELIMIT, P + "batch too large for one launch")
        # N = 0: OK without a launch, no pointer looked at (gravity may be NULL without Gx)
        before = rtbhip.last_launch()
        _refused(fn, (h, None, None, 0, None, 63, B, None, B, None), OK, None)
        assert rtbhip.last_launch() == before and not buf.any()


def test_more_than_sixteen_joints_is_a_limit():
    import rne_vjp_cases as dhc
    rb = dhc.random_robot(17, 0, 5)
    B = np.zeros(4096).ctypes.data
    _refused("rtbhip_opspace", (rb._dyn_handle(), B, B, 1, None, 63, B, None, None, None), ELIMIT, "opspace: robots of 1..16 joints")
    _refused("rtbhip_opspace", (rb._dyn_handle(), B, B, 0, None, 63, B, None, None, None), ELIMIT, "opspace: robots of 1..16 joints")


def test_the_hand_numbered_tree_is_refused():
    rb = cases.robot(cases.REFUSED)
    B = np.zeros(4096).ctypes.data
    msg = "tree_opspace: the robot is not numbered in group order (joint j of the q row must be moved by link group j)"
    _refused("rtbhip_tree_opspace", (rb._handle(), B, B, 3, None, 63, B, None, None, None), EINVAL, msg)
    _refused("rtbhip_tree_opspace", (rb._handle(), B, B, 0, None, 63, B, None, None, None), EINVAL, msg)


def test_front_end_refusals_that_need_no_device():
    puma = cases.robot("puma560")
    with pytest.raises(ValueError, match="needs q"):
        opspace.manipulability(puma, None, J=np.eye(6))
    with pytest.raises(ValueError, match="serves method"):
        opspace.manipulability(puma, np.zeros(6), method="yoshikawa")
    with pytest.raises(TypeError, match="end"):
        opspace.inertia_x(puma, np.zeros(6), end="link3")
    tree = cases.robot("tree7")                                     # a branched tree: no path moves all seven joints
    with pytest.raises(ValueError, match="of the robot's 7 joints"):
        opspace.inertia_x(tree, np.zeros(7))
    with pytest.raises(ValueError, match="of the robot's 7 joints"):
        opspace.manipulability(tree, np.zeros(7))
    with pytest.raises(TypeError, match="no dynamics"):
        opspace.inertia_x(rtbhip.models.Panda(), np.zeros(7))


# ------------------------------------------------------------------------------------------------ the device: raw ABI
def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(torch, name, q, J, axes=63, want=(True, True, True), guarded=False):
    """-> [Mx (n, 6, 6), Gx (n, 6), asada (n,)] as NumPy (None where not wanted)"""
    from flush_guard import Guarded
    fn, h = _handle(name)
    n = q.shape[0]
    dq, dJ = torch.from_numpy(np.array(q)).cuda(), torch.from_numpy(np.array(J)).cuda()
    widths = (36, 6, 1)
    if guarded:
        outs = [Guarded(torch, n, w, "float64") if k else None for w, k in zip(widths, want)]
        ptrs = [None if o is None else o.ptr for o in outs]
    else:
        outs = [torch.full((n, w), float("nan"), dtype=torch.float64, device="cuda") if k else None for w, k in zip(widths, want)]
        ptrs = [_ptr(o) for o in outs]
    g = cases.gravity3(name)
    rc = getattr(_lib.lib(), fn)(h, _ptr(dq), _ptr(dJ), n, _lib.host_ptr(g), axes, ptrs[0], ptrs[1], ptrs[2], _stream(torch))
    assert rc == OK, _lib.lib().rtbhip_last_error()
    torch.cuda.synchronize()
    if guarded:
        assert all(o is None or o.guards_intact() for o in outs), "a guard row changed"
        outs = [None if o is None else o.live() for o in outs]
    shapes = ((n, 6, 6), (n, 6), (n,))
    return [None if o is None else o.cpu().numpy().reshape(s) for o, s in zip(outs, shapes)]


def _tiled(name, n=N):
    q, J, _, _ = cases.inputs(name)
    ref = cases.reference(name)
    return cases.tiled(q, n), cases.tiled(J, n), {k: cases.tiled(v, n) for k, v in ref.items()}


@gpu
@pytest.mark.parametrize("name", cases.ALL)
def test_every_row_equals_the_oracle_between_guard_rows(name):
    torch = _torch()
    q, J, ref = _tiled(name)
    for key, mask in cases.AXES.items():
        Mx, Gx, asada = _raw(torch, name, q, J, axes=mask, guarded=True)
        r = [cases.ratio(Mx, ref["Mx"], ref["cond"]), cases.ratio(Gx, ref["Gx"], ref["cond"])]
        if name not in cases.NONSYMMETRIC:
            r.append(cases.ratio(asada, ref[key], ref["cond"], unit=True))
        print("opspace device %s/%s (n = %d): err / (eps cond^2 |ref|max) = %s" % (name, key, q.shape[1], ", ".join("%.3f" % x for x in r)))
        assert max(r) <= cases.K
        if q.shape[1] < 6:
            assert not asada.any()


@gpu
@pytest.mark.parametrize("name", cases.ALL)
def test_rows_are_independent_bit_for_bit(name):
    """N = 129 against a permuted batch, and against rows of the permuted batch taken one at a time"""
    torch = _torch()
    q, J, _ = _tiled(name)
    full = _raw(torch, name, q, J)
    perm = np.random.default_rng(3).permutation(N)
    shuffled = _raw(torch, name, q[perm], J[perm])
    for a, b in zip(full, shuffled):
        assert np.array_equal(a[perm], b)
    for i in (0, 63, 64, 128):
        one = _raw(torch, name, q[perm][i:i + 1], J[perm][i:i + 1])
        for a, b in zip(shuffled, one):
            assert np.array_equal(a[i:i + 1], b)


@gpu
@pytest.mark.parametrize("name", ["n3s", "puma560", "panda", "n9s", "mdhp6", "KinovaGen3"])
def test_a_null_output_is_neither_computed_nor_stored(name):
    torch = _torch()
    q, J, _ = _tiled(name)
    full = _raw(torch, name, q, J)
    for want in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        got = _raw(torch, name, q, J, want=want, guarded=True)
        for o, f, w in zip(got, full, want):
            assert (o is None) == (not w)
            if w:
                assert np.array_equal(o, f)


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n9s", "UR5"])
def test_a_singular_row_touches_no_other_row(name):
    torch = _torch()
    q, J, _ = _tiled(name)
    full = _raw(torch, name, q, J)
    J2 = np.array(J)
    J2[33] = 0.0
    J2[64, 2] = J2[64, 1]
    J2[128] = np.nan
    got = _raw(torch, name, q, J2, guarded=True)
    keep = np.ones(N, bool)
    keep[[33, 64, 128]] = False
    for o, f in zip(got, full):
        assert np.array_equal(o[keep], f[keep])
    assert not np.isfinite(got[0][33]).all() and not np.isfinite(got[0][128]).any() and not np.isfinite(got[1][128]).any()
    assert got[2][64] == 0.0


@gpu
def test_asada_is_zero_at_puma_qz():
    torch = _torch()
    q = np.zeros((5, 6))
    assert not _raw(torch, "puma560", q, cases.jacob0("puma560", q), want=(0, 0, 1))[2].any()


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda"])
def test_the_device_equals_the_reference_classes(name):
    """tests/golden/opspace_reference.npz: what the reference's own DHRobot.inertia_x / gravload_x / manipulability(method="asada") returned"""
    torch = _torch()
    z = np.load(GOLDEN)
    q, J = z[name + "_q"], z[name + "_J"]
    rb = cases.robot(name)
    cond = np.array([np.linalg.cond(Ji) for Ji in J])
    ok = cond <= cases.COND_MAX
    assert ok.sum() >= 6
    for key in cases.AXES:
        Mx = opspace.inertia_x(rb, q[ok], representation=None)
        Gx = opspace.gravload_x(rb, q[ok], representation=None)
        a = opspace.manipulability(rb, q[ok], axes=key)
        assert cases.ratio(Mx, z[name + "_Mx"][ok], cond[ok]) <= cases.K
        assert cases.ratio(Gx, z[name + "_Gx"][ok], cond[ok]) <= cases.K
        assert cases.ratio(a, z[name + "_asada_" + key][ok], cond[ok], unit=True) <= cases.K
    if (~ok).any():
        assert not np.asarray(opspace.manipulability(rb, q[~ok])).any() and not z[name + "_asada_all"][~ok].any()


# ------------------------------------------------------------------------------------------------ the device: front end
@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "n3s", "UR5", "KinovaGen3"])
def test_shapes_memory_kinds_and_the_oracle(name):
    torch = _torch()
    rb = cases.robot(name)
    q, J, _, _ = cases.inputs(name)
    ref = cases.reference(name)
    end = cases.end_link(name)
    kw = dict(end=end) if cases.is_tree(name) else {}
    # NumPy in, NumPy out; 2-D q adds the batch axis
    Mx = opspace.inertia_x(rb, q, representation=None, **kw)
    Gx = opspace.gravload_x(rb, q, gravity=cases.GRAVITY, representation=None, **kw)
    a = opspace.manipulability(rb, q, **kw)
    assert isinstance(Mx, np.ndarray) and Mx.shape == (cases.ROWS, 6, 6) and Gx.shape == (cases.ROWS, 6) and a.shape == (cases.ROWS,)
    assert cases.ratio(Mx, ref["Mx"], ref["cond"]) <= cases.K and cases.ratio(Gx, ref["Gx"], ref["cond"]) <= cases.K
    assert cases.ratio(a, ref["all"], ref["cond"], unit=True) <= cases.K
    # 1-D q: (6, 6), (6,), a scalar -- the bits of row 0
    m0, g0, a0 = opspace.inertia_x(rb, q[0], representation=None, **kw), opspace.gravload_x(rb, q[0], gravity=cases.GRAVITY, representation=None, **kw), opspace.manipulability(rb, q[0], **kw)
    assert m0.shape == (6, 6) and g0.shape == (6,) and isinstance(a0, float)
    assert np.array_equal(m0, Mx[0]) and np.array_equal(g0, Gx[0]) and a0 == a[0]
    # CUDA float64 in, tensors out, bit for bit what NumPy got; requires_grad changes nothing
    qt = torch.from_numpy(np.array(q)).cuda()
    Mt, Gt, at = opspace.inertia_x(rb, qt, representation=None, **kw), opspace.gravload_x(rb, qt, gravity=cases.GRAVITY, representation=None, **kw), opspace.manipulability(rb, qt, **kw)
    assert Mt.is_cuda and Mt.dtype == torch.float64 and tuple(Mt.shape) == (cases.ROWS, 6, 6) and tuple(Gt.shape) == (cases.ROWS, 6) and tuple(at.shape) == (cases.ROWS,)
    assert np.array_equal(Mt.cpu().numpy(), Mx) and np.array_equal(Gt.cpu().numpy(), Gx) and np.array_equal(at.cpu().numpy(), a)
    qg = qt.clone().requires_grad_(True)
    Mg = opspace.inertia_x(rb, qg, representation=None, **kw)
    assert not Mg.requires_grad and torch.equal(Mg, Mt)
    s = opspace.manipulability(rb, qt[0], **kw)
    assert s.dim() == 0 and float(s) == a[0]
    # J= with q: the same launch on the caller's Jacobian (the robot's own jacob0: the bits of the launch without J=)
    assert np.array_equal(opspace.manipulability(rb, q, J=rb.jacob0(q, **kw), axes="trans"), opspace.manipulability(rb, q, axes="trans", **kw))
    assert torch.equal(opspace.manipulability(rb, qt, J=rb.jacob0(qt, **kw), axes="rot"), opspace.manipulability(rb, qt, axes="rot", **kw))
    assert cases.ratio(opspace.manipulability(rb, q, J=J, axes="rot"), ref["rot"], ref["cond"], unit=True) <= cases.K          # and the oracle's
    both = opspace.manipulability(rb, q, axes="both", **kw)
    assert isinstance(both, tuple) and np.array_equal(both[0], opspace.manipulability(rb, q, axes="trans", **kw))
    # float32 is refused as elsewhere
    with pytest.raises(TypeError, match="float64"):
        opspace.inertia_x(rb, qt.float(), representation=None, **kw)


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda"])
@pytest.mark.parametrize("representation", ["rpy/xyz", "rpy/zyx", "eul", "exp", None])
def test_every_representation(name, representation):
    rb = cases.robot(name)
    q = cases.inputs(name)[0]
    Ja = cases.jacob0(name, q, representation)
    cond = np.array([np.linalg.cond(Ji) for Ji in Ja])
    ok = cond <= cases.COND_MAX                  # a rate transform has singularities of its own: those rows are another Jacobian's ill-conditioned rows
    print("opspace %s/%s: %d of %d rows within cond <= %g" % (name, representation, ok.sum(), len(ok), cases.COND_MAX))
    assert 2 * ok.sum() >= len(ok)
    M, g = cases.inertia(name, q), cases.gravload(name, q)
    want = [cases.formula(M[i], g[i], Ja[i]) for i in np.flatnonzero(ok)]
    Mx = opspace.inertia_x(rb, q[ok], representation=representation)
    Gx = opspace.gravload_x(rb, q[ok], gravity=cases.GRAVITY, representation=representation)
    assert cases.ratio(Mx, np.array([w[0] for w in want]), cond[ok]) <= cases.K
    assert cases.ratio(Gx, np.array([w[1] for w in want]), cond[ok]) <= cases.K
    if representation == "rpy/xyz":              # the default
        assert np.array_equal(opspace.inertia_x(rb, q[ok]), Mx) and np.array_equal(opspace.inertia_x(rb, q[ok], pinv=True), Mx)
    with pytest.raises(ValueError):
        opspace.inertia_x(rb, q, representation="quaternion")


@gpu
@pytest.mark.parametrize("name", ["puma560", "panda", "UR5"])
def test_a_supplied_inverse_is_used_as_it_is(name):
    torch = _torch()
    rb = cases.robot(name)
    q, J, _, _ = cases.inputs(name)
    Ji = np.linalg.pinv(J)                       # (ROWS, n, 6)
    M, g = rb.inertia(q), rb.gravload(q)
    Mx, Gx = opspace.inertia_x(rb, q, Ji=Ji), opspace.gravload_x(rb, q, Ji=Ji)
    assert np.array_equal(Mx, np.swapaxes(Ji, 1, 2) @ M @ Ji) and np.array_equal(Gx, (np.swapaxes(Ji, 1, 2) @ g[..., None])[..., 0])
    assert np.array_equal(opspace.inertia_x(rb, q[0], Ji=Ji[0]), Ji[0].T @ rb.inertia(q[0]) @ Ji[0])
    qt, Jt = torch.from_numpy(np.array(q)).cuda(), torch.from_numpy(Ji).cuda()
    Mt = opspace.inertia_x(rb, qt, Ji=Jt)
    assert Mt.is_cuda and torch.equal(Mt, Jt.transpose(1, 2) @ rb.inertia(qt) @ Jt)
    ref = cases.reference(name)
    assert cases.ratio(Mx, ref["Mx"], ref["cond"]) <= cases.K


@gpu
def test_the_reference_test_bodies_on_the_dh_puma():
    """the bodies of the reference's tests/test_DHRobot.py test_inertia_x and test_asada on rtbhip.models.DH.Puma560(), the expected values from the
    oracle (to the reference's four decimals and to this file's bound)"""
    import numpy.testing as nt
    puma = rtbhip.models.DH.Puma560()
    q = puma.qn
    J = cases.jacob0("puma560", np.array([q, puma.qz]))
    M, g = cases.inertia("puma560", q.reshape(1, 6))[0], cases.gravload("puma560", q.reshape(1, 6))[0]
    Mr = cases.formula(M, g, J[0])[0]
    M0 = opspace.inertia_x(puma, q, representation=None)
    M1 = opspace.inertia_x(puma, np.c_[q, q].T, representation=None)
    nt.assert_array_almost_equal(M0, Mr, decimal=4)
    nt.assert_array_almost_equal(M1[0, :, :], Mr, decimal=4)
    nt.assert_array_almost_equal(M1[1, :, :], Mr, decimal=4)
    bound = cases.K * cases.EPS * np.linalg.cond(J[0]) ** 2
    assert np.abs(M0 - Mr).max() <= bound * np.abs(Mr).max() and np.array_equal(M1[0], M0) and np.array_equal(M1[1], M0)
    m1 = opspace.manipulability(puma, q, method="asada")
    m2 = opspace.manipulability(puma, np.c_[q, q].T, method="asada")
    m3 = opspace.manipulability(puma, q, axes="trans", method="asada")
    m4 = opspace.manipulability(puma, q, axes="rot", method="asada")
    m5 = opspace.manipulability(puma, puma.qz, method="asada")
    a0, a2, a3 = (cases.formula(M, g, J[0], cases.AXES[k])[2] for k in ("all", "trans", "rot"))
    a4 = 0.0
    assert np.linalg.matrix_rank(J[1]) < 6
    for got, want in ((m1, a0), (m2[0], a0), (m2[1], a0), (m3, a2), (m4, a3), (m5, a4)):
        nt.assert_almost_equal(got, want, decimal=4)
        assert abs(got - want) <= bound
