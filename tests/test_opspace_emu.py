"""The operational-space dynamics on the CPU (no GPU needed): the lane body and the tile fill / flush phases of k_opspace / k_tree_opspace
(csrc/opspace_device.h) compiled host-side for this test (tests/emu_opspace/emu_opspace.cpp, built by tests/opspace_emu_harness.py and linked
against tests/emu/libemu.so for the handle registry and the tree compiler) and held against the oracle of tests/opspace_cases.py -- oracle.inertia_dh / erobot_inertia, oracle.rne_dh /
erobot_rne, oracle.jacob0 and numpy.linalg.inv / pinv / eig -- at its bound, K eps cond(J)^2 max|ref| per row.  The device runs the same source
through another compiler: tests/test_opspace.py."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_harness
import opspace_emu_harness as ops_emu
import opspace_cases as cases

ROOT = emu_harness.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "opspace_reference.npz")
N = 70          # a full tile and a ragged one


@pytest.fixture(scope="module")
def lib():
    """tests/opspace_emu_harness.py builds the library (by parts, in parallel) when the digest of its sources changed"""
    return ops_emu.lib()


def _dyn_handle(name):
    return ops_emu.dyn_handle(cases.robot(name))


def _run(lib, name, q, J, axes=63, want=(True, True, True), fill=np.nan, rc=0):
    """-> [Mx (N, 6, 6), Gx (N, 6), asada (N)]; an output not wanted is handed over as NULL and comes back as the untouched buffer"""
    return ops_emu.run(cases.robot(name), cases.is_tree(name), q, J, cases.gravity3(name), axes, want, fill, rc)


def _tiled(name):
    q, J, _, _ = cases.inputs(name)
    ref = cases.reference(name)
    return cases.tiled(q, N), cases.tiled(J, N), {k: cases.tiled(v, N) for k, v in ref.items()}


def test_the_cases_are_what_they_claim(lib):
    want_n = {"puma560": 6, "panda": 7, "n3s": 3, "n8m": 8, "n9s": 9, "n16s": 16, "pris6": 6, "mdhp6": 6, "UR5": 6, "KinovaGen3": 7, "tree7": 7}
    assert {k: cases.robot(k).n for k in cases.ALL} == want_n and cases.robot(cases.REFUSED).n == 4
    assert cases.robot("panda").mdh == 1 and cases.robot("n8m").mdh == 1 and cases.robot("n9s").mdh == 0
    pr, mp = cases.robot("pris6"), cases.robot("mdhp6")
    assert pr.mdh == 0 and [l.sigma for l in pr.links] == [0, 0, 1, 0, 0, 0]
    assert mp.mdh == 1 and [l.sigma for l in mp.links] == [1, 0, 0, 0, 0, 0]
    M = cases.inertia("mdhp6", cases.inputs("mdhp6")[0])
    assert np.abs(M - M.transpose(0, 2, 1)).max() > 1e-3 * np.abs(M).max()           # the non-symmetric matrix of the reference's recursion
    assert not cases.robot(cases.REFUSED)._in_group_order() and all(cases.robot(k)._in_group_order() for k in cases.TREES)
    for name in cases.ALL:
        q, J, draws, replaced = cases.inputs(name)
        print("opspace case %s: %d of %d draws replaced (cond > %g)" % (name, replaced, draws, cases.COND_MAX))
        assert 3 * replaced <= draws and cases.reference(name)["cond"].max() <= cases.COND_MAX
    # the layouts the kernels use: packed triangle for all-revolute DH chains and trees, the full tile otherwise; the run-time-n tail from 9 joints
    lay = np.zeros(5, np.int32)
    lib.emu_opspace_layout(7, 1, 1, emu_harness._p(lay))
    assert list(lay) == [28, 0, 28, 70, 71]
    lib.emu_opspace_layout(6, 0, 0, emu_harness._p(lay))
    assert list(lay) == [36, 36, 42, 78, 79]
    lib.emu_opspace_layout(9, 1, 1, emu_harness._p(lay))
    assert list(lay) == [45, 0, 45, 99, 109]


@pytest.mark.parametrize("name", cases.ALL)
def test_lane_body_equals_the_oracle(lib, name):
    q, J, ref = _tiled(name)
    worst = 0.0
    for key, mask in cases.AXES.items():
        Mx, Gx, asada = _run(lib, name, q, J, axes=mask)
        r = [cases.ratio(Mx, ref["Mx"], ref["cond"]), cases.ratio(Gx, ref["Gx"], ref["cond"])]
        if name not in cases.NONSYMMETRIC:
            r.append(cases.ratio(asada, ref[key], ref["cond"], unit=True))
        worst = max(worst, max(r))
        print("opspace lane %s/%s (n = %d): err / (eps cond^2 |ref|max) = %s" % (name, key, q.shape[1], ", ".join("%.3f" % x for x in r)))
        assert max(r) <= cases.K
        if q.shape[1] < 6:
            assert not asada.any()
    print("opspace lane %s: largest ratio %.4f" % (name, worst))


@pytest.mark.parametrize("name", ["n3s", "puma560", "panda", "n9s", "mdhp6", "KinovaGen3"])
def test_a_null_output_is_not_written(lib, name):
    q, J, ref = _tiled(name)
    full = _run(lib, name, q, J)
    for want in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        got = _run(lib, name, q, J, want=want, fill=7.0)
        for o, f, w in zip(got, full, want):
            assert np.array_equal(o, f) if w else (o == 7.0).all()


@pytest.mark.parametrize("name", ["puma560", "panda", "n9s", "UR5"])
def test_a_singular_row_touches_no_other_row(lib, name):
    q, J, ref = _tiled(name)
    full = _run(lib, name, q, J)
    J2 = np.array(J)
    J2[33] = 0.0                                 # a zero Jacobian between finite rows: zero pivots
    J2[64, 2] = J2[64, 1]                        # two equal rows in the ragged tile: rank 5
    got = _run(lib, name, q, J2)
    keep = np.ones(N, bool)
    keep[[33, 64]] = False
    for o, f in zip(got, full):
        assert np.array_equal(o[keep], f[keep])
    assert not np.isfinite(got[0][33]).all() and not np.isfinite(got[1][33]).all()
    assert got[2][64] == 0.0                     # rank-deficient: Asada's measure is 0 whatever Mx holds
    big = np.abs(got[0][64]).max()
    assert not np.isfinite(big) or big > 1e6 * np.abs(full[0][64]).max()


def test_asada_is_zero_at_puma_qz_and_below_six_joints(lib):
    puma = cases.robot("puma560")
    q = np.zeros((N, 6))
    J = cases.jacob0("puma560", q)
    assert np.linalg.matrix_rank(J[0]) < 6
    assert not _run(lib, "puma560", q, J, want=(0, 0, 1))[2].any()
    q3, J3, _ = _tiled("n3s")
    assert not _run(lib, "n3s", q3, J3, want=(0, 0, 1))[2].any()
    assert puma.n == 6


def test_the_hand_numbered_tree_is_refused(lib):
    rb = cases.robot(cases.REFUSED)
    _run(lib, cases.REFUSED, np.zeros((3, rb.n)), np.ones((3, 6, rb.n)), rc=-2)


@pytest.mark.parametrize("name", ["puma560", "panda"])
def test_the_restatement_and_the_replay_equal_the_reference_classes(lib, name):
    """the recorded outputs of the reference's own DHRobot.inertia_x / gravload_x / manipulability(method="asada"): the NumPy restatement of
    opspace_cases and the replayed lane body both reproduce them (geometric Jacobian, representation=None; the reference's default gravity)"""
    z = np.load(GOLDEN)
    q, J = z[name + "_q"], z[name + "_J"]
    rb = cases.robot(name)
    M = cases.inertia(name, q)
    from oracle import oracle
    g = oracle.rne_dh(rb.L24(), rb.mdh, q, np.zeros_like(q), np.zeros_like(q), rb._gravity_c(None))
    cond = np.array([np.linalg.cond(Ji) for Ji in J])
    ok = cond <= cases.COND_MAX
    assert ok.sum() >= 6
    for i in range(q.shape[0]):
        for key, mask in cases.AXES.items():
            if ok[i]:
                Mx, Gx, a = cases.formula(M[i], g[i], J[i], mask)
                assert np.abs(Mx - z[name + "_Mx"][i]).max() <= cases.K * cases.EPS * cond[i] ** 2 * np.abs(Mx).max()
                assert np.abs(Gx - z[name + "_Gx"][i]).max() <= cases.K * cases.EPS * cond[i] ** 2 * np.abs(Gx).max()
                assert abs(a - z[name + "_asada_" + key][i]) <= cases.K * cases.EPS * cond[i] ** 2
            else:                                # qz: the reference's measure is 0 there, and so is the replay's (below)
                assert np.linalg.matrix_rank(J[i]) < 6 and z[name + "_asada_" + key][i] == 0.0
    p = emu_harness._p
    qq, JJ = np.ascontiguousarray(q[ok]), np.ascontiguousarray(J[ok])
    out = [np.full((len(qq), 6, 6), np.nan), np.full((len(qq), 6), np.nan), np.full(len(qq), np.nan)]
    gc = rb._gravity_c(None)
    for key, mask in cases.AXES.items():
        assert lib.emu_opspace(_dyn_handle(name), p(qq), p(JJ), len(qq), p(gc), mask, p(out[0]), p(out[1]), p(out[2])) == 0
        assert cases.ratio(out[0], z[name + "_Mx"][ok], cond[ok]) <= cases.K
        assert cases.ratio(out[1], z[name + "_Gx"][ok], cond[ok]) <= cases.K
        assert cases.ratio(out[2], z[name + "_asada_" + key][ok], cond[ok], unit=True) <= cases.K
    if (~ok).any():
        qb, Jb, a = np.ascontiguousarray(q[~ok]), np.ascontiguousarray(J[~ok]), np.full(int((~ok).sum()), np.nan)
        assert lib.emu_opspace(_dyn_handle(name), p(qb), p(Jb), len(qb), None, 63, None, None, p(a)) == 0 and not a.any()
