"""The two walks of k_kin_reg on the CPU (no GPU needed): reg_compute<NJ, WANT_J, SIG> for the built-in structure signatures against the general
reg_compute<NJ, WANT_J> (csrc/kin_reg.h), byte for byte.

The signature walk multiplies by each constant segment with the general UNFUSED product's specialisation for that segment's exact zeros and ones
(kin_device.h: pose_mul_seg_sig, pose_seg_translate_sum; exactform.h: dotk).  Every rewrite returns the same number for finite operands; what a
rewrite CAN change is the sign of a zero (a dropped `+ 0 x` no longer turns a -0 into +0).  So the rows that make zeros are in: q = 0, -0, +-pi/2,
+-pi, 1e-300, a value >= 2^20, all-zero rows, every joint drawn from those values, and exact zeros mixed into ordinary values -- and the comparison is
on the raw 64-bit words.  On such rows the two column-permutation classes (pure register moves: the UR arms have them) returned the other sign of
zero in about 4 % of the rows; they take the general product inside these kernels (kin_device.h: RTB_SIG_UNFUSED_GENERAL) and this test pins that.
The device runs the same source through another compiler: tests/test_kin_sig_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtbhip
from rtbhip import urdf
import emu_harness

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu", "emu_kin_sig.cpp")
SO = os.path.join(ROOT, "tests", "emu", "libemu_kin_sig.so")
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32

CHAINS = {
    "panda_ets": lambda: rtbhip.models.Panda().ets(),
    "panda_urdf": lambda: urdf.load("Panda").ets(),
    "ur5": lambda: urdf.load("UR5").ets(),
}


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the chain compiler and registry (built if stale)
    import __graft_entry__ as g
    digest = g.source_digest(emu_harness._deps())
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        emu_dir = os.path.dirname(SO)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include"),
                               "-shared", SRC, "-o", SO, "-L" + emu_dir, "-l:libemu.so", "-Wl,-rpath," + emu_dir])
        open(stamp, "w").write(digest)
    so = C.CDLL(SO)
    so.emu_kin_reg_sig.argtypes = [_u64, _vp, _i64, _vp, _i32, _vp, _vp, _i32]
    assert base is not None
    return so


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    big = float(2 ** 20) + 0.5
    special = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e-300, big]
    zeros = np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e-300])
    M = 4000
    rows = [rng.uniform(-np.pi, np.pi, (300, n))]
    rows.append(np.array([np.roll(special, k)[:n] for k in range(7)]))
    rows.append(np.zeros((1, n)))
    rows.append(-np.zeros((1, n)))
    rows.append(zeros[rng.integers(0, len(zeros), (M, n))])                                            # every joint at a zero, a quarter or a half turn
    rows.append(np.where(rng.random((M, n)) < 0.5, 0.0, rng.uniform(-np.pi, np.pi, (M, n))))           # exact zeros among ordinary values
    rows.append(np.where(rng.random((M, n)) < 0.3, zeros[rng.integers(0, len(zeros), (M, n))], rng.uniform(-np.pi, np.pi, (M, n))))
    return np.ascontiguousarray(np.concatenate(rows))


BASE = np.array([[0.0, -1.0, 0.0, 0.1], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, -0.3], [0.0, 0.0, 0.0, 1.0]])


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_signature_walk_returns_the_general_walks_bits_on_the_host(lib, name):
    ets = CHAINS[name]()
    h, n = emu_harness.chain_handle(ets), ets.n
    q = _rows(n, 3)
    N = len(q)
    for frame in (0, 1):
        for base in (None, BASE):
            out = {}
            for use_sig in (1, 0):
                T, J = np.full((N, 16), np.nan), np.full((N, 6 * n), np.nan)
                rc = lib.emu_kin_reg_sig(h, emu_harness._p(q), N, emu_harness._p(base), frame, emu_harness._p(T), emu_harness._p(J), use_sig)
                assert rc == use_sig, rc                                       # 1: the signature instantiation ran, 0: the general walk
                T2 = np.full((N, 16), np.nan)
                assert lib.emu_kin_reg_sig(h, emu_harness._p(q), N, emu_harness._p(base), frame, emu_harness._p(T2), None, use_sig) == use_sig      # fkine alone
                assert np.array_equal(T.view(np.int64), T2.view(np.int64))
                out[use_sig] = (T, J)
            for a, b, what in ((out[1][0], out[0][0], "T"), (out[1][1], out[0][1], "J")):
                bad = np.argwhere(a.view(np.int64) != b.view(np.int64))
                assert len(bad) == 0, "%s frame %d base %s %s: %d words differ, first (row, entry) %r: %r against %r, q = %r" % (
                    name, frame, base is not None, what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])], q[bad[0][0]].tolist())
                assert np.isfinite(a).all()
