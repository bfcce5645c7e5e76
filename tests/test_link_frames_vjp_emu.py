"""The all-frame adjoint of link_frames on the CPU (no GPU needed): the per-lane body of k_frames_vjp (csrc/frames_vjp_kernels.hip: frames_vjp_lane)
compiled host-side by this test (tests/emu_frames_vjp/emu_frames_vjp.cpp, linked against tests/emu/libemu.so for rtbhip_chain_create and
chain.cpp's lowering of the marks) and held against the oracle of tests/link_frames_vjp_cases.py -- one prefix chain per mark through the compiled
reference -- at the kinematics bound, 1e-10 absolute.  The device runs the same source through another compiler: tests/test_link_frames_vjp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_harness
import link_frames_vjp_cases as cases

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_frames_vjp", "emu_frames_vjp.cpp")
SO = os.path.join(ROOT, "tests", "emu_frames_vjp", "libemu_frames_vjp.so")
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32


@pytest.fixture(scope="module")
def lib():
    base = emu_harness.lib()                     # libemu.so: the chain compiler and registry (built if stale)
    import __graft_entry__ as g
    digest = g.source_digest(emu_harness._deps() + [SRC])
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        emu_dir = os.path.dirname(emu_harness.EMU_SO)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include"),
                               "-shared", SRC, "-o", SO, "-L" + emu_dir, "-l:libemu.so", "-Wl,-rpath," + emu_dir])
        open(stamp, "w").write(digest)
    so = C.CDLL(SO)
    so.emu_frames_vjp.argtypes = [_u64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32]
    assert base is not None
    return so


def _run(lib, ets, marks, base, q, G, force_rt=False):
    p = emu_harness._p
    h = emu_harness.chain_handle(ets)
    q, G = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(G, dtype=np.float64)
    mk = np.ascontiguousarray(marks, dtype=np.int32)
    b = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    out = np.full(q.shape, np.nan)
    assert lib.emu_frames_vjp(h, p(q), q.shape[0], p(b), p(mk), len(mk), p(G), p(out), int(force_rt)) == 0
    return out


def test_the_cases_are_what_they_claim():
    assert cases.ROWS == 24
    assert cases.ets_of("one").n == 1 and cases.ets_of("n12").n == 12 and cases.ets_of("n32").n == 32
    assert len(cases.marks_of("n12")) == len(cases.marks_of("n32")) == 33
    two = [e for e in cases.ets_of("two").joints()]
    assert len(two) == 2 and not two[0].isrotation and two[1].isflip
    cols = cases.ets_of("cols")
    assert list(cols.jindices) == [1, 3] and cols.q_width == 5
    import rtbhip
    panda = rtbhip.models.Panda()
    k, marks = 0, [0]
    for seg in panda._links():
        k += len(seg)
        marks.append(k)
    assert marks == cases.PANDA_MARKS and len(cases.ets_of("panda")) == 22
    assert cases.marks_of("repeat") == [1, 1, 1, 5, 5, 12, 12] and cases.marks_of("zeros") == [0, 0, 0]


@pytest.mark.parametrize("name", cases.EMU_CASES)
def test_lane_body_equals_the_oracle(lib, name):
    ets, marks, base, q, G, ref = cases.case(name)
    got = _run(lib, ets, marks, base, q, G)
    err = float(np.abs(got - ref).max())
    print("link_frames_vjp lane %s (n = %d, %d marks): err %.3e, |ref|max %.3g" % (name, ets.n, len(marks), err, np.abs(ref).max()))
    assert err <= cases.BOUND, (name, err)
    if name == "zeros":
        assert not got.any() and not ref.any()
    else:
        assert np.abs(ref).max() > 1e-3                                      # the comparison is not one of zeros
    if name == "cols":
        assert not got[:, [0, 2, 4]].any() and got[:, [1, 3]].all()          # columns no joint reads: exactly 0


@pytest.mark.parametrize("name", ["one", "two", "rxry", "panda_base", "cols"])
def test_run_time_n_form_agrees(lib, name):
    """the NJ = 0 body (per-joint state in private memory, serves 9..32 joints on the device) on chains the compile-time body also serves"""
    ets, marks, base, q, G, ref = cases.case(name)
    got = _run(lib, ets, marks, base, q, G, force_rt=True)
    assert float(np.abs(got - ref).max()) <= cases.BOUND
    assert np.array_equal(got, _run(lib, ets, marks, base, q, G))


@pytest.mark.parametrize("name", ["panda_base", "rxry", "n12"])
def test_the_bottom_row_of_G_is_never_read(lib, name):
    ets, marks, base, q, G, ref = cases.case(name)
    a = _run(lib, ets, marks, base, q, G)
    G2 = np.array(G)
    G2[:, :, 3, :] = 1e300
    assert np.array_equal(a, _run(lib, ets, marks, base, q, G2))


def test_a_library_linked_without_the_kernel_unit_loads_and_refuses(lib):
    """tests/emu/libemu.so links the product's api.cpp.o with a fixed list of units that does not include frames_vjp_kernels.hip: the launcher is a
    weak reference there, the library loads, and the entry point says what is missing instead of jumping through a null pointer"""
    emu = emu_harness.lib()
    ets, marks, base, q, G, ref = cases.case("one")
    p = emu_harness._p
    h = emu_harness.chain_handle(ets)
    mk = np.ascontiguousarray(marks, dtype=np.int32)
    q, G, out = np.array(q), np.array(G), np.zeros(q.shape)
    proto = C.CFUNCTYPE(C.c_int, _u64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _vp)       # a prototype of this test's own: the shared CDLL object is left as it is
    call = proto(("rtbhip_link_frames_vjp", emu))
    assert call(h, p(q), q.shape[0], None, p(mk), len(mk), p(G), p(out), 0, None) == -1
    assert emu.rtbhip_last_error().decode() == "link_frames_vjp: not built into this library"
    # no frames: zeros, no kernel needed
    out[:] = 7.0
    assert call(h, p(q), q.shape[0], None, None, 0, None, p(out), 0, None) == 0 and not out.any()
