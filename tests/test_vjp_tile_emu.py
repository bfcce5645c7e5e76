"""The tile staging and flush of the adjoint kernels on the CPU (no GPU needed): the phases of csrc/vjp_tile.h -- all that k_rne_vjp, k_tree_rne_vjp
and k_inertia_vjp (and their run-time-n forms) do around their lane bodies, and the flush (B = 2) of k_tree_coriolis_vjp, which keeps a staging
of its own; k_tree_inertia_vjp and k_coriolis_vjp keep all of their own I/O (DESIGN 4.2a has the measurements behind that) -- compiled host-side by this test
(tests/emu_vjp_tile/emu_vjp_tile.cpp), run for lanes 0..63 in a loop with the kernel's barriers as the loop boundaries, and held BIT FOR BIT to a
numpy model of the layout: the phases are moves plus the one addition of the symmetric fold.

LDS row of a sample: A column blocks of n (lds[row * stride + a * n + col]), then the (n x n) block folded onto the packed
triangle (+ j (j + 1) / 2 + i, j >= i), at an odd stride.  Every buffer is pre-filled with NaN and carries NaN guard words: what a phase must not
touch has to come back as it went in.  The inputs have 129 distinct rows, so a row moved by any period shows."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robotics-toolbox-python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emu_vjp_tile", "emu_vjp_tile.cpp")
SO = os.path.join(ROOT, "tests", "emu_vjp_tile", "libemu_vjp_tile.so")
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
ROWS, WAVE, GUARD = 129, 64, 256          # (the guard takes a write that is a row or two out)
NONE, FOLDED = 0, 2
# (N, tile): ncfg = 64, 64, 1, 63
TILES = [(129, 0), (129, 1), (129, 2), (127, 1)]


@pytest.fixture(scope="module")
def lib():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    digest = g.source_digest(sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(ROOT, "include", "rtbhip.h"), SRC])
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include"),
                               "-shared", SRC, "-o", SO])
        open(stamp, "w").write(digest)
    so = C.CDLL(SO)
    so.emu_vjp_tile_stage.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _vp, _vp, _vp]
    so.emu_vjp_tile_flush.argtypes = [_i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _vp, _vp]
    return so


def _ptrs(arrays):
    return (_vp * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _msize(n, mat):
    return {NONE: 0, FOLDED: n * (n + 1) // 2}[mat]


def _inputs(n, A, dtype, seed):
    """129 distinct rows per block, no two elements alike, none a zero"""
    rng = np.random.default_rng(seed)
    cols = [(rng.permutation(ROWS * n).reshape(ROWS, n) + 1 + 1000 * a + rng.uniform(0.1, 0.9, (ROWS, n))).astype(dtype) for a in range(A)]
    gm = rng.permutation(ROWS * n * n).reshape(ROWS, n, n) + 0.5 + rng.uniform(0.01, 0.4, (ROWS, n, n))
    assert all(len(np.unique(c)) == c.size for c in cols) and len(np.unique(gm)) == gm.size
    return cols, gm


def _model_stage(n, A, mat, N, tile, stride, cols, gm):
    """the LDS tile (with its guard words) as the layout has it"""
    cfg0 = tile * WAVE
    ncfg = min(WAVE, N - cfg0)
    lds = np.full(WAVE * stride + GUARD, np.nan)
    rows = lds[:WAVE * stride].reshape(WAVE, stride)
    rows[:, :A * n + _msize(n, mat)] = 0.0                      # rows at and past ncfg, absent inputs: zeros
    for a in range(A):
        if cols[a] is not None:
            rows[:ncfg, a * n:(a + 1) * n] = cols[a][cfg0:cfg0 + ncfg].astype(np.float64)
    g = gm[cfg0:cfg0 + ncfg]
    if mat == FOLDED:
        for j in range(n):
            for i in range(j + 1):
                rows[:ncfg, A * n + j * (j + 1) // 2 + i] = g[:, j, i] + g[:, i, j] if j > i else g[:, i, i]      # the lower element first
    return lds


FORMS = [  # A, dtype, the blocks that are absent
    (1, np.float64, ()), (2, np.float64, ()), (4, np.float64, ()), (4, np.float64, (1, 2)), (4, np.float64, (2,)), (4, np.float32, ()), (4, np.float32, (1,))]


@pytest.mark.parametrize("n", [1, 3, 8, 9])
@pytest.mark.parametrize("A,dtype,absent", FORMS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_staging_puts_every_element_in_its_slot_and_touches_nothing_else(lib, n, A, dtype, absent):
    nj = n if n <= 8 else 0
    cols, gm = _inputs(n, A, dtype, 100 * n + A)
    given = [None if a in absent else c for a, c in enumerate(cols)]
    for opt in ((1,) if absent else (0, 1)):
        for mat in (NONE, FOLDED):
            stride = (A * n + _msize(n, mat)) | 1
            for N, tile in TILES:
                lds = np.full(WAVE * stride + GUARD, np.nan)
                assert lib.emu_vjp_tile_stage(nj, n, A, int(dtype == np.float32), opt, mat, tile, N, stride, _ptrs(given), gm.ctypes.data, lds.ctypes.data) == 0
                want = _model_stage(n, A, mat, N, tile, stride, given, gm)
                bad = np.flatnonzero(_bits(lds) != _bits(want))
                assert bad.size == 0, (n, A, dtype.__name__, absent, opt, mat, N, tile, "first at double %d (row %d, slot %d)" % (bad[0], bad[0] // stride, bad[0] % stride))


def test_the_fold_is_lower_plus_upper_and_the_diagonal_alone(lib):
    """spelled out for one row: slot (j, i) holds exactly gM[j,i] + gM[i,j], the diagonal gM[i,i], and a gM that is zero but for one
    off-diagonal entry lands in the one slot its transpose lands in"""
    n, A = 3, 1
    cols, gm = _inputs(n, A, np.float64, 7)
    stride = (n + 6) | 1
    lds = np.full(WAVE * stride + GUARD, np.nan)
    assert lib.emu_vjp_tile_stage(n, n, A, 0, 0, FOLDED, 0, ROWS, stride, _ptrs(cols), gm.ctypes.data, lds.ctypes.data) == 0
    row = lds[5 * stride:6 * stride]
    assert row[n + 0] == gm[5, 0, 0] and row[n + 2] == gm[5, 1, 1] and row[n + 5] == gm[5, 2, 2]
    assert row[n + 1] == gm[5, 1, 0] + gm[5, 0, 1] and row[n + 3] == gm[5, 2, 0] + gm[5, 0, 2] and row[n + 4] == gm[5, 2, 1] + gm[5, 1, 2]
    one = np.zeros_like(gm)
    one[:, 0, 2] = 0.7
    got = []
    for g in (one, np.ascontiguousarray(one.transpose(0, 2, 1))):
        lds = np.full(WAVE * stride + GUARD, np.nan)
        assert lib.emu_vjp_tile_stage(n, n, A, 0, 0, FOLDED, 0, ROWS, stride, _ptrs(cols), g.ctypes.data, lds.ctypes.data) == 0
        got.append(lds)
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and got[0][5 * stride + n + 3] == 0.7


@pytest.mark.parametrize("n", [1, 3, 8, 9])
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_flush_sends_the_result_slots_out_and_nothing_past_them(lib, n, B, dtype):
    nj = n if n <= 8 else 0
    stride = (B * n + 5) | 1                      # (something behind the result slots, as in every kernel's row)
    rng = np.random.default_rng(10 * n + B)
    lds = rng.permutation(WAVE * stride + GUARD) + rng.uniform(0.1, 0.9, WAVE * stride + GUARD)      # the lane bodies' results: every slot its own value
    rows = lds[:WAVE * stride].reshape(WAVE, stride)
    for opt, missing in [(0, None), (1, None)] + [(1, b) for b in range(B)]:          # each output NULL once where the flag allows it
        for N, tile in TILES:
            cfg0 = tile * WAVE
            ncfg = min(WAVE, N - cfg0)
            outs = [None if b == missing else np.full((ROWS + 2, n), np.nan, dtype) for b in range(B)]      # two guard rows behind the batch
            assert lib.emu_vjp_tile_flush(nj, n, B, int(dtype == np.float32), opt, tile, N, stride, _ptrs(outs), lds.ctypes.data) == 0
            for b in range(B):
                if outs[b] is None:
                    continue              # (a NULL output that was dereferenced would have ended the process)
                want = np.full((ROWS + 2, n), np.nan, dtype)
                want[cfg0:cfg0 + ncfg] = rows[:ncfg, b * n:(b + 1) * n].astype(dtype)      # rounded once, to nearest even
                assert np.array_equal(_bits(outs[b]), _bits(want)), (n, B, dtype.__name__, opt, missing, N, tile, b)


def test_forms_the_replay_was_not_built_with_are_refused(lib):
    z = np.zeros(8)
    assert lib.emu_vjp_tile_stage(2, 2, 1, 0, 0, NONE, 0, 1, 3, _ptrs([z]), None, z.ctypes.data) == -1
    assert lib.emu_vjp_tile_stage(0, 9, 1, 0, 0, 1, 0, 1, 91, _ptrs([z]), None, z.ctypes.data) == -1          # (no plain (n x n) phase exists)
    assert lib.emu_vjp_tile_stage(3, 3, 2, 1, 0, NONE, 0, 1, 7, _ptrs([z, z]), None, z.ctypes.data) == -1
