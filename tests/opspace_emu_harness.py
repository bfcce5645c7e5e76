"""tests/opspace_emu_harness.py -- TEST INFRASTRUCTURE (not a test module), shared by tests/test_opspace_emu.py and tests/test_opspace_census.py:
builds tests/emu_opspace/emu_opspace.cpp -- the lane body and the tile phases of k_opspace / k_tree_opspace on the CPU, every instantiation the
launchers serve -- into tests/emu_opspace/libemu_opspace.so and calls it.

The one source is compiled once per part (-DEMU_OPS_PART=k: the entry points, or the instantiations of a range of sizes), the parts in parallel,
and the objects (build/emu_opspace, git-ignored) are linked into one library.  The library is rebuilt when the digest of its sources, kept next to
it, changes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import emu_harness

ROOT = emu_harness.ROOT
SRC = os.path.join(ROOT, "tests", "emu_opspace", "emu_opspace.cpp")
SO = os.path.join(ROOT, "tests", "emu_opspace", "libemu_opspace.so")
PARTS = 10
_vp, _u64, _i64, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32
_so = None


def lib():
    global _so
    if _so is not None:
        return _so
    base = emu_harness.lib()                     # libemu.so: the registry, tree.cpp (built if stale)
    assert base is not None
    import __graft_entry__ as g
    digest = g.source_digest(emu_harness._deps() + [SRC, os.path.abspath(__file__)])
    stamp = SO + ".stamp"
    if not (os.path.exists(SO) and os.path.exists(stamp) and open(stamp).read().strip() == digest):
        from concurrent.futures import ThreadPoolExecutor
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        emu_dir = os.path.dirname(emu_harness.EMU_SO)
        objdir = os.path.join(ROOT, "build", "emu_opspace")
        os.makedirs(objdir, exist_ok=True)
        flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-fPIC", "-x", "hip", "-w", "-I" + os.path.join(ROOT, "include")]

        def one(part):
            obj = os.path.join(objdir, "emu_opspace_%d.o" % part)
            subprocess.check_call([hipcc] + flags + ["-DEMU_OPS_PART=%d" % part, "-c", SRC, "-o", obj])
            return obj

        with ThreadPoolExecutor(max_workers=min(PARTS, 16, os.cpu_count() or 1)) as ex:
            objs = list(ex.map(one, range(PARTS)))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", SO, "-L" + emu_dir, "-l:libemu.so", "-Wl,-rpath," + emu_dir])
        open(stamp, "w").write(digest)
    from rtbhip._lib import rtbhip_tree_group
    so = C.CDLL(SO)
    so.emu_opspace.argtypes = [_u64, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp]
    so.emu_tree_opspace.argtypes = [C.POINTER(rtbhip_tree_group), _i32, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp]
    so.emu_tree_nslots.argtypes = [C.POINTER(rtbhip_tree_group), _i32]
    so.emu_opspace_layout.argtypes, so.emu_opspace_layout.restype = [_i32, _i32, _i32, _vp], None
    so.emu_opspace_tile_rows.argtypes = [_i32]
    so.emu_opspace_set_tile_limit.argtypes, so.emu_opspace_set_tile_limit.restype = [_i64], None
    so.emu_opspace_last_launch.argtypes, so.emu_opspace_last_launch.restype = [_vp], None
    _so = so
    return so


_handles = {}


def dyn_handle(rb):
    """the replay library's own handle of a DH robot (kept with the robot: the registry is the library's)"""
    if id(rb) not in _handles:
        L = np.ascontiguousarray(rb.L24())
        h = _u64(0)
        assert emu_harness.lib().rtbhip_dyn_create(emu_harness._p(L), rb.n, int(rb.mdh), C.byref(h)) == 0
        _handles[id(rb)] = (h.value, rb)
    return _handles[id(rb)][0]


def groups(rb):
    from rtbhip._lib import rtbhip_tree_group
    recs = rb.group_table()
    arr = (rtbhip_tree_group * len(recs))()
    for k, r in enumerate(recs):
        arr[k].parent, arr[k].kind, arr[k].flip, arr[k].jindex = r["parent"], r["kind"], r["flip"], r["jindex"]
        arr[k].T[:] = list(np.ascontiguousarray(r["T"]).reshape(16))
        arr[k].m = r["m"]
        arr[k].h[:] = list(r["h"])
        arr[k].I[:] = list(r["I"])
    return arr, len(recs)


def nslots(rb):
    """the branch slots csrc/tree.cpp's compiler gives the robot's group table"""
    arr, ng = groups(rb)
    return lib().emu_tree_nslots(arr, ng)


def run(rb, tree, q, J, grav3, axes=63, want=(True, True, True), fill=np.nan, rc=0):
    """-> [Mx (N, 6, 6), Gx (N, 6), asada (N)]; an output not wanted is handed over as NULL and comes back as the untouched buffer"""
    p = emu_harness._p
    q, J = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(J, dtype=np.float64)
    n = q.shape[0]
    out = [np.full((n, 6, 6), fill), np.full((n, 6), fill), np.full((n,), fill)]
    ptrs = [p(o) if w else None for o, w in zip(out, want)]
    g = np.ascontiguousarray(grav3, dtype=np.float64)
    if tree:
        arr, ng = groups(rb)
        got = lib().emu_tree_opspace(arr, ng, p(q), p(J), n, p(g), axes, *ptrs)
    else:
        got = lib().emu_opspace(dyn_handle(rb), p(q), p(J), n, p(g), axes, *ptrs)
    assert got == rc, got
    return out


def last_launch():
    """(workgroups, rows per tile, doubles per row) of the last replayed launch"""
    a = np.zeros(3, np.int64)
    lib().emu_opspace_last_launch(emu_harness._p(a))
    return tuple(int(x) for x in a)
