"""Every instantiation and both tile sizes of the operational-space kernels, on the CPU replay and on the device: rtbhip_opspace dispatches
k_opspace<NJ, MDH, ALLREV> for NJ = 1..16, both DH conventions, all-revolute or not (64 kernels), rtbhip_tree_opspace k_tree_opspace<NG> for
NG = 1..16.  tests/opspace_cases.py reaches ten of the 80; tests/opspace_census_cases.py names a robot for each, and for the launch classes of the
trees (the first request above 48 KB, the largest request at all, a tile of 32 rows at 16 and at 14 groups).

(a) the census, no GPU: the `case K:` labels and the `default:` branch of the two launchers' switches and kOpsMaxJoints, kOpsRegMax and
    kTreeSlotDoubles are read from the source text; every (n, convention, all-revolute?) and every NG they serve, and every launch class, must be
    named by the table.  ops_layout and ops_tile_rows are restated in Python next to the table and pinned here on nine values; the replay
    library's own ops_layout / ops_tile_rows must give what the restatement gives, for every size.
(b) the CPU replay (tests/emu_opspace, every instantiation): every census case at N = 97 for the masks 63, 7 and 56 against the oracle of
    opspace_cases.formula -- oracle.inertia_dh / erobot_inertia, oracle.rne_dh / erobot_rne, numpy.linalg.inv / pinv / eig -- at
    K eps cond(J)^2 max|ref| per row; err / (eps cond^2 max|ref|) is printed per case, mask and output, and the largest is what
    opspace_census_cases.K_CENSUS_MEASURED records.  The replayed launch shape equals the restatement, every N of SIZES returns the bits of the
    leading rows, and with a compute unit's limit moved from 160 KB to 96 KB the tile seam falls on other robots: other shapes, the same oracle.
(c) the device, through the raw ABI with every input and output in a flush_guard.Guarded buffer, the module under rtbhip.tune("jit", 0): every
    case at N = 97 with mask 63 -- all rows of Mx, Gx and Asada at the bound, Asada exactly 0 below six joints, guard rows intact, inputs
    unchanged, last_launch() equal to the restatement -- and every N of SIZES with the bits of the leading rows of that result (the rows are
    distinct: row independence across the seams of both tile sizes); masks 7 and 56 on one case at least per tail class of each launcher.  One
    case per (tail class x tile size): the six proper subsets of the outputs return the bits of the full call and leave the unasked buffers
    alone; a zeroed, a rank-deficient and a NaN Jacobian at rows 31, 32 and 96 change no other row.
    The tree oracle (a Python loop of n + 1 inverse-dynamics passes) runs on all 97 rows of every tree, once per tree (under a second for the
    16-group trees): no tree is held to the composition instead.

RESULTS.  The replay and the device (MI355X) show the same figures to three digits; the largest err / (eps cond^2 max|ref|) over the 85 robots
and three masks: Mx 30.356 (p10m), Gx 132.189 (r1s, the row where the one joint's gravity torque nearly vanishes; 10.1 without it), Asada 10.459
(p16m, rot).  All 117 device tests pass in 12 s, the whole non-GPU part (133 tests) in 26 s after the replay library's build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtbhip
from rtbhip import _lib
from helpers import replaying
import opspace_cases as zoo
import opspace_census_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robotics-toolbox-python_amd", "csrc")
N = cases.ROWS
OK = 0
# launcher -> (source file, the launch function whose switch dispatches, the switch's operand)
LAUNCHERS = {"dh": ("opspace_kernels.hip", "int launch_opspace(", "d->n"), "tree": ("tree_opspace_kernels.hip", "int launch_tree_opspace(", "t->n")}
CONSTANTS = {"kOpsMaxJoints": "opspace_device.h", "kOpsRegMax": "opspace_device.h", "kOpsOutW": "opspace_device.h", "kTreeSlotDoubles": "tree_device.h"}


# ------------------------------------------------------------------------------------------------ (a) the census (no GPU)
def read_constants(csrc=CSRC):
    out = {}
    for name, fname in CONSTANTS.items():
        found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(csrc, fname)).read())
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    return out


def read_launchers(csrc=CSRC):
    """{launcher: sorted sizes it serves}: the `case K:` labels of its switch, and kOpsMaxJoints for the `default:` branch"""
    limit = read_constants(csrc)["kOpsMaxJoints"]
    out = {}
    for fam, (fname, launch, operand) in LAUNCHERS.items():
        text = open(os.path.join(csrc, fname)).read()
        assert text.count(launch) == 1, (fam, launch)
        body = text[text.index(launch):]
        switches = re.findall(r"switch \(%s\) \{\n(.*?)\n    \}" % re.escape(operand), body, re.S)
        assert len(switches) == 1, (fam, len(switches))
        labels = [int(k) for k in re.findall(r"^\s*case\s+(\d+)\s*:", switches[0], re.M)]
        assert labels and len(set(labels)) == len(labels) and len(re.findall(r"^\s*default\s*:", switches[0], re.M)) == 1, (fam, labels)
        assert limit not in labels, (fam, "the default branch serves kOpsMaxJoints")
        assert "> kOpsMaxJoints" in body[:body.index("switch (")], (fam, "the launcher refuses beyond kOpsMaxJoints")
        out[fam] = sorted(labels + [limit])
    return out


def required(launchers):
    need = {("dh", n, m, r) for n in launchers["dh"] for m in (0, 1) for r in (True, False)} | {("tree", n) for n in launchers["tree"]}
    return need | {("class", text) for text in cases.TREE_CLASSES}


def missing(csrc=CSRC, named=None):
    named = cases.named() if named is None else named
    return sorted((f for f in required(read_launchers(csrc)) if not named.get(f)), key=repr)


def test_every_instantiation_and_launch_class_is_named():
    """a `case` added to a launcher, or a robot taken out of the table, fails here until a robot is named for the form"""
    launchers = read_launchers()
    assert launchers == {"dh": list(range(1, 17)), "tree": list(range(1, 17))}
    k = read_constants()
    assert (k["kOpsMaxJoints"], k["kOpsRegMax"], k["kTreeSlotDoubles"], k["kOpsOutW"]) == (cases.MAX_JOINTS, cases.REG_MAX, cases.SLOT_DOUBLES, cases.OUT_W)
    need = required(launchers)
    assert len([f for f in need if f[0] == "dh"]) == 64 and len([f for f in need if f[0] == "tree"]) == 16
    assert missing() == []
    named = cases.named()
    assert set(named) == need                    # and nothing is filed under a form the launchers do not have
    assert sum(len(v) for v in named.values()) == len(cases.ALL) == 64 + 16 + len(cases.TREE_CLASSES)
    for name in cases.TREES:
        rob = cases.tree_robot(name)[0]
        assert rob._in_group_order(), name
    print("opspace census: %d DH forms, %d tree forms, %d launch classes named by %d robots" % (64, 16, len(cases.TREE_CLASSES), len(cases.ALL)))


@pytest.mark.parametrize("name", ["r1s", "p1m", "r5m", "p6s", "p15s", "r16m", "p16m", "t1", "t9", "t16", "lad8_1", "lad16_3", "lad16_4", "lad14_6"])
def test_the_census_notices_a_missing_robot(name):
    """any one robot out of the table: the census names the form (or the launch class) that is left without one"""
    named = {f: [k for k in v if k != name] for f, v in cases.named().items()}
    gone = missing(named=named)
    if name in cases.DH_ROBOTS:
        n, mdh, allrev = cases.DH_ROBOTS[name]
        assert gone == [("dh", n, mdh, allrev)]
    elif name in cases.LADDERS:
        assert gone == [("class", text) for text, v in cases.TREE_CLASSES.items() if v[0] == name] and len(gone) == 1
    else:
        assert gone == [("tree", cases.RANDOM_TREES[name][2])]


def test_every_robot_of_the_table_is_needed():
    """(the parametrised test above on every robot: each form and each class has exactly one, so taking any one out is noticed)"""
    named = cases.named()
    assert all(len(v) == 1 for v in named.values()) and sorted(k for v in named.values() for k in v) == sorted(cases.ALL)
    for f, (name,) in named.items():
        assert missing(named={g: [k for k in w if k != name] for g, w in named.items()}) == [f]


@pytest.mark.parametrize("fam", sorted(LAUNCHERS))
def test_the_census_notices_a_new_label(tmp_path, fam):
    """a copy of the sources with a `case 17:` in this launcher's switch: the form has no robot"""
    for f in set(CONSTANTS.values()) | {v[0] for v in LAUNCHERS.values()}:
        text = open(os.path.join(CSRC, f)).read()
        if f == LAUNCHERS[fam][0]:
            grow = lambda m: m.group(1) + m.group(1).replace("case 15:", "case 17:").replace("<15>", "<17>").lstrip("\n")
            text, k = re.subn(r"(\n    case 15: [^\n]*\n)", grow, text)
            assert k == 1
        open(str(tmp_path / f), "w").write(text)
    got = missing(str(tmp_path))
    want = [("dh", 17, m, r) for m in (0, 1) for r in (True, False)] if fam == "dh" else [("tree", 17)]
    assert got == sorted(want, key=repr), got


def test_the_restated_layout_is_pinned():
    """per-row doubles, tile and LDS bytes, derived from ops_layout / ops_tile_rows / kTreeSlotDoubles = 18 by hand"""
    pins = [((7, False, True, 0), 71, 64, 36352), ((9, False, True, 0), 109, 64, 55808), ((16, False, True, 0), 249, 64, 127488),
            ((7, False, False, 0), 99, 64, 50688), ((14, False, False, 0), 309, 64, 158208), ((15, False, False, 0), 345, 32, 88320),
            ((16, False, False, 0), 385, 32, 98560), ((16, True, True, 0), 265, 64, 135680),
            # 319 doubles are 163328 bytes at 64 rows, 512 bytes UNDER the 163840 of a compute unit: three slots keep the tile of 64, the halving
            # starts at four (337 doubles: 172544 bytes)
            ((16, True, True, 3), 319, 64, 163328), ((16, True, True, 4), 337, 32, 86272), ((14, True, True, 6), 325, 32, 83200),
            ((14, True, True, 5), 307, 64, 157184), ((8, True, True, 1), 111, 64, 56832), ((16, True, True, 2), 301, 64, 154112),
            ((16, True, True, 14), 517, 32, 132352)]
    for (n, tree, allrev, slots), w, tile, lds in pins:
        got = cases.per_row(n, tree, allrev, slots)
        assert (got, cases.tile_rows(got), cases.tile_rows(got) * got * 8) == (w, tile, lds), (n, tree, allrev, slots, got)
    # the 48 KB threshold (hipFuncSetAttribute): first passed by all-revolute n = 9, general n = 7 and a tree of 8 groups with one slot
    lds = lambda *a: 64 * 8 * cases.per_row(*a)
    assert lds(8, False, True) <= 48 * 1024 < lds(9, False, True) and lds(6, False, False) <= 48 * 1024 < lds(7, False, False)
    assert lds(8, True, True, 0) <= 48 * 1024 < lds(8, True, True, 1) and lds(7, True, True, 1) <= 48 * 1024 < lds(9, True, True, 0)
    # a tile of 32 rows: the general DH forms at 15 and 16 joints; trees from these slot counts on (a tree of n groups has at most n - 2)
    assert [n for n in range(1, 17) for r in (True, False) if cases.tile_rows(cases.per_row(n, False, r)) < 64] == [15, 16]
    first32 = {n: min([k for k in range(0, n - 1) if cases.tile_rows(cases.per_row(n, True, slots=k)) < 64], default=None) for n in range(1, 17)}
    assert {n: k for n, k in first32.items() if k is not None} == {12: 9, 13: 7, 14: 6, 15: 5, 16: 4}
    assert all(cases.tile_rows(cases.per_row(n, True, slots=max(0, n - 2))) >= 32 for n in range(1, 17))          # never below 32: no third tile size
    # every named class is what it is filed as
    for text, (name, w, tile, nbytes) in cases.TREE_CLASSES.items():
        assert cases.launch_shape(name, 1) == (1, 64, nbytes) and cases.row_doubles(name) == w and cases.tile_rows(w) == tile, text
    assert cases.launch_shape("p16s", 97) == (4, 64, 98560) and cases.launch_shape("p14m", 97) == (2, 64, 158208) and cases.launch_shape("lad16_4", 97) == (4, 64, 86272)


# ------------------------------------------------------------------------------------------------ (b) the CPU replay (no GPU)
@pytest.fixture(scope="module")
def emu():
    import opspace_emu_harness as h
    h.lib()
    return h


def test_the_replay_library_has_the_restated_layout(emu):
    lay = np.zeros(5, np.int32)
    for n in range(1, 17):
        for packed, q_in_tile in ((1, 1), (0, 0), (1, 0)):
            emu.lib().emu_opspace_layout(n, packed, q_in_tile, lay.ctypes.data_as(C.c_void_p))
            assert tuple(int(x) for x in lay) == cases.layout(n, bool(packed), bool(q_in_tile)), (n, packed, q_in_tile)
    for w in range(43, 520):
        assert emu.lib().emu_opspace_tile_rows(w) == cases.tile_rows(w), w
    for name in cases.TREES:
        assert emu.nslots(cases.tree_robot(name)[0]) == cases.tree_slots(name), name


def _replay(emu, name, q, J, axes=63, **kw):
    return emu.run(cases.robot(name), cases.is_tree(name), q, J, cases.gravity3(name), axes, **kw)


def _shape_of_replay(emu):
    tiles, tile, w = emu.last_launch()
    return tiles, 64, tile * w * 8


WORST = {}


@pytest.mark.parametrize("name", cases.ALL)
def test_replay_equals_the_oracle(emu, name):
    q, J, draws, replaced = cases.inputs(name)
    ref = cases.reference(name)
    n = q.shape[1]
    print("opspace census case %s (n = %d): %d of %d draws replaced (cond > %g), cond up to %.3g" % (name, n, replaced, draws, cases.COND_MAX, ref["cond"].max()))
    assert 3 * replaced <= draws and ref["cond"].max() <= cases.COND_MAX and q.shape == (N, n) and J.shape == (N, 6, n)
    full = None
    for key, mask in cases.AXES.items():
        got = _replay(emu, name, q, J, axes=mask)
        assert _shape_of_replay(emu) == cases.launch_shape(name, N), (name, emu.last_launch())
        r = cases.ratios(got, ref, key)
        WORST[name] = max(WORST.get(name, 0.0), max(r))
        print("opspace census replay %s/%s (n = %d): err / (eps cond^2 |ref|max) = %s" % (name, key, n, ", ".join("%.3f" % x for x in r)))
        assert cases.within(r, cases.K_CENSUS_BY_OUTPUT), (name, key, r, "the replay exceeds the recorded largest ratios: record the new figure")
        if n < 6:
            assert not got[2].any()
        full = got if mask == 63 else full
    for rows in cases.SIZES:
        part = _replay(emu, name, q[:rows], J[:rows])
        assert _shape_of_replay(emu) == cases.launch_shape(name, rows), (name, rows)
        for a, b in zip(part, full):
            assert a.tobytes() == b[:rows].tobytes(), (name, rows)
    print("opspace census replay %s: largest ratio %.4f" % (name, WORST[name]))


def test_the_census_bound_is_the_projects():
    """8 x the replay's largest ratio; the zoo's own K is as it was"""
    assert cases.K == 8.0 * max(cases.K_CENSUS_MEASURED, zoo.K_MEASURED) and zoo.K == 8.0 * 3.17 and zoo.K_MEASURED == 3.17
    assert cases.K_CENSUS_MEASURED == max(cases.K_CENSUS_BY_OUTPUT) and max(cases.K_OUT) == cases.K and min(cases.K_OUT) >= zoo.K


MOVED = 96 * 1024


# (rows per tile at 160 KB, at 96 KB): 64 -> 32 between the limits, 32 -> 16 beyond both, unchanged below both (r8s) and where 32 rows fit both (lad14_6)
MOVED_TILES = {"p11s": (64, 32), "p12m": (64, 32), "p14m": (64, 32), "p16s": (32, 16), "r16m": (64, 32), "t12": (64, 32), "t16": (64, 32),
               "lad14_6": (32, 32), "lad16_2": (64, 32), "r8s": (64, 64)}


@pytest.mark.parametrize("name", sorted(MOVED_TILES))
def test_a_moved_tile_limit_moves_the_shapes_and_not_the_result(emu, name):
    """ops_tile_rows with 96 KB in place of 160 KB: the robots between the two limits now run tiles of 32 rows -- the asserted launch shape
    changes with the limit, the comparison with the oracle passes as before, and the result has the bits of the 160 KB run: the tile seam is
    exercised, not assumed"""
    q, J, _, _ = cases.inputs(name)
    ref = cases.reference(name)
    here = _replay(emu, name, q, J)
    assert _shape_of_replay(emu) == cases.launch_shape(name, N)
    emu.lib().emu_opspace_set_tile_limit(MOVED)
    try:
        moved = _replay(emu, name, q, J)
        shape = _shape_of_replay(emu)
    finally:
        emu.lib().emu_opspace_set_tile_limit(0)
    assert shape == cases.launch_shape(name, N, MOVED)
    tiles = (cases.tile_rows(cases.row_doubles(name)), cases.tile_rows(cases.row_doubles(name), MOVED))
    assert tiles == MOVED_TILES[name] and (shape != cases.launch_shape(name, N)) == (tiles[0] != tiles[1]), (name, shape, tiles)
    assert cases.within(cases.ratios(moved, ref, "all"), cases.K_CENSUS_BY_OUTPUT)
    for a, b in zip(here, moved):
        assert a.tobytes() == b.tobytes()


# one case per (tail class x tile size) that exists: DH n < 6, n = 6, 7..8, 9..16 at tile 64 and at tile 32; trees the same, tile 32 at 16 and at 14 groups
DEEP = ["p4m", "p6s", "r6m", "p8m", "r7s", "p12m", "r16s", "p15m", "p16s", "t4", "t6", "lad8_1", "t12", "lad16_3", "lad16_4", "lad14_6"]
SUBSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]


def _singular(J):
    """a zeroed Jacobian in the last row of the first 32, a rank-deficient one in the first row of the next 32, a NaN one in the last row of all"""
    J2 = np.array(J)
    J2[31] = 0.0
    J2[32, 2] = J2[32, 1]
    J2[96] = np.nan
    keep = np.ones(N, bool)
    keep[[31, 32, 96]] = False
    return J2, keep


def _check_singular(name, got, full, keep):
    for o, f in zip(got, full):
        assert o[keep].tobytes() == f[keep].tobytes(), name
    assert not np.isfinite(got[0][31]).all() and not np.isfinite(got[0][96]).any() and not np.isfinite(got[1][96]).any()
    assert got[2][32] == 0.0


@pytest.mark.parametrize("name", DEEP)
def test_replay_subsets_and_singular_rows(emu, name):
    q, J, _, _ = cases.inputs(name)
    full = _replay(emu, name, q, J)
    for want in SUBSETS:
        got = _replay(emu, name, q, J, want=want, fill=7.0)
        for o, f, w in zip(got, full, want):
            assert o.tobytes() == f.tobytes() if w else (o == 7.0).all(), (name, want)
    J2, keep = _singular(J)
    _check_singular(name, _replay(emu, name, q, J2), full, keep)


# ------------------------------------------------------------------------------------------------ (c) the device
def _torch():
    return pytest.importorskip("torch")


def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the operational-space kernels run on the device only: not served by the CPU replay")(f))


@pytest.fixture(scope="module")
def jit0():
    """the robots are ad hoc: no case waits for, or leaves behind, a run-time compile"""
    rtbhip.tune("jit", 0)
    yield
    rtbhip.tune("jit", 1)


WIDTHS = (36, 6, 1)


def _raw(torch, name, q, J, axes=63, want=(True, True, True)):
    """one raw call, every input and every output between guard rows: the guards keep their pattern, the inputs their bits, an output that was not
    asked for its pattern everywhere -> ([Mx (n, 6, 6), Gx (n, 6), asada (n,)] with None where not asked for, last_launch())"""
    from flush_guard import Guarded
    tree = cases.is_tree(name)
    rb = cases.robot(name)
    fn, h = ("rtbhip_tree_opspace", rb._handle()) if tree else ("rtbhip_opspace", rb._dyn_handle())
    rows, n = q.shape
    ins = [Guarded(torch, rows, n, "float64").load(torch, q), Guarded(torch, rows, 6 * n, "float64").load(torch, J.reshape(rows, -1))]
    snap = [g.bits.clone() for g in ins]
    outs = [Guarded(torch, rows, w, "float64") for w in WIDTHS]
    g3 = np.ascontiguousarray(cases.gravity3(name), dtype=np.float64)
    rc = getattr(_lib.lib(), fn)(h, ins[0].ptr, ins[1].ptr, rows, _lib.host_ptr(g3), axes, *[o.ptr if w else None for o, w in zip(outs, want)],
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == OK, _lib.lib().rtbhip_last_error()
    launch = _lib.last_launch()
    torch.cuda.synchronize()
    for g, s in zip(ins, snap):
        assert torch.equal(g.bits, s), (name, "an input buffer was written")
    res = []
    for o, w, shape in zip(outs, want, ((rows, 6, 6), (rows, 6), (rows,))):
        assert o.guards_intact(), (name, "a guard row changed")
        if not w:
            assert bool((o.bits == o.pattern).all()), (name, "an output that was not asked for was written")
        res.append(o.live().cpu().numpy().reshape(shape).copy() if w else None)
    return res, launch


# masks 7 and 56: one case at least per tail class of each launcher at each tile size, both conventions (test_the_deep_cases_... holds that)
MASKED = ["p3s", "r5m", "p6s", "r6m", "p7s", "p8m", "r9s", "p12s", "p16m", "p15s", "t4", "t6", "t7", "lad8_1", "t11", "lad16_3", "lad16_4", "lad14_6"]


@gpu
@pytest.mark.parametrize("name", cases.ALL)
def test_every_form_on_the_device(jit0, name):
    torch = _torch()
    q, J, _, _ = cases.inputs(name)
    ref = cases.reference(name)
    n = q.shape[1]
    full = None
    for key, mask in cases.AXES.items():
        if mask != 63 and name not in MASKED:
            continue
        got, launch = _raw(torch, name, q, J, axes=mask)
        assert launch == cases.launch_shape(name, N), (name, launch, cases.launch_shape(name, N))
        r = cases.ratios(got, ref, key)
        print("opspace census device %s/%s (n = %d, launch %r): err / (eps cond^2 |ref|max) = %s" % (name, key, n, launch, ", ".join("%.3f" % x for x in r)))
        assert cases.within(r), (name, key, r)
        if n < 6:
            assert not got[2].any()
        full = got if mask == 63 else full
    for rows in cases.SIZES:
        part, launch = _raw(torch, name, q[:rows], J[:rows])
        assert launch == cases.launch_shape(name, rows), (name, rows, launch)
        for a, b in zip(part, full):
            assert a.tobytes() == b[:rows].tobytes(), (name, rows, "differs from the leading rows of the N = %d result" % N)


def test_the_deep_cases_cover_every_class_and_tile():
    seen = {("tree" if cases.is_tree(k) else "dh", cases.tail_class(cases.robot(k).n), cases.tile_rows(cases.row_doubles(k))) for k in DEEP}
    want = {(f, c, 64) for f in ("dh", "tree") for c in ("n<6", "n=6", "7..8", "9..16")} | {("dh", "9..16", 32), ("tree", "9..16", 32)}
    assert seen == want
    masked = {("tree" if cases.is_tree(k) else "dh", cases.tail_class(cases.robot(k).n), cases.tile_rows(cases.row_doubles(k))) for k in MASKED}
    assert masked == want


@gpu
@pytest.mark.parametrize("name", DEEP)
def test_a_null_output_is_neither_computed_nor_stored(jit0, name):
    torch = _torch()
    q, J, _, _ = cases.inputs(name)
    full, _ = _raw(torch, name, q, J)
    for want in SUBSETS:
        got, launch = _raw(torch, name, q, J, want=want)
        assert launch == cases.launch_shape(name, N)
        for o, f, w in zip(got, full, want):
            assert (o is None) == (not w)
            if w:
                assert o.tobytes() == f.tobytes(), (name, want)


@gpu
@pytest.mark.parametrize("name", DEEP)
def test_a_singular_row_touches_no_other_row(jit0, name):
    torch = _torch()
    q, J, _, _ = cases.inputs(name)
    full, _ = _raw(torch, name, q, J)
    J2, keep = _singular(J)
    _check_singular(name, _raw(torch, name, q, J2)[0], full, keep)
