"""Every instantiation and every size limit of the six fused adjoint kernel families, on the device: rtbhip_rne_vjp (fp64 and float32),
rtbhip_tree_rne_vjp, rtbhip_inertia_vjp, rtbhip_tree_inertia_vjp, rtbhip_coriolis_vjp, rtbhip_tree_coriolis_vjp.

Each launcher dispatches on the joint or group count: one unrolled register form per `case K:` of its switch, a run-time-n form above that; the DH
families double every form by convention, rne_vjp again by storage type.  The sibling tests draw from a fixed zoo that leaves some of them out;
tests/vjp_census_cases.py names a robot for each of those and for the two size classes of rne_vjp that sit on launch-code thresholds (the tile
passes 48 KB between n = 23 and n = 24; at n = 32 the stride turns even).

(a) the census, no GPU: the launchers' `case` labels and limits are read from the source text and every (family, K[, convention[, storage]]), each
    run-time form at its smallest and largest served size, and rne_vjp at n = 23, 24, 31, 32 must be named by the zoo or by the new table.
(b) the oracle's own error, no GPU: the stencil at h against h / 2 within 1e-10 max(1, |ref|max), a tenth of the bound, on every new case.
(c) the device: every gradient within BOUND = 1e-9 max(1, |ref|max) of the oracle (the project's contract, as the sibling tests use it); gqdd of the
    two rne families also against the exact identity inertia_gqdd; poison-filled outputs of N + 1 rows whose row N keeps the poison; inputs
    unchanged bit for bit; rows 0, 63 and 64 of the 65-row call with the bits of three one-row calls; _lib.last_launch() equal to
    (ceil(N / 64), 64, the LDS bytes of the stride formulas restated below); rne_vjp in float32 bit-equal to the rounded fp64 call.
    The tree Coriolis adjoint at 20 groups has no oracle (38 s per row): it is held to the composition it replaces, 2 n launches of
    rtbhip_tree_rne_vjp, at 2e-9 max(1, |composition|max) on 65 distinct rows -- resting on the tree_rne_vjp case of the same robot passing its
    own oracle here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rtbhip import _lib
from helpers import replaying
import vjp_census_cases as cases
import rne_vjp_cases as dh_cases
import tree_rne_vjp_cases as tree_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robotics-toolbox-python_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "rtbhip.h")
DEV = 1
POISON = -7.25
N = cases.N
FINE = 1e-10          # (b): a tenth of the bound


def _torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ (a) the census (no GPU)
# family -> (source file, the launch function whose switch dispatches, the constant that ends the run-time form's range, DH family?)
LAUNCHERS = {
    "rne_vjp": ("rne_vjp_kernels.hip", "int vjp_launch(", "RTBHIP_MAX_JOINTS", True),
    "inertia_vjp": ("inertia_vjp_kernels.hip", "int launch_inertia_vjp(", "kInertiaVjpMaxJoints", True),
    "coriolis_vjp": ("coriolis_vjp_kernels.hip", "int launch_coriolis_vjp(", "kCoriolisVjpMaxJoints", True),
    "tree_rne_vjp": ("tree_rne_vjp_kernels.hip", "int launch_tree_rne_vjp(", "kTreeVjpMaxGroups", False),
    "tree_inertia_vjp": ("tree_inertia_vjp_kernels.hip", "int launch_tree_inertia_vjp(", "kTreeInertiaVjpMaxGroups", False),
    "tree_coriolis_vjp": ("tree_coriolis_vjp_kernels.hip", "int launch_tree_coriolis_vjp(", "kTreeCoriolisVjpMaxGroups", False),
}
REG_MAX = {"coriolis_vjp": "kCoriolisVjpRegMax", "tree_inertia_vjp": "kTreeInertiaVjpRegMax", "tree_coriolis_vjp": "kTreeCoriolisVjpRegMax"}          # the largest `case`, as a named constant


def read_launchers(csrc=CSRC, header=HEADER):
    """{family: (sorted `case K:` labels of the launcher's switch, largest served size)} from the source text"""
    consts = {"RTBHIP_MAX_JOINTS": int(re.search(r"#define\s+RTBHIP_MAX_JOINTS\s+(\d+)", open(header).read()).group(1))}
    out = {}
    for fam, (fname, launch, limit, _) in LAUNCHERS.items():
        text = open(os.path.join(csrc, fname)).read()
        consts.update({k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", text)})
        assert text.count(launch) == 1, (fam, launch)
        body = text[text.index(launch):]
        switches = re.findall(r"switch \(rt \? 0 : \w+->n\) \{\n(.*?)\n    \}", body, re.S)
        assert len(switches) == 1, (fam, len(switches))
        labels = [int(k) for k in re.findall(r"^\s*case\s+(\d+)\s*:", switches[0], re.M)]
        assert labels and len(set(labels)) == len(labels) and re.search(r"^\s*default\s*:", switches[0], re.M), (fam, labels)
        assert sorted(labels) == list(range(1, max(labels) + 1)), (fam, labels)          # the run-time form starts right above the last label
        if fam in REG_MAX:
            assert consts[REG_MAX[fam]] == max(labels), (fam, labels)
        assert consts[limit] > max(labels), (fam, limit)
        out[fam] = (sorted(labels), consts[limit])
    return out


def required(launchers):
    """{family: the keys (vjp_census_cases.named's) that some robot must carry}: ("reg", K, ...) for every label, ("rt", n, ...) for the run-time
    form at its smallest and its largest served size"""
    need = {}
    for fam, (labels, limit) in launchers.items():
        forms = {("reg", k) for k in labels} | {("rt", max(labels) + 1), ("rt", limit)}
        if fam == "rne_vjp":
            forms |= {("rt", n) for n in (23, 24, 31, 32)}
            need[fam] = {f + (m, s) for f in forms for m in (0, 1) for s in ("f64", "f32")}
        elif LAUNCHERS[fam][3]:
            need[fam] = {f + (m,) for f in forms for m in (0, 1)}
        else:
            need[fam] = forms
    return need


def missing(csrc=CSRC, header=HEADER, named=None):
    named = cases.named() if named is None else named
    return {fam: sorted(want - named[fam]) for fam, want in required(read_launchers(csrc, header)).items() if want - named[fam]}


def test_every_instantiation_and_size_limit_is_named():
    """a `case 9:` added to a launcher, or a robot taken out of the table, fails here until a robot is named for the form"""
    launchers = read_launchers()
    assert set(launchers) == set(LAUNCHERS)
    assert {fam: labels[-1] for fam, (labels, _) in launchers.items()} == cases.FILED_REGISTER_MAX          # the forms the robots were filed under
    assert missing() == {}
    # what the two thresholds of rne_vjp are filed under
    assert [_rne_lds(n) for n in (23, 24, 31, 32)] == [47616, 49664, 64000, 65536] and _rne_lds(23) <= 48 * 1024 < _rne_lds(24)


def test_the_census_notices_a_missing_robot():
    named = cases.named()
    less = {k: set(v) for k, v in named.items()}
    less["inertia_vjp"].discard(("reg", 4, 0))
    less["tree_rne_vjp"].discard(("rt", 24))
    less["rne_vjp"].discard(("rt", 32, 1, "f32"))
    assert missing(named=less) == {"inertia_vjp": [("reg", 4, 0)], "tree_rne_vjp": [("rt", 24)], "rne_vjp": [("rt", 32, 1, "f32")]}


@pytest.mark.parametrize("fam", sorted(LAUNCHERS))
def test_the_census_notices_a_new_label(tmp_path, fam):
    """a copy of the launchers with one more `case` in this family's switch (and, where the last label is a named constant, that constant raised):
    the robots of that size are filed under the run-time form, so the new register form has no robot"""
    last = cases.FILED_REGISTER_MAX[fam]
    for f in os.listdir(CSRC):
        if not f.endswith("_vjp_kernels.hip"):
            continue
        text = open(os.path.join(CSRC, f)).read()
        if f == LAUNCHERS[fam][0]:
            grow = lambda m: m.group(1) + m.group(1).replace("case %d:" % last, "case %d:" % (last + 1)).lstrip("\n")
            text, k = re.subn(r"(\n    case %d: [^\n]*\n)" % last, grow, text)
            assert k == 1
            if fam in REG_MAX:
                text, k = re.subn(r"(constexpr int %s = )%d;" % (REG_MAX[fam], last), r"\g<1>%d;" % (last + 1), text)
                assert k == 1
        open(str(tmp_path / f), "w").write(text)
    got = missing(str(tmp_path))
    assert set(got) == {fam} and {k[:2] for k in got[fam]} == {("reg", last + 1)}, got


# ------------------------------------------------------------------------------------------------ (b) the oracle's own error (no GPU)
def _fine(tag, a, b):
    for what, x, y in zip(("gq", "gqd", "gqdd"), a, b):
        err = float(np.abs(x - y).max()) / max(1.0, float(np.abs(x).max()))
        print("%s %s: stencil at h against h / 2 %.3e (|ref|max %.3g)" % (tag, what, err, np.abs(x).max()))
        assert err <= FINE, (tag, what, err)


@pytest.mark.parametrize("name", cases.RNE_ALL)
def test_oracle_fineness_rne(name):
    _fine("rne_vjp " + name, cases.rne_case(name)[5], cases.rne_case(name, N, cases.H / 2)[5])


@pytest.mark.parametrize("name", cases.TREE_RNE_ALL)
def test_oracle_fineness_tree_rne(name):
    _fine("tree_rne_vjp " + name, cases.tree_rne_case(name)[7], cases.tree_rne_case(name, cases.H / 2)[7])


@pytest.mark.parametrize("name", cases.DH_ALL)
def test_oracle_fineness_inertia(name):
    _fine("inertia_vjp " + name, cases.inertia_dh_case(name)[3:], cases.inertia_dh_case(name, cases.H / 2)[3:])


@pytest.mark.parametrize("name", cases.TREE_INERTIA_ALL)
def test_oracle_fineness_tree_inertia(name):
    _fine("tree_inertia_vjp " + name, cases.inertia_tree_case(name)[4:], cases.inertia_tree_case(name, cases.H / 2)[4:])


@pytest.mark.parametrize("name", cases.DH_ALL)
def test_oracle_fineness_coriolis(name):
    """(gqd is exact -- C is linear in qd -- and does not depend on h: only gq is a stencil)"""
    _fine("coriolis_vjp " + name, cases.coriolis_dh_case(name)[4:], cases.coriolis_dh_case(name, cases.H / 2)[4:])


@pytest.mark.parametrize("name", [k for k in cases.TREE_CORIOLIS_ALL if cases.TREE_CORIOLIS_ROWS[k]])
def test_oracle_fineness_tree_coriolis(name):
    _fine("tree_coriolis_vjp " + name, cases.coriolis_tree_case(name)[5:], cases.coriolis_tree_case(name, cases.H / 2)[5:])


@pytest.mark.parametrize("name", cases.DH_ALL)
def test_the_batched_coriolis_reference_is_the_reference(name):
    """vjp_census_cases.coriolis_dh_batched gathers the reference's inverse-dynamics calls; what it returns has the reference's bits"""
    import coriolis_vjp_cases as cc
    rb = cases.dh_robot(name)
    q, qd, _ = cc.draw(rb.n, 3, 5)
    q, qd = np.array(q), np.array(qd)
    q[1, 0], qd[2] = 0.0, 0.0
    a, b = cases.coriolis_dh_batched(rb)(q, qd), cc.dh_coriolis(rb)(q, qd)
    assert a.shape == b.shape == (3, rb.n, rb.n) and a.tobytes() == b.tobytes() and np.abs(b).max() > 0


def test_the_structured_inputs_hold_what_they_claim():
    for name in cases.STRUCTURED:
        rb, q, qd, qdd, g = cases.rne_inputs(name)
        assert q.shape == (N, rb.n) and len({q[r].tobytes() for r in range(N)}) == N
        k = q[[3, 40, 64]] / cases.HP
        assert np.array_equal(k, np.round(k)) and q[3, 0] == 0.0 and (k == 0).any() and (k != 0).any()
        assert not qd[17].any() and all(qd[r, r % rb.n] == 0.0 for r in range(2, N, 7)) and (qd == 0).sum() == rb.n + len(range(2, N, 7))
        assert all(l.offset == 0.0 and not np.any(l.Tc) for l in rb.links)
    for name in ("planar4s", "wrist6m"):
        assert all(l.B == 0.0 and l.Jm == 0.0 and l.G == 1.0 for l in cases.dh_robot(name).links)
    w = cases.dh_robot("wrist6m").links[4]
    assert w.m == 0.0 and not np.any(w.I) and not np.any(w.r)


# ------------------------------------------------------------------------------------------------ (c) the device
def gpu(f):
    """device kernels on device tensors: not served by the CPU replay of the GPU suite (tests/test_gpu_suite_on_cpu_replay.py)"""
    return pytest.mark.gpu(pytest.mark.skipif(replaying(), reason="the fused adjoints run on the device only: not served by the CPU replay")(f))


# The LDS request of each launcher, restated (csrc/*_vjp_kernels.hip: the *_stride functions and `lds` in the launch functions): 64 lanes, 8 bytes,
# one row per lane; the trees add their branch slots, the register form of the tree Coriolis adjoint 18 doubles per kept group.
def _rne_lds(n):
    return 64 * 8 * (4 * n + 1 if (4 * n + 1) * 64 * 8 <= 65536 else 4 * n)


def _inertia_lds(n):
    return 64 * 8 * ((n + n * (n + 1) // 2) | 1)


def _coriolis_lds(n, reg_max):
    return 64 * 8 * ((2 * n + (n if n > reg_max else n * n)) | 1)


def _slots_kept(rob):
    """(branch slots, kept groups) of a robot's group table, restated from the two places that decide them: compile_tree in csrc/tree.cpp (the loop
    that hands out save_slot / parent_slot and counts `nslots`: one slot per parent that some group other than the next one hangs off) and
    launch_tree_coriolis_vjp in csrc/tree_coriolis_vjp_kernels.hip (`nkept`: the state of group j is kept unless group j + 1 hangs directly off
    it).  A change to either must be made here too: the expected LDS bytes of the three tree families rest on this copy"""
    par = [r["parent"] for r in rob.group_table()]
    n = len(par)
    return len({p for j, p in enumerate(par) if p >= 0 and p != j - 1}), sum(1 for j in range(n) if j + 1 >= n or par[j + 1] != j)


def _tree_rne_lds(rob):
    return 64 * 8 * (((4 * rob.n) | 1) + 18 * _slots_kept(rob)[0])


def _tree_inertia_lds(rob):
    """(the odd stride while the tile fits a CU's 160 KiB; t20 -- 230 doubles a row, five branch slots -- fits at the even stride only: exactly 160 KiB)"""
    row, slots = rob.n + rob.n * (rob.n + 1) // 2, 18 * _slots_kept(rob)[0]
    return 64 * 8 * ((row | 1) + slots) if 64 * 8 * ((row | 1) + slots) <= 160 * 1024 else 64 * 8 * (row + slots)


def _tree_coriolis_lds(rob, reg_max):
    n, (nslots, nkept) = rob.n, _slots_kept(rob)
    reg = 64 * 8 * (((2 * n + n * n) | 1) + 24 * nslots + 18 * nkept)
    return reg if n <= reg_max and reg <= 160 * 1024 else 64 * 8 * (((3 * n) | 1) + 24 * nslots)


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(torch, x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def _call_rne(rb):
    gc = np.ascontiguousarray(rb._gravity_c(None))

    def call(torch, ins, outs, rows):
        fn = _lib.lib().rtbhip_rne_vjp_f32 if ins[0].dtype == torch.float32 else _lib.lib().rtbhip_rne_vjp
        q, qd, qdd, g = ins
        _lib.check(fn(rb._dyn_handle(), _ptr(q), _ptr(qd), _ptr(qdd), rows, _lib.host_ptr(gc), None, _ptr(g), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                      DEV, _stream(torch)))
    return call


def _call_tree_rne(rob, gravity):
    gc = np.ascontiguousarray(gravity, dtype=np.float64)

    def call(torch, ins, outs, rows):
        q, qd, qdd, g = ins
        _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rob._handle(), _ptr(q), _ptr(qd), _ptr(qdd), rows, _lib.host_ptr(gc), _ptr(g), _ptr(outs[0]), _ptr(outs[1]),
                                                  _ptr(outs[2]), DEV, _stream(torch)))
    return call


def _call_inertia(rb, tree):
    fn, h = (_lib.lib().rtbhip_tree_inertia_vjp, rb._handle()) if tree else (_lib.lib().rtbhip_inertia_vjp, rb._dyn_handle())

    def call(torch, ins, outs, rows):
        _lib.check(fn(h, _ptr(ins[0]), rows, _ptr(ins[1]), _ptr(outs[0]), DEV, _stream(torch)))
    return call


def _call_coriolis(rb, tree):
    fn, h = (_lib.lib().rtbhip_tree_coriolis_vjp, rb._handle()) if tree else (_lib.lib().rtbhip_coriolis_vjp, rb._dyn_handle())

    def call(torch, ins, outs, rows):
        _lib.check(fn(h, _ptr(ins[0]), _ptr(ins[1]), rows, _ptr(ins[2]), _ptr(outs[0]), _ptr(outs[1]), DEV, _stream(torch)))
    return call


def _run(torch, tag, call, n, ins, n_out, lds, dtype=None):
    """one call on `ins` (numpy or device arrays of N rows) into n_out poison-filled outputs of N + 1 rows: row N keeps the poison, the inputs keep
    their bits, the launch is (ceil(N / 64), 64, lds), and rows 0, 63, 64 and N - 1 have the bits of one-row calls on those rows.
    -> the n_out outputs' N live rows (device tensors)"""
    dtype = torch.float64 if dtype is None else dtype
    dev = [(x if hasattr(x, "data_ptr") else torch.from_numpy(np.array(x)).cuda()).to(dtype).contiguous() for x in ins]
    rows = int(dev[0].shape[0])
    before = [_bits(torch, x).clone() for x in dev]
    outs = [torch.full((rows + 1, n), POISON, dtype=dtype, device="cuda") for _ in range(n_out)]
    call(torch, dev, outs, rows)
    launch = _lib.last_launch()
    torch.cuda.synchronize()
    print("%s: launch %r" % (tag, launch))
    assert launch == ((rows + 63) // 64, 64, lds), (tag, launch, lds)
    for o in outs:
        assert bool((o[rows] == POISON).all()), (tag, "row N was written")
        assert not bool((o[:rows] == POISON).any()), (tag, "a live value was not written")
    for x, b in zip(dev, before):
        assert torch.equal(_bits(torch, x), b), (tag, "an input changed")
    for r in sorted({0, 63, 64, rows - 1} & set(range(rows))):
        one = [torch.full((2, n), POISON, dtype=dtype, device="cuda") for _ in range(n_out)]
        call(torch, [x[r:r + 1].contiguous() for x in dev], one, 1)
        torch.cuda.synchronize()
        for k, (o, full) in enumerate(zip(one, outs)):
            assert torch.equal(_bits(torch, o[0]), _bits(torch, full[r])) and bool((o[1] == POISON).all()), (tag, "row %d, output %d" % (r, k))
    return [o[:rows] for o in outs]


def _check(tag, names, got, ref, bound=None):
    bound = cases.BOUND if bound is None else bound
    for what, a, b in zip(names, got, ref):
        err = cases.rel_err(a.cpu().numpy(), b)
        print("%s %s: rel err %.3e (|ref|max %.3g)" % (tag, what, err, np.abs(b).max()))
        assert err <= bound, (tag, what, err)


def _f32_rule(torch, tag, rb, ins, lds):
    """f32_call(x32) == fp64_call(x32.double()).float(), bit for bit (tests/test_rne_vjp.py: test_f32_equals_rounded_fp64)"""
    x32 = [torch.from_numpy(np.array(x)).cuda().float() for x in ins]
    got = _run(torch, tag + " f32", _call_rne(rb), rb.n, x32, 3, lds, torch.float32)
    want = _run(torch, tag + " f64 of the f32 inputs", _call_rne(rb), rb.n, [x.double() for x in x32], 3, lds)
    for what, a, b in zip(("gq", "gqd", "gqdd"), got, want):
        assert a.dtype == torch.float32 and torch.equal(_bits(torch, a), _bits(torch, b.float())), (tag, what)
    print("%s: float32 has the bits of the rounded fp64 call" % tag)
    # and the fp64 call on those rounded inputs is within the bound of the oracle on the same inputs, so a float32 instantiation is not named on
    # the strength of agreeing with its fp64 twin alone; float32 itself then sits within one rounding, 2^-24 |value|, of that
    xs = [x.double().cpu().numpy() for x in x32]
    ref = dh_cases.rne_oracle(rb, *xs)
    _check(tag + " f64 of the f32 inputs", ("gq", "gqd", "gqdd"), want, ref)
    _check(tag + " f32", ("gq", "gqd", "gqdd"), got, ref, bound=cases.BOUND + 2.0 ** -24 * (1 + cases.BOUND))


RNE_PARAMS = [(k, N) for k in cases.RNE_ALL] + [(k, rows) for k in cases.RNE_ALL if k[0] == "n" and int(k[1:-1]) in cases.RNE_SIZES
                                                for rows in cases.RNE_SIZES[int(k[1:-1])]]


@gpu
@pytest.mark.parametrize("name,rows", RNE_PARAMS, ids=["%s-N%d" % p for p in RNE_PARAMS])
def test_rne_vjp(name, rows):
    torch = _torch()
    rb, q, qd, qdd, g, ref = cases.rne_case(name, rows)
    lds = _rne_lds(rb.n)
    tag = "rne_vjp %s N=%d" % (name, rows)
    if rb.n in (23, 24, 31, 32):
        print("%s: n = %d asks for %d bytes of LDS" % (tag, rb.n, lds))
    assert (lds > 48 * 1024) == (rb.n >= 24)          # n = 24, 31 and 32 sit beyond the 48 KB threshold, where they were filed
    got = _run(torch, tag, _call_rne(rb), rb.n, (q, qd, qdd, g), 3, lds)
    _check(tag, ("gq", "gqd", "gqdd"), got, ref)
    _check(tag + " identity", ("gqdd",), got[2:], [dh_cases.inertia_gqdd(rb, q, g)])
    _f32_rule(torch, tag, rb, (q, qd, qdd, g), lds)


@gpu
@pytest.mark.parametrize("name", cases.RNE_F32_ZOO)
def test_rne_vjp_float32_on_the_zoo(name):
    """the float32 instantiations of the sizes the sibling zoo covers in fp64 only (it runs float32 on puma560, panda and n9m): the bit rule, and
    the oracle on the rounded inputs (_f32_rule)"""
    torch = _torch()
    rb, q, qd, qdd, g = cases.rne_inputs(name)
    _f32_rule(torch, "rne_vjp %s N=%d" % (name, N), rb, (q, qd, qdd, g), _rne_lds(rb.n))


@gpu
@pytest.mark.parametrize("name", cases.TREE_RNE_ALL)
def test_tree_rne_vjp(name):
    torch = _torch()
    rob, orc, q, qd, qdd, g, gravity, ref = cases.tree_rne_case(name)
    tag = "tree_rne_vjp %s" % name
    got = _run(torch, tag, _call_tree_rne(rob, gravity), rob.n, [cases.tiled(x, N) for x in (q, qd, qdd, g)], 3, _tree_rne_lds(rob))
    _check(tag, ("gq", "gqd", "gqdd"), got, [cases.tiled(r, N) for r in ref])
    _check(tag + " identity", ("gqdd",), got[2:], [cases.tiled(tree_cases.inertia_gqdd(orc, q, g), N)])


@gpu
@pytest.mark.parametrize("name", cases.DH_ALL)
def test_inertia_vjp(name):
    torch = _torch()
    rb, q, g, ref = cases.inertia_dh_case(name)
    tag = "inertia_vjp %s" % name
    got = _run(torch, tag, _call_inertia(rb, False), rb.n, (q, g), 1, _inertia_lds(rb.n))
    _check(tag, ("gq",), got, [ref])


@gpu
@pytest.mark.parametrize("name", cases.TREE_INERTIA_ALL)
def test_tree_inertia_vjp(name):
    torch = _torch()
    rob, orc, q, g, ref = cases.inertia_tree_case(name)
    tag = "tree_inertia_vjp %s" % name
    got = _run(torch, tag, _call_inertia(rob, True), rob.n, [cases.tiled(x, N) for x in (q, g)], 1, _tree_inertia_lds(rob))
    _check(tag, ("gq",), got, [cases.tiled(ref, N)])
    if rob.n == 20:
        # both 20-group trees have five branch slots and take the even stride: 64 * 8 * (230 + 90) bytes, all of a CU's LDS
        assert _slots_kept(rob)[0] == 5 and _tree_inertia_lds(rob) == 160 * 1024


@gpu
def test_tree_inertia_vjp_refuses_a_tree_that_fits_at_neither_stride():
    """20 groups and six branch slots: 230 + 108 doubles per lane even at the even stride, more than a CU's 160 KiB -- refused loudly, nothing
    launched, the output untouched; the inverse-dynamics adjoint serves the same tree"""
    torch = _torch()
    rob, orc = cases.tree_robot("t20w")
    assert rob.n == 20 and _slots_kept(rob)[0] == 6 and 64 * 8 * (230 + 18 * 6) > 160 * 1024
    q, g = cases.inertia_cases.draw(rob.n, 3, 1)
    dq, dg = (torch.from_numpy(np.array(x)).cuda() for x in (q, g))
    out = torch.full((3, rob.n), POISON, dtype=torch.float64, device="cuda")
    rc = _lib.lib().rtbhip_tree_inertia_vjp(rob._handle(), _ptr(dq), 3, _ptr(dg), _ptr(out), DEV, _stream(torch))
    torch.cuda.synchronize()
    assert rc == -3 and _lib.lib().rtbhip_last_error().decode() == "tree_inertia_vjp: tree needs more LDS than a CU has"
    assert bool((out == POISON).all())
    outs = [torch.full((4, rob.n), POISON, dtype=torch.float64, device="cuda") for _ in range(3)]
    qd, qdd, gt = (torch.from_numpy(np.array(x)).cuda() for x in tree_cases.draw(rob.n, 5, rows=3)[1:])
    _call_tree_rne(rob, tree_cases.gravity_of(rob, "plain"))(torch, (dq, qd, qdd, gt), outs, 3)
    assert _lib.last_launch() == (1, 64, _tree_rne_lds(rob)) and all(bool(torch.isfinite(o[:3]).all()) for o in outs)


@gpu
@pytest.mark.parametrize("name", cases.DH_ALL)
def test_coriolis_vjp(name):
    torch = _torch()
    rb, q, qd, g, rq, rd = cases.coriolis_dh_case(name)
    tag = "coriolis_vjp %s" % name
    got = _run(torch, tag, _call_coriolis(rb, False), rb.n, (q, qd, g), 2, _coriolis_lds(rb.n, read_launchers()["coriolis_vjp"][0][-1]))
    _check(tag, ("gq", "gqd"), got, (rq, rd))


def _tree_composition(torch, rob, q, qd, g):
    """tests/test_coriolis_vjp.py: _composition -- 2 n launches of rtbhip_tree_rne_vjp at qd +- e_k, gtau = +-1/4 gC[:, :, k], no gravity, no qdd, summed"""
    zero = np.zeros(3)
    tq, td = torch.zeros_like(q), torch.zeros_like(q)
    for k in range(rob.n):
        for sign in (1.0, -1.0):
            v = qd.clone()
            v[:, k] += sign
            gk = (0.25 * sign) * g[:, :, k].contiguous()
            gq, gqd = torch.empty_like(q), torch.empty_like(q)
            _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rob._handle(), _ptr(q), _ptr(v), None, q.shape[0], _lib.host_ptr(zero), _ptr(gk), _ptr(gq), _ptr(gqd), None,
                                                      DEV, _stream(torch)))
            tq, td = tq + gq, td + gqd
    return [tq, td]


@gpu
@pytest.mark.parametrize("name", cases.TREE_CORIOLIS_ALL)
def test_tree_coriolis_vjp(name):
    torch = _torch()
    tag = "tree_coriolis_vjp %s" % name
    reg_max = read_launchers()["tree_coriolis_vjp"][0][-1]
    if cases.TREE_CORIOLIS_ROWS[name] is None:
        rob, q, qd, g = cases.coriolis_tree_distinct(name)
        assert len({q[r].tobytes() for r in range(N)}) == N
        dev = [torch.from_numpy(np.array(x)).cuda() for x in (q, qd, g)]
        got = _run(torch, tag, _call_coriolis(rob, True), rob.n, dev, 2, _tree_coriolis_lds(rob, reg_max))
        comp = _tree_composition(torch, rob, *dev)
        for what, f, c in zip(("gq", "gqd"), got, comp):
            scale = max(1.0, float(c.abs().max()))
            err = float((f - c).abs().max()) / scale
            print("%s %s: fused against the composition %.3e (|composition|max %.3g)" % (tag, what, err, scale))
            assert bool(torch.isfinite(f).all()) and err <= 2e-9, (tag, what, err)
        return
    rob, orc, q, qd, g, rq, rd = cases.coriolis_tree_case(name)
    got = _run(torch, tag, _call_coriolis(rob, True), rob.n, [cases.tiled(x, N) for x in (q, qd, g)], 2, _tree_coriolis_lds(rob, reg_max))
    _check(tag, ("gq", "gqd"), got, [cases.tiled(r, N) for r in (rq, rd)])
