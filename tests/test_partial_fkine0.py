"""ETS.partial_fkine0 on the device at every launch geometry and order (csrc/partial_kernels.hip: k_partial3 on workgroups that own whole
configurations, k_partial<3..6> on runs of (6, n) blocks that straddle them).  What decides the launch shape is data: how many configurations a
workgroup owns or touches, whether their Jacobians and Hessians are staged in LDS or read from global memory, whether lanes idle, the 24-bit
index arithmetic, the tile assembled in LDS and flushed as one run of 16-byte stores.  None of it exists in the CPU replay (tests/emu calls the
column function once per column with plain indexing), so every shape of tests/partial_cases.py runs here on the device and EVERY entry of EVERY
row is compared with a long-double restatement of the reference's recursion; rtbhip.last_launch() proves each case took the path it is filed
under.  Bit-for-bit properties on top: a row of a batch equals the same row computed alone, the A/B switches return the same bits, nothing but
the N rows is written, host arrays and device tensors agree.

-m "not gpu": the restatement is pinned on the loop oracle and on the reference's own literal, its float64 evaluation bounds what it can resolve
(1e-13, a hundred times below the device bound), the launch geometry restated in Python reaches every path the table claims, and the column
function is replayed on the CPU at order 6 and at 15 / 16 joints.

Observed on an MI355X, first run, all 109 (path, joints, order, batch) cases (deviation relative to max(1, |ref|max); bound 1e-11), worst per path:
    k3_many 8.3e-16 (7 joints, order 3)    k3_one 9.2e-16 (8, 3)          gen3_staged 2.8e-15 (10, 3)
    unstaged 2.1e-15 (15, 4)               many_staged 5.1e-16 (4, 4)     straddle 2.3e-15 (14, 4)
Every bit-for-bit property held (row independence, both A/B switches, poisoned buffers, host against device), and every case's last launch
had the grid and the LDS bytes the restated geometry predicts.  The float64 restatement stays within 5.2e-16 of the long-double one.
"""
import numpy as np
import numpy.testing as nt
import pytest

import rtbhip
from rtbhip import _lib
from oracle import oracle, chains
from helpers import literals, product_ets, replaying, DEV
from test_random_chains import random_spec
import partial_cases as pc

GPU_BOUND = 1e-11          # what tests/test_diff_kinematics.py::test_gpu_partial_fkine0 holds orders 3..5 to
FLOOR_BOUND = 1e-13        # the restatement in float64 against itself in long double: what the reference can resolve
PIN_BOUND = 1e-14          # the restatement against the loop oracle

_ETS = {}


def ets_of(n, order):
    if (n, order) not in _ETS:
        _ETS[(n, order)] = product_ets(pc.problem(n, order)[0])
    return _ETS[(n, order)]


def batch(e, q, order, tool):
    """partial_fkine0 of the rows of q with the batch axis kept (a (1, n) array is ONE configuration to the ETS methods, as in the reference)"""
    out = e.partial_fkine0(q, n=order, tool=tool)
    return out.reshape((len(q),) + tuple(out.shape[-(order + 1):]))


def rel(got, ref):
    """largest deviation relative to max(1, |ref|max); inf when an entry is not finite"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def path_holds(path, n, order, N, g):
    """does the launch `g` (partial_cases.launch) of a case take the path the table files it under?"""
    if path == "k3_many":
        return g["kernel"] == "k_partial3" and g["G"] > 1
    if path == "k3_one":
        return g["kernel"] == "k_partial3" and g["G"] == 1 and g["U"] in (2, 3)
    if g["kernel"] != "k_partial":
        return False
    if path == "gen3_staged":
        return order == 3 and g["stage_cfgs"] > 0 and g["idle"] > 0
    if path == "unstaged":
        return g["stage_cfgs"] == 0
    if path == "many_staged":
        covers = -(-g["perU"] // g["bpc"])
        return g["stage_cfgs"] >= 3 and covers >= 2 and max(g["K"]) <= g["stage_cfgs"] and (N < covers or max(g["K"]) >= covers)
    if path == "straddle":
        return g["stage_cfgs"] > 0 and g["bpc"] % g["perU"] != 0 and max(g["K"]) <= g["stage_cfgs"] and (N < 2 or 2 in g["K"])
    return False


# ---------------------------------------------------------------- -m "not gpu": the reference
@pytest.mark.parametrize("with_tool", [False, True], ids=["notool", "tool"])
@pytest.mark.parametrize("n,order", [(1, 4), (2, 6), (3, 3), (3, 5), (4, 4)])
def test_restatement_is_the_loop_oracle(n, order, with_tool):
    rng = np.random.default_rng(400 + 10 * n + order)
    spec = random_spec(rng, n)
    ch = chains.Chain(spec)
    tool = chains.elementary("ty", 0.2) @ chains.elementary("Rz", -0.6) @ chains.elementary("tx", 0.1) if with_tool else None
    q = rng.uniform(-2.5, 2.5, (2, n))
    got = pc.partial_ref(ch, q, order, tool=tool)
    assert got.dtype == np.longdouble and got.shape == (2,) + (n,) * (order - 1) + (6, n)
    for i in range(2):
        want = oracle.partial_fkine0(ch, q[i], order, tool=tool)
        err = float(np.abs(got[i] - want).max())
        assert err <= PIN_BOUND * max(1.0, float(np.abs(want).max())), err
    if n > 1:
        assert np.abs(got).max() > 1e-3                       # not a comparison of zeros


def test_restatement_is_the_reference_literal():
    """reference tests/test_ETS.py:4259-4263: the (7, 7, 6, 7) literal for the Panda (assert_almost_equal, 7 decimals)"""
    LIT = literals()
    got = pc.partial_ref(chains.panda_ets(), np.array(LIT["panda_q"]), 3)
    nt.assert_almost_equal(np.asarray(got[0], dtype=np.float64), np.array(LIT["K_panda_partial_fkine3"]))


@pytest.mark.parametrize("n,order", pc.SHAPES, ids=["n%d-o%d" % s for s in pc.SHAPES])
def test_rounding_floor_of_the_restatement(n, order):
    """every shape the device tests use: float64 against long double, a hundred times below the device bound -- a case that misses this gets
    other inputs, never another bound"""
    _, ch, tool, q = pc.problem(n, order)
    ref = pc.reference(n, order)
    f64 = pc.partial_ref(ch, q, order, tool=tool, dtype=np.float64)
    err = rel(f64, ref)
    print("floor n=%d order=%d N=%d: %.3g" % (n, order, len(q), err))
    assert err <= FLOOR_BOUND, err


# ---------------------------------------------------------------- -m "not gpu": the geometry
def test_geometry_restated():
    """the restatement itself, on the values the kernels' comments and the launcher give"""
    assert [pc.partial3_geometry(n)[0] for n in range(1, 12)] == [768, 96, 28, 12, 6, 3, 2, 1, 1, 0, 0]
    assert [pc.partial3_geometry(n)[1] for n in (7, 8, 9)] == [3, 2, 3]
    assert [pc.blocks_per_group(n) for n in (1, 2, 3, 4, 7, 10, 13, 16, 24)] == [256, 128, 80, 64, 32, 24, 16, 16, 10]
    # the general kernel stages 2 .. 14 joints at every order; from 15 on, and for one joint (512 configurations per workgroup), nothing
    for order in (3, 4, 5, 6):
        for n in range(2, 17):
            if n ** order < 1 << 24:
                assert (pc.launch(n, order, 1, partial3=False)["stage_cfgs"] > 0) == (n <= 14), (n, order)
        g = pc.launch(1, order, 1, partial3=False)
        assert g["stage_cfgs"] == 0 and g["perU"] // g["bpc"] == 512
    assert pc.launch(2, 4, 1)["stage_cfgs"] == 33 and pc.launch(2, 5, 1)["stage_cfgs"] == 17 and pc.launch(2, 6, 1)["stage_cfgs"] == 9
    assert pc.launch(3, 4, 1)["stage_cfgs"] == 7 and pc.launch(4, 4, 1)["stage_cfgs"] == 3
    # rtbhip_tune("partial3", 0): order 3 of one and two joints on the general kernel -- 512 unstaged / 65 staged configurations
    g1, g2 = pc.launch(1, 3, 1025, partial3=False), pc.launch(2, 3, 193, partial3=False)
    assert g1["kernel"] == g2["kernel"] == "k_partial" and g1["stage_cfgs"] == 0 and g1["perU"] // g1["bpc"] == 512
    assert g2["stage_cfgs"] == 65 and max(g2["K"]) == 64


def test_the_case_table_reaches_the_paths_it_claims():
    """a later retune of the geometry must fail HERE, not quietly move a case to another path"""
    assert set(pc.TABLE) == {"k3_many", "k3_one", "gen3_staged", "unstaged", "many_staged", "straddle"}
    for path, n, order, N in pc.CASES:
        assert path_holds(path, n, order, N, pc.launch(n, order, N)), (path, n, order, N, pc.launch(n, order, N))
        assert N * 48 * n ** order <= 10.5e6, (n, order, N)                     # one output stays around 10 MB
        if order == 3:      # grid and LDS bytes tell the two kernels apart, so last_launch() does prove which one ran
            a, b = pc.launch(n, 3, N), pc.launch(n, 3, N, partial3=False)
            assert a["kernel"] == b["kernel"] or (a["grid"], a["lds"]) != (b["grid"], b["lds"]), (n, N)
    for n, _, Ns in pc.TABLE["k3_many"]:
        G = pc.partial3_geometry(n)[0]
        assert {1, G, G + 1, 2 * G + 1} <= set(Ns) and (G - 1 in Ns or G == 2)      # a lone row, full, ragged, two workgroups and a row
    assert {pc.partial3_geometry(n)[1] for n, _, _ in pc.TABLE["k3_one"]} == {2, 3}
    assert all(256 % n != 0 for n, _, _ in pc.TABLE["gen3_staged"])
    unst = pc.TABLE["unstaged"]
    assert {(n, c) for n, c, _ in unst} >= {(15, 3), (16, 3), (15, 4), (16, 4), (1, 4), (1, 5), (1, 6)}
    for n, c, Ns in unst:
        if n == 1:
            assert Ns == [1, 511, 512, 513, 1025] and pc.launch(1, c, 1025)["grid"] == 3
    for n, c, Ns in pc.TABLE["many_staged"]:
        g = pc.launch(n, c, max(Ns))
        covers = -(-g["perU"] // g["bpc"])
        assert Ns == sorted({max(1, covers - 1), covers, covers + 1, 2 * covers + 1}) and g["grid"] >= 3
    assert {pc.launch(n, c, 1)["stage_cfgs"] for n, c, _ in pc.TABLE["many_staged"]} == {33, 17, 9, 7, 3}
    assert {c for _, c, _ in pc.TABLE["many_staged"]} == {4, 5, 6} == {c for _, c, _ in pc.TABLE["straddle"]}
    # the property cases are cases of the table (one per row of it), at the largest batch of their shape
    for n, c, N in pc.PROPERTY_CASES:
        assert N == max(M for _, m, o, M in pc.CASES if (m, o) == (n, c)), (n, c, N)
    assert {p for p, m, o, _ in pc.CASES if (m, o, ) in {(a, b) for a, b, _ in pc.PROPERTY_CASES}} == set(pc.TABLE)


# ---------------------------------------------------------------- -m "not gpu": the column function replayed on the CPU
@pytest.mark.parametrize("n,order", [(2, 6), (3, 6), (15, 4), (16, 4)])
def test_emu_columns_at_order_6_and_beyond_14_joints(n, order):
    import emu_harness as emu
    rng = np.random.default_rng(900 + 10 * n + order)
    spec = random_spec(rng, n)
    ch, ets = chains.Chain(spec), product_ets(spec)
    tool = chains.elementary("tx", 0.1) @ chains.elementary("Ry", 0.3) if n % 2 else None
    q = rng.uniform(-2.5, 2.5, (2, n))
    got = emu.partial(ets, q, order, tool=tool)
    assert got.shape == (2,) + (n,) * (order - 1) + (6, n)
    want = np.asarray(pc.partial_ref(ch, q, order, tool=tool), dtype=np.float64)
    nt.assert_allclose(got, want, rtol=0, atol=1e-12)
    if n == 2:                                                                # and the loop oracle itself where it is affordable
        nt.assert_allclose(got[1], oracle.partial_fkine0(ch, q[1], order, tool=tool), rtol=0, atol=1e-12)
    assert np.abs(want).max() > 1e-3


# ---------------------------------------------------------------- -m gpu
def check_launch(n, order, N, partial3=True):
    """the call's last launch is the one the restated geometry predicts (the CPU replay launches nothing)"""
    if replaying():
        return
    g = pc.launch(n, order, N, partial3=partial3)
    assert _lib.last_launch() == (g["grid"], pc.BLOCK, g["lds"]), (n, order, N, g, _lib.last_launch())


@pytest.mark.gpu
@pytest.mark.parametrize("path,n,order,N", pc.CASES, ids=pc.CASE_IDS)
def test_gpu_every_entry_of_every_row(path, n, order, N):
    _, _, tool, q = pc.problem(n, order)
    assert path_holds(path, n, order, N, pc.launch(n, order, N))
    got = batch(ets_of(n, order), np.array(q[:N]), order, tool)
    check_launch(n, order, N)
    err = rel(got, pc.reference(n, order)[:N])
    print("partial_fkine0 %s n=%d order=%d N=%d: %.3g" % (path, n, order, N, err))
    assert err <= GPU_BOUND, err


@pytest.mark.gpu
@pytest.mark.parametrize("n,order,N", pc.PROPERTY_CASES, ids=["n%d-o%d-N%d" % c for c in pc.PROPERTY_CASES])
def test_gpu_a_row_of_a_batch_is_the_row_alone(n, order, N):
    """bit for bit: staging offsets, the configurations a workgroup touches, straddling and the tile's assembly all cancel or show"""
    _, _, tool, q = pc.problem(n, order)
    e = ets_of(n, order)
    full = batch(e, np.array(q[:N]), order, tool)
    check_launch(n, order, N)
    assert rel(full, pc.reference(n, order)[:N]) <= GPU_BOUND
    for i in range(N):
        alone = e.partial_fkine0(np.array(q[i]), n=order, tool=tool)
        assert np.array_equal(alone, full[i]), (i, float(np.abs(alone - full[i]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 7, 9])
def test_gpu_order_3_returns_the_same_bits_on_every_path(n):
    """rtbhip_tune("partial3", 0) -- the general kernel at order 3 -- and ("partial3_fused", 0) -- k_partial3 fed a Hessian tensor written by
    a launch of its own -- against the defaults: partial_device.h and partial_kernels.hip claim equal bits for both"""
    _, _, tool, q = pc.problem(n, 3)
    e = ets_of(n, 3)
    Ns = [N for _, m, c, N in pc.CASES if (m, c) == (n, 3)]
    assert len(Ns) >= 2
    try:
        for N in Ns:
            qn = np.array(q[:N])
            rtbhip.tune("partial3", 1); rtbhip.tune("partial3_fused", 1)
            base = batch(e, qn, 3, tool)
            check_launch(n, 3, N)
            assert rel(base, pc.reference(n, 3)[:N]) <= GPU_BOUND
            rtbhip.tune("partial3_fused", 0)
            unfused = batch(e, qn, 3, tool)
            check_launch(n, 3, N)
            rtbhip.tune("partial3_fused", 1); rtbhip.tune("partial3", 0)
            general = batch(e, qn, 3, tool)
            check_launch(n, 3, N, partial3=False)
            assert np.array_equal(unfused, base), ("partial3_fused", n, N, float(np.abs(unfused - base).max()))
            assert np.array_equal(general, base), ("partial3", n, N, float(np.abs(general - base).max()))
    finally:
        rtbhip.tune("partial3", 1)
        rtbhip.tune("partial3_fused", 1)


POISON = -1.2345678e301
POISON_CASES = [(1, 3, 769), (1, 4, 513), (2, 4, 33), (5, 4, 3), (9, 3, 3), (15, 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,order,N", POISON_CASES, ids=["n%d-o%d-N%d" % c for c in POISON_CASES])
def test_gpu_writes_its_rows_and_nothing_else(n, order, N):
    """the raw ABI on a poisoned device buffer of N + 1 configurations: every entry of rows < N is written, row N keeps the poison (the
    comparison alone proves little where the tensor is mostly zeros, as for one joint)"""
    import torch
    from rtbhip._lib import lib, check, MEM_DEVICE
    _, _, tool, q = pc.problem(n, order)
    assert N <= len(q)
    size = 6 * n ** order
    qd = torch.from_numpy(np.array(q[:N])).to(DEV())
    out = torch.full(((N + 1) * size,), POISON, dtype=torch.float64, device=DEV())
    t16 = None if tool is None else np.ascontiguousarray(tool, dtype=np.float64)
    check(lib().rtbhip_partial_fkine0(ets_of(n, order)._handle(), qd.data_ptr(), N, None if t16 is None else t16.ctypes.data, order,
                                      out.data_ptr(), MEM_DEVICE, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    check_launch(n, order, N)
    o = out.cpu().numpy().reshape(N + 1, size)
    assert (o[N] == POISON).all(), int((o[N] != POISON).sum())
    assert not (o[:N] == POISON).any(), int((o[:N] == POISON).sum())
    assert rel(o[:N].reshape((N,) + (n,) * (order - 1) + (6, n)), pc.reference(n, order)[:N]) <= GPU_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("n,order,N", [(11, 3, 5), (15, 4, 3), (3, 3, 57)], ids=["staged", "unstaged", "k_partial3"])
def test_gpu_host_arrays_and_device_tensors_agree(n, order, N):
    import torch
    _, _, tool, q = pc.problem(n, order)
    e = ets_of(n, order)
    host = batch(e, np.array(q[:N]), order, tool)
    dev = batch(e, torch.from_numpy(np.array(q[:N])).cuda(), order, tool)
    assert dev.is_cuda and tuple(dev.shape) == host.shape
    check_launch(n, order, N)
    assert np.array_equal(dev.cpu().numpy(), host)
    assert rel(host, pc.reference(n, order)[:N]) <= GPU_BOUND
