"""The output flush of the register-resident fkine / Jacobian tile (csrc/kin_tile.h: kin_flush, kin_flush_packed, flush_full) writes its rows and
nothing else.

A full round of the tile -- 64 pose rows, 32 Jacobian rows, 16 packed rows -- is written by an unrolled form whose LDS reads run ahead of the
stores; a ragged round (the last tile of a batch) by the rolled loop.  Every output buffer here has 64 guard rows in front and behind, filled with
a fixed NaN bit pattern: after the call the guard rows still hold it (compared as raw integers, so no NaN compares equal to another by accident),
the live rows are bit for bit those of the same call on the general kernel (rtbhip.tune("kin_sig", 0)), and within 1e-10 of the oracle.

N in {1, 31, 32, 33, 63, 64, 65, 96, 127, 129, 200}: the 16-, 32- and 64-row seams of the three round sizes, one row either side of each, and
batches of one, two and four tiles whose last round is full, ragged or empty.  Forms: T+J and packed for frames 0 and 1, T only, J only for
frames 0 and 1; float64 and float32 rows; Panda (ETS model and URDF) and UR5 (the structure-signature instantiations), a 9-joint chain (general
k_kin_reg<9>), a 12-joint chain (the run-time-n tile k_kin), and one small fleet launch.

What is independent here: the guard rows and the oracle.  The general kernel takes the same unrolled flush, so the bit comparison pins the walk, not
the flush; and no test sees the KIND of a store -- that the non-temporal pose path's unrolled stores carry `nt` is read off the code object
(profiles/r08_kin_wave_latency.txt, section 1).  "T" alone runs that path (fkine alone always streams), T+J here the plain one.

float32 rows are the fp64 result rounded once (csrc/kin_tile.h), so their distance from the oracle is bounded by 1e-10 plus half a float32 ulp of
the value: 1e-10 + 2^-24 |x|."""
import ctypes as C

import numpy as np
import pytest

import rtbhip
from rtbhip import urdf, _lib
from helpers import replaying, chain_from_ets, product_ets
from flush_guard import Guarded
from oracle import oracle, chains

# raw device pointers into guarded buffers, and two device kernels compared: not served by the CPU replay of the GPU suite
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(replaying(), reason="raw device pointers into guarded buffers: not served by the CPU replay")]

SIZES = (1, 31, 32, 33, 63, 64, 65, 96, 127, 129, 200)
FORMS = ("T+J f0", "T+J f1", "packed f0", "packed f1", "T", "J f0", "J f1")


def _serial(n, seed):
    """an all-revolute chain of n joints about mixed axes, with a translation and (every other link) a constant rotation between them"""
    rng = np.random.default_rng(seed)
    spec = []
    for j in range(n):
        spec.append((["tx", "ty", "tz"][j % 3], float(rng.uniform(0.05, 0.25))))
        if j % 2:
            spec.append((["Rx", "Ry", "Rz"][(j // 2) % 3], float(rng.uniform(-1.5, 1.5))))
        spec.append((["Rz", "Rx", "Ry"][j % 3], None, False))
    spec.append(("tz", 0.1))
    return product_ets(spec), chains.Chain(spec)


def _panda_ets():
    return rtbhip.models.Panda().ets(), chains.panda_ets()


def _from_urdf(name):
    e = urdf.load(name).ets()
    return e, chain_from_ets(e)


CHAINS = {
    "panda_ets": _panda_ets,
    "panda_urdf": lambda: _from_urdf("Panda"),
    "ur5": lambda: _from_urdf("UR5"),
    "nine": lambda: _serial(9, 9),
    "twelve": lambda: _serial(12, 12),
}
_cache = {}


def _case(name):
    """(ets, float64 q of the largest batch, oracle T, oracle J frame 0, oracle J frame 1), computed once per chain; batch N is its first N rows"""
    if name not in _cache:
        ets, ch = CHAINS[name]()
        q = np.random.default_rng(len(name)).uniform(-np.pi, np.pi, (max(SIZES), ets.n))
        q32 = q.astype(np.float32).astype(np.float64)
        _cache[name] = (ets, {"float64": q, "float32": q32},
                        {d: (oracle.fkine(ch, x), oracle.jacob(ch, x, None, 0), oracle.jacob(ch, x, None, 1)) for d, x in (("float64", q), ("float32", q32))})
    return _cache[name]


@pytest.fixture(autouse=True)
def _knob():
    yield
    rtbhip.tune("kin_sig", 1)


def _launch(torch, ets, q, form, dtype):
    """one raw call of `form` into guarded buffers -> {"T": Guarded, "J": Guarded, "TJ": Guarded} (those the form writes)"""
    N, n = q.shape[0], ets.n
    L, h, qp, stream = _lib.lib(), ets._handle(), C.c_void_p(q.data_ptr()), _lib.current_stream_ptr()
    f32 = dtype == "float32"
    out = {}
    frame = 1 if form.endswith("f1") else 0
    if form.startswith("packed"):
        out["TJ"] = Guarded(torch, N, 16 + 6 * n, dtype)
        fn = L.rtbhip_fkine_jacob_packed_f32 if f32 else L.rtbhip_fkine_jacob_packed
        _lib.check(fn(h, qp, N, None, None, frame, out["TJ"].ptr, _lib.MEM_DEVICE, stream))
    elif form.startswith("T+J"):
        out["T"], out["J"] = Guarded(torch, N, 16, dtype), Guarded(torch, N, 6 * n, dtype)
        fn = L.rtbhip_fkine_jacob_f32 if f32 else L.rtbhip_fkine_jacob
        _lib.check(fn(h, qp, N, None, None, frame, out["T"].ptr, out["J"].ptr, _lib.MEM_DEVICE, stream))
    elif form == "T":
        out["T"] = Guarded(torch, N, 16, dtype)
        if f32:
            _lib.check(L.rtbhip_fkine_jacob_f32(h, qp, N, None, None, 0, out["T"].ptr, None, _lib.MEM_DEVICE, stream))
        else:
            _lib.check(L.rtbhip_fkine(h, qp, N, None, None, out["T"].ptr, _lib.MEM_DEVICE, stream))
    else:
        out["J"] = Guarded(torch, N, 6 * n, dtype)
        if f32:
            _lib.check(L.rtbhip_fkine_jacob_f32(h, qp, N, None, None, frame, None, out["J"].ptr, _lib.MEM_DEVICE, stream))
        else:
            _lib.check(L.rtbhip_jacob(h, qp, N, None, frame, out["J"].ptr, _lib.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    return out


def _against_oracle(got, want, dtype, what):
    got = got.double().cpu().numpy()
    tol = 1e-10 + (2.0 ** -24 * np.abs(want) if dtype == "float32" else 0.0)
    err = np.abs(got - want) - tol
    assert float(err.max()) <= 0.0, (what, float(np.abs(got - want).max()))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_flush_writes_its_rows_and_leaves_the_guard_rows(name, dtype):
    import torch
    ets, qs, refs = _case(name)
    n = ets.n
    T0, J0, J1 = refs[dtype]
    for N in SIZES:
        qh = qs[dtype][:N]
        q = torch.from_numpy(qh.astype(np.float32) if dtype == "float32" else qh).cuda()
        for form in FORMS:
            rtbhip.tune("kin_sig", 1)
            new = _launch(torch, ets, q, form, dtype)
            rtbhip.tune("kin_sig", 0)
            gen = _launch(torch, ets, q, form, dtype)
            rtbhip.tune("kin_sig", 1)
            what = (name, dtype, N, form)
            for k in new:
                assert new[k].guards_intact(), what + (k, "guard rows written")
                assert gen[k].guards_intact(), what + (k, "guard rows written (general kernel)")
                assert torch.equal(new[k].live_bits(), gen[k].live_bits()), what + (k, "bits differ from the general kernel's")
            Jw = (J1 if form.endswith("f1") else J0)[:N].reshape(N, 6 * n)
            if "TJ" in new:
                rows = new["TJ"].live()
                _against_oracle(rows[:, :16], T0[:N].reshape(N, 16), dtype, what + ("T",))
                _against_oracle(rows[:, 16:], Jw, dtype, what + ("J",))
            if "T" in new:
                _against_oracle(new["T"].live(), T0[:N].reshape(N, 16), dtype, what + ("T",))
            if "J" in new:
                _against_oracle(new["J"].live(), Jw, dtype, what + ("J",))


@pytest.mark.parametrize("packed", [False, True])
def test_fleet_launch_leaves_the_guard_rows(packed):
    """one launch over three arms with batches that end on a full tile, one row into a tile and mid-round (k_fleet: the same tile, run-time joint count)"""
    import torch
    from rtbhip import fleet
    names, sizes = ("panda_ets", "ur5", "nine"), (64, 65, 96 + 17)
    ets, qs, bufs = [], [], []
    for nm, N in zip(names, sizes):
        e, q, _ = _case(nm)
        ets.append(e)
        qs.append(torch.from_numpy(q["float64"][:N]).cuda())
        bufs.append([])
    view = lambda g, *shape: g.live_bits().view(torch.float64).reshape(g.N, *shape)
    for knob in (1, 0):                                          # (the fleet kernel takes no signature: the same launch twice)
        rtbhip.tune("kin_sig", knob)
        mine = [(Guarded(torch, N, 16 + 6 * e.n, "float64"),) if packed else (Guarded(torch, N, 16, "float64"), Guarded(torch, N, 6 * e.n, "float64"))
                for e, N in zip(ets, sizes)]
        if packed:
            fleet.fleet_fkine_jacob_packed(ets, qs, out=[view(b[0], b[0].w) for b in mine])
        else:
            fleet.fleet_fkine_jacob(ets, qs, out=([view(b[0], 4, 4) for b in mine], [view(b[1], 6, e.n) for b, e in zip(mine, ets)]))
        torch.cuda.synchronize()
        for i, b in enumerate(mine):
            bufs[i].append(b)
    rtbhip.tune("kin_sig", 1)
    for nm, N, e, (b, b0) in zip(names, sizes, ets, bufs):
        T0, J0, _ = _case(nm)[2]["float64"]
        for g, g0 in zip(b, b0):
            assert g.guards_intact() and g0.guards_intact(), (nm, N, packed, "guard rows written")
            assert torch.equal(g.live_bits(), g0.live_bits()), (nm, N, packed, "bits differ between the two launches")
        if packed:
            rows = b[0].live()
            _against_oracle(rows[:, :16], T0[:N].reshape(N, 16), "float64", (nm, "T"))
            _against_oracle(rows[:, 16:], J0[:N].reshape(N, 6 * e.n), "float64", (nm, "J"))
        else:
            _against_oracle(b[0].live(), T0[:N].reshape(N, 16), "float64", (nm, "T"))
            _against_oracle(b[1].live(), J0[:N].reshape(N, 6 * e.n), "float64", (nm, "J"))
