"""No GPU: the engine of tests/test_flush_guard_all_gpu.py sees what it is there to see.  A stand-in "entry point" (NumPy on the host memory behind
CPU tensors) doubles its input rows; variants of it write one row too many, write into the row in front, skip the last row, touch their input, write
an output that was not asked for, let a row depend on its neighbour or miss the oracle by ten times the bound -- each must fail the check named for it, and the honest one must pass.

Where the oracle is affordable on a few rows only (the tree Coriolis adjoint), a flush that swaps two rows the oracle does not visit -- eight rows
apart, or two: the periods of the cyclic inputs of tests/coriolis_vjp_cases.py, which CANNOT see such a swap -- passes every check above; the second,
all-rows reference of Case (second, tol2) is what fails it, and a result that depends on the batch size fails the leading-rows comparison that
goes with it.  The census of the table is run here too: it reads include/rtbhip.h and needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import test_flush_guard_all_gpu as eng

W = 7          # an odd row width


def _rows(ptr, first, count):
    """`count` rows of W doubles starting `first` rows from the address `ptr` (a c_void_p into a Guarded buffer)"""
    return np.ctypeslib.as_array(C.cast(ptr.value + first * W * 8, C.POINTER(C.c_double)), shape=(count, W))


class _Lib:
    def __init__(self, fault):
        self.fault = fault

    def double_rows(self, x, N, y, z):
        a, out, f = _rows(x, 0, N), _rows(y, 0, N), self.fault
        out[:] = 2.0 * a
        if f == "one row too many":
            _rows(y, N, 1)[:] = 1.0
        elif f == "the row in front":
            _rows(y, -1, 1)[:, W - 1] = 1.0
        elif f == "last row skipped":
            out[N - 1] = np.nan
        elif f == "input written":
            a[0, 0] += 1.0
        elif f == "unasked output written":
            _rows(z, 0, 1)[:] = 0.0
        elif f == "row depends on its neighbour" and N > 1:
            out[N - 1, 0] += 1e-13 * a[N - 2, 0]
        elif f == "one entry off by 1e-9":
            out[:, 3] += 1e-9
        elif f in SWAPS and N > SWAP_ROW + SWAPS[f]:
            r, o = SWAP_ROW, SWAP_ROW + SWAPS[f]
            out[[r, o]] = out[[o, r]]
        elif f == "row depends on the batch size" and N == 47:
            out[SWAP_ROW, 0] += 1e-13
        return 0


SWAPS = {"rows r and r + 8 swapped": 8, "rows r and r + 2 swapped": 2}
SWAP_ROW = 34          # 34, 36 and 42: no seam row (none is computed alone) and no oracle row


def _sparse_case(with_second):
    """y = 2 x with the oracle on ORACLE_ROWS_24 only, as the tree Coriolis rows of the table have it; the second reference is 2 x on every row"""
    x = np.random.default_rng(6).uniform(-1, 1, (eng.NMAX, W))
    rows = eng.ORACLE_ROWS_24
    assert not {SWAP_ROW, SWAP_ROW + 2, SWAP_ROW + 8} & (set(rows.tolist()) | set(eng.SEAM_ROWS.tolist()))
    return eng.Case("double_rows", {"x": eng.In(x)}, [eng.O("y", W), eng.O("z", W)], lambda N, p, s: (p("x"), N, p("y"), p.address_of("z")),
                    ref={"y": eng._sparse(rows, 2.0 * x[rows])}, rows=rows, tol=lambda name, w, rows: 1e-10,
                    second=(lambda: {"y": 2.0 * x}) if with_second else None, tol2=(lambda name, w: 2e-10) if with_second else None)


def _case():
    """y = 2 x; z is an output nobody asks for: the stand-in gets its address through p.address_of, which does not count as asking"""
    x = np.random.default_rng(5).uniform(-1, 1, (eng.NMAX, W))
    return eng.Case("double_rows", {"x": eng.In(x)}, [eng.O("y", W), eng.O("z", W)], lambda N, p, s: (p("x"), N, p("y"), p.address_of("z")),
                    ref={"y": 2.0 * x}, tol=lambda name, w, rows: 1e-10)


def _stand_in(monkeypatch, fault):
    import torch
    monkeypatch.setattr(eng, "DEV", lambda: "cpu")
    monkeypatch.setattr(eng._lib, "lib", lambda: _Lib(fault))
    monkeypatch.setattr(eng._lib, "check", lambda rc: None)
    monkeypatch.setattr(eng._lib, "current_stream_ptr", lambda: None)
    monkeypatch.setattr(eng._lib, "last_launch", lambda: (0, 0, 0))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)


@pytest.mark.parametrize("fault,message", [
    (None, None), ("one row too many", "guard rows written"), ("the row in front", "guard rows written"), ("last row skipped", "not finite"),
    ("input written", "an input buffer was written"), ("unasked output written", "not asked for"),
    ("row depends on its neighbour", "computed alone"), ("one entry off by 1e-9", "max deviation")])
def test_the_engine_sees_each_kind_of_wrong_flush(monkeypatch, fault, message):
    _stand_in(monkeypatch, fault)
    run = lambda: eng._run_row("stand-in", "double_rows", {}, _case)
    if fault is None:
        run()
        return
    with pytest.raises(AssertionError) as info:
        run()
    assert message in str(info.value), str(info.value)


@pytest.mark.parametrize("fault,message", [
    (None, None), ("rows r and r + 8 swapped", "second reference: max deviation"), ("rows r and r + 2 swapped", "second reference: max deviation"),
    ("row depends on the batch size", "differs from the leading rows")])
def test_a_row_swap_between_oracle_rows_fails_the_second_reference(monkeypatch, fault, message):
    """the oracle on a few rows, every row against the second reference: a swap of two rows the oracle does not visit is seen by the second
    reference ALONE -- the same case without it passes, which is the gap the hook closes"""
    _stand_in(monkeypatch, fault)
    if fault is None:
        eng._run_row("stand-in", "double_rows", {}, lambda: _sparse_case(True))
        return
    eng._run_row("stand-in", "double_rows", {}, lambda: _sparse_case(False))          # nothing else sees it
    with pytest.raises(AssertionError) as info:
        eng._run_row("stand-in", "double_rows", {}, lambda: _sparse_case(True))
    assert message in str(info.value), str(info.value)


def test_the_census_reads_the_header():
    """every `int rtbhip_*(..., int32_t mem, void *stream)` and every `int rtbhip_*(... int64_t N ..., void *stream)` of include/rtbhip.h has a row in the table or is guard-checked elsewhere, whatever type
    rtbhip/_lib.py gives its stream argument; a declaration the table does not know fails it"""
    eng.test_every_compute_entry_point_is_in_the_table_or_guard_checked_elsewhere()
    declared = eng.header_census()
    assert {"rtbhip_inertia_vjp", "rtbhip_tree_inertia_vjp", "rtbhip_coriolis_vjp", "rtbhip_tree_coriolis_vjp", "rtbhip_p_servo", "rtbhip_ik_qp"} <= declared
    assert not declared & {"rtbhip_device_copy", "rtbhip_ik_restart", "rtbhip_tree_create", "rtbhip_last_launch", "rtbhip_stream_probe"}
    assert not eng.types_census() >= declared          # the types rule alone misses the four (rtbhip/_lib.py: _si, _sc)
    # the three entry points that take device pointers only (no mem argument) are declared compute entry points too, and only they are added
    assert eng.MEMLESS == {"rtbhip_ik_vjp", "rtbhip_opspace", "rtbhip_tree_opspace"} <= declared
    assert eng.header_census(mem_only=True) == declared - eng.MEMLESS and len(eng.header_census(mem_only=True)) == len(declared) - 3
