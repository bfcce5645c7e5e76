"""No GPU: the engine of tests/test_flush_guard_all_gpu.py sees what it is there to see.  A stand-in "entry point" (NumPy on the host memory behind
CPU tensors) doubles its input rows; variants of it write one row too many, write into the row in front, skip the last row, touch their input, write
an output that was not asked for, let a row depend on its neighbour or miss the oracle by ten times the bound -- each must fail the check named for it, and the honest one must pass."""
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
        return 0


def _case():
    """y = 2 x; z is an output nobody asks for: the stand-in gets its address through p.address_of, which does not count as asking"""
    x = np.random.default_rng(5).uniform(-1, 1, (eng.NMAX, W))
    return eng.Case("double_rows", {"x": eng.In(x)}, [eng.O("y", W), eng.O("z", W)], lambda N, p, s: (p("x"), N, p("y"), p.address_of("z")),
                    ref={"y": 2.0 * x}, tol=lambda name, w, rows: 1e-10)


@pytest.mark.parametrize("fault,message", [
    (None, None), ("one row too many", "guard rows written"), ("the row in front", "guard rows written"), ("last row skipped", "not finite"),
    ("input written", "an input buffer was written"), ("unasked output written", "not asked for"),
    ("row depends on its neighbour", "computed alone"), ("one entry off by 1e-9", "max deviation")])
def test_the_engine_sees_each_kind_of_wrong_flush(monkeypatch, fault, message):
    import torch
    monkeypatch.setattr(eng, "DEV", lambda: "cpu")
    monkeypatch.setattr(eng._lib, "lib", lambda: _Lib(fault))
    monkeypatch.setattr(eng._lib, "check", lambda rc: None)
    monkeypatch.setattr(eng._lib, "current_stream_ptr", lambda: None)
    monkeypatch.setattr(eng._lib, "last_launch", lambda: (0, 0, 0))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    run = lambda: eng._run_row("stand-in", "double_rows", {}, _case)
    if fault is None:
        run()
        return
    with pytest.raises(AssertionError) as info:
        run()
    assert message in str(info.value), str(info.value)
