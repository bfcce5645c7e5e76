"""Shared by tests/test_staged_host_path.py, tests/test_kin_flush_guard_gpu.py and tests/test_flush_guard_all_gpu.py (not a test module): raw-ABI
calls into buffers the test owns.

Out / both_ways: one entry point called on host arrays and on device tensors, every output compared bit for bit.
Guarded: N rows of an input or an output with GUARD rows of a fixed bit pattern in front and behind, as ONE device allocation -- an overrun of up
to a whole tile lands inside the allocation and shows as a changed guard row (compared as raw integers: no NaN equals another by accident)."""
import ctypes as C

import numpy as np
import numpy.testing as nt

from rtbhip import _lib
from rtbhip._lib import lib, check, MEM_HOST, MEM_DEVICE

GUARD = 64
NAN64 = 0x7FF8DEAD0000BEEF
NAN32 = 0x7FC0BEEF
POISON8 = 0xA5          # integer rows have no NaN: a pattern no result of the library takes (success / arrived are 0 or 1)


class Out:
    """An output array of the call: shape and dtype."""

    def __init__(self, *shape, dtype=np.float64):
        self.shape, self.dtype = shape, dtype


def both_ways(fn, make_args):
    """Call `fn` twice -- make_args(ptr, mem, stream) builds the argument tuple, ptr(x) giving the address of input array / Out x in the
    memory kind of that call -- and compare every Out of the host call with the device call's, bit for bit.  -> the host results."""
    import torch
    results = []
    for mem in (MEM_HOST, MEM_DEVICE):
        keep, outs = [], []

        def ptr(x):
            if x is None:
                return None
            if isinstance(x, Out):
                a = np.full(x.shape, 123, dtype=x.dtype)          # never left as allocated: an output the call skips shows
                outs.append(None)
                slot = len(outs) - 1
            else:
                a, slot = np.ascontiguousarray(x), None
            if mem == MEM_HOST:
                keep.append(a)
                if slot is not None:
                    outs[slot] = a
                return a.ctypes.data
            t = torch.from_numpy(a).cuda()
            keep.append(t)
            if slot is not None:
                outs[slot] = t
            return t.data_ptr()
        stream = None if mem == MEM_HOST else _lib.current_stream_ptr()
        check(getattr(lib(), fn)(*make_args(ptr, mem, stream)))
        if mem == MEM_DEVICE:
            torch.cuda.synchronize()
            outs = [t.cpu().numpy() for t in outs]
        results.append(outs)
    assert len(results[0]) == len(results[1]) > 0
    for h, d in zip(*results):
        nt.assert_array_equal(h, d)
        assert not np.all(h == 123)
    return results[0]


class Guarded:
    """N rows of `width` values of `dtype` with GUARD rows of the NaN pattern either side, as one device allocation.
    dtype: "float64" | "float32", and for the integer outputs of IK and p_servo "int32" | "uint8" (a fixed non-result pattern)."""

    def __init__(self, torch, N, width, dtype, device="cuda"):
        self.N, self.w = N, width
        self.itype, self.pattern, self.ftype = {
            "float64": (torch.int64, NAN64, torch.float64), "float32": (torch.int32, NAN32, torch.float32),
            "int32": (torch.int32, NAN32, torch.int32), "uint8": (torch.uint8, POISON8, torch.uint8)}[dtype]
        self.bits = torch.full(((N + 2 * GUARD) * width,), self.pattern, dtype=self.itype, device=device)
        self.ptr = C.c_void_p(self.bits.data_ptr() + GUARD * width * self.bits.element_size())

    def guards_intact(self):
        g = GUARD * self.w
        return bool((self.bits[:g] == self.pattern).all()) and bool((self.bits[g + self.N * self.w:] == self.pattern).all())

    def live_bits(self):
        g = GUARD * self.w
        return self.bits[g:g + self.N * self.w]

    def live(self):
        return self.live_bits().view(self.ftype).reshape(self.N, self.w)

    def load(self, torch, rows):
        """the live rows := `rows` ((N, width), converted to this buffer's dtype): an INPUT between guard rows"""
        t = torch.from_numpy(np.ascontiguousarray(rows)).to(self.ftype).reshape(-1)
        assert t.numel() == self.N * self.w
        self.live_bits().copy_(t.view(self.itype).to(self.bits.device))
        return self
