"""k_kin_reg<NJ, WANT_T, WANT_J, PACKED, SIG> (csrc/kin_kernels.hip): fkine / jacob0 / jacobe and their fused and packed forms with the walk of a
known robot written out (built in: Panda as the reference's ETS model, Panda and UR from their URDFs; kin_reg.h: kSig*).

The general k_kin_reg multiplies by every constant segment with the UNFUSED product (kin_device.h: pose_mul_general<false>); a signature
instantiation runs that product's exact specialisation for the segment's zeros and ones (pose_mul_seg_sig -> pose_seg_translate_sum, dotk), so it
must return the general kernel's BITS -- compared here as raw integers, so that a -0 against a +0 or two different NaNs cannot pass as equal.
rtbhip.tune("kin_sig", 0) puts the same call on the general kernel.

Rows: N in {1, 63, 64, 65, 200} -- one lane, the last lane dead, a full tile, one live lane in a second tile, the 32-lane Jacobian round cut
mid-round.  q is drawn from U(-pi, pi); three rows are replaced by the values where zeros and their signs are made: 0, +-pi/2, +-pi, 1e-300 and
a value >= 2^20 (which sends its whole wave through the library sincos), placed so that both the fast and the library branch see the zeros."""
import numpy as np
import pytest

import rtbhip
from rtbhip import urdf
from helpers import replaying

# about the device kernels' bits: the CPU replay of the GPU suite has no second kernel to compare (the host replay of the two walks: tests/test_kin_sig_emu.py)
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(replaying(), reason="compares two device kernels: not served by the CPU replay")]

SIZES = (1, 63, 64, 65, 200)
CHAINS = {
    "panda_ets": lambda: rtbhip.models.Panda().ets(),
    "panda_urdf": lambda: urdf.load("Panda").ets(),
    "ur5": lambda: urdf.load("UR5").ets(),
}
BIG = float(2 ** 20) + 0.5


@pytest.fixture(autouse=True)
def _knob():
    yield
    rtbhip.tune("kin_sig", 1)


def _affine(ax, ang, t):
    c, s = np.cos(ang), np.sin(ang)
    R = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


BASE = _affine("y", 0.3, [0.1, -0.2, 0.4]) @ _affine("z", -1.1, [0.0, 0.05, 0.0])
TOOL = _affine("x", 0.7, [0.02, 0.0, 0.11])


def _q(torch, N, n, dtype, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-np.pi, np.pi, (N, n))
    tiny = 1e-300 if dtype == "float64" else 1e-38          # (1e-300 is 0 in float32: the smallest magnitudes it has instead)
    a = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, tiny, BIG]
    a = a[:n - 1] + [BIG]                                    # every chain gets the value >= 2^20
    b = [tiny, -np.pi, np.pi, -np.pi / 2, np.pi / 2, 0.0, 0.0][:n]
    c = [-np.pi / 2, 0.0, tiny, np.pi, 0.0, np.pi / 2, -np.pi][:n]
    if N >= 3:
        q[N - 1] = a                                         # N = 65: alone in the second tile (library sincos); 63, 64, 200: last tile
        q[N - 2] = b                                         # N = 65: last lane of the first tile, fast branch
    if N >= 200:
        q[5] = c                                             # first tile: fast branch
    elif N >= 3:
        q[0] = c
    t = torch.from_numpy(q)
    return (t.float() if dtype == "float32" else t).cuda()


def _calls(ets, q, base, tool=None):
    out = {}
    for frame in (0, 1):
        T, J = ets.fkine_jacob0(q, base=base, tool=tool, frame=frame)
        out["T+J f%d T" % frame], out["T+J f%d J" % frame] = T, J
        out["packed f%d" % frame] = ets.fkine_jacob0(q, base=base, tool=tool, frame=frame, packed=True)[2]
    out["T only"] = ets.eval(q, base=base, tool=tool)
    out["J only f0"] = ets.jacob0(q, tool=tool)
    out["J only f1"] = ets.jacobe(q, tool=tool)
    return out


def _bits(torch, x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def _ab(torch, ets, q, base, tool=None):
    rtbhip.tune("kin_sig", 1)
    sig = _calls(ets, q, base, tool)
    rtbhip.tune("kin_sig", 0)
    gen = _calls(ets, q, base, tool)
    rtbhip.tune("kin_sig", 1)
    torch.cuda.synchronize()
    return sig, gen


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_signature_kernel_returns_the_general_kernels_bits(name, dtype):
    import torch
    ets = CHAINS[name]()
    want = torch.float64 if dtype == "float64" else torch.float32
    for N in SIZES:
        q = _q(torch, N, ets.n, dtype, 100 + N)
        for base in (None, BASE):
            sig, gen = _ab(torch, ets, q, base)
            for k in sig:
                assert sig[k].dtype == want and sig[k].shape == gen[k].shape, (k, N)
                a, b = _bits(torch, sig[k]), _bits(torch, gen[k])
                if not torch.equal(a, b):
                    bad = (a != b).nonzero()
                    first = tuple(int(v) for v in bad[0])
                    raise AssertionError("%s %s N=%d base=%s %s: %d entries differ, first at %r: %r against %r" % (
                        name, dtype, N, base is not None, k, len(bad), first, sig[k].contiguous()[first].item(), gen[k].contiguous()[first].item()))
                assert bool(torch.isfinite(sig[k]).all()), (k, N)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_a_tool_takes_the_general_kernel(name, dtype):
    """With a tool the host folds it into the tail (chain.cpp: chain_tail) while a signature's last segment is the table's own: the launcher must
    fall back.  A signature kernel launched all the same would walk the table's tail and drop the tool -- so: the knob makes no difference, and
    the tool is in the result."""
    import torch
    ets = CHAINS[name]()
    for N in (65, 200):
        q = _q(torch, N, ets.n, dtype, 7 + N)
        sig, gen = _ab(torch, ets, q, BASE, TOOL)
        for k in sig:
            assert torch.equal(_bits(torch, sig[k]), _bits(torch, gen[k])), (k, N)
        plain = ets.eval(q, base=BASE).double().reshape(N, 4, 4)[:N - 2]
        tooled = sig["T only"].double().reshape(N, 4, 4)[:N - 2]
        want = plain @ torch.from_numpy(TOOL).cuda()
        tol = 1e-12 if dtype == "float64" else 1e-5
        assert float((tooled - want).abs().max()) <= tol
        assert float((tooled - plain).abs().max()) >= 1e-2
