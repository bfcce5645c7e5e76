#!/usr/bin/env python3
"""The fused adjoint of inverse dynamics (rtbhip_rne_vjp) beside the forward kernel it differentiates: DH Panda and Puma560, N = 1e6.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    fwd      rtbhip_rne: the forward kernel, unchanged by the adjoint's arrival -- the baseline of the same run
    all      rtbhip_rne_vjp, gq + gqd + gqdd         reads q, qd, qdd, gtau, writes three gradients: 7 n 8 bytes per row
    gq       rtbhip_rne_vjp, gq alone                reads the same four, writes one: 5 n 8 bytes per row
    fwd32 / all32 / gq32   the float32 forms (half the bytes)
Every repetition is a fresh child process.  `hbm_frac` = the leg's own byte model / time / 8 TB/s (7 n 8 bytes per row for all three gradients,
5 n 8 for gq alone, 4 n 8 for the forward call; half of each for float32).  The lane body computes all three gradients whichever are asked
for -- they share the four sweeps -- so the gq leg saves two stores per element, not arithmetic.  `fd_forward_launches` = 3 n: what a finite-difference gradient of all three inputs costs in forward launches;
`fd_over_all` = that many forward launches against the one adjoint launch.  The result file also records what the code objects ask for.

    python scripts/bench_rne_vjp.py [--reps 5] [--out profiles/rne_vjp_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "robotics-toolbox-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM = 8.0e12
RING = 3
N = 1000000
ROBOTS = ("panda", "puma560")


def child():
    import numpy as np
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_rne_vjp needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name in ROBOTS:
        rb = rtbhip.models.DH.Panda() if name == "panda" else rtbhip.models.DH.Puma560()
        n = rb.n
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        sign = torch.where(torch.rand((N, n), device="cuda") < 0.5, -1.0, 1.0).double()
        qd = (0.1 + 1.9 * torch.rand((N, n), dtype=torch.float64, device="cuda")) * sign
        qdd = 4.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 2.0
        g = 2.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 1.0
        x64, x32 = (q, qd, qdd, g), tuple(x.float() for x in (q, qd, qdd, g))
        gc = np.ascontiguousarray(rb._gravity_c(None))
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())

        def vjp(x, want):
            outs = [torch.empty_like(x[0]) if w else None for w in want]
            fn = _lib.lib().rtbhip_rne_vjp_f32 if x[0].dtype == torch.float32 else _lib.lib().rtbhip_rne_vjp
            _lib.check(fn(rb._dyn_handle(), ptr(x[0]), ptr(x[1]), ptr(x[2]), N, _lib.host_ptr(gc), None, ptr(x[3]), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), 1,
                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return keep(outs)

        steps = {"fwd": lambda: keep(rb.rne(*x64[:3])), "all": lambda: vjp(x64, (1, 1, 1)), "gq": lambda: vjp(x64, (1, 0, 0)),
                 "fwd32": lambda: keep(rb.rne(*x32[:3])), "all32": lambda: vjp(x32, (1, 1, 1)), "gq32": lambda: vjp(x32, (1, 0, 0))}
        # what is timed is what is tested: gq alone has the all-gradients call's bits, the float32 form is the rounded fp64 one, and gqdd is M(q) gtau
        full = vjp(x64, (1, 1, 1))
        assert torch.equal(vjp(x64, (1, 0, 0))[0], full[0])
        w32 = vjp(tuple(x.double() for x in x32), (1, 1, 1))
        assert all(torch.equal(a, b.float()) for a, b in zip(vjp(x32, (1, 1, 1)), w32))
        mg = rb.rne(q[:4096], None, g[:4096].contiguous(), gravity=[0, 0, 0])
        assert float((full[2][:4096] - mg).abs().max()) <= 1e-9 * max(1.0, float(mg.abs().max()))
        for leg, step in steps.items():
            ring.clear()
            out[name + "." + leg] = benchlib.sustained_ms(step)[0]
    print("BENCH_RNE_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_rne_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_RNE_VJP ")][-1]
    return json.loads(line[len("BENCH_RNE_VJP "):])


def code_object_notes():
    """{kernel: notes} of the two robots' instantiations (Panda: NJ = 7 modified DH; Puma560: NJ = 6 standard DH), from the library's gfx950 code objects"""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "robotics-toolbox-python_amd", "lib", "librtbhip.so")
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(lib)):
        return None
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp, f)], capture_output=True, text=True).stdout
            for e in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", e).group(1)
                m = re.search(r"9k_rne_vjpILi(\d)ELb([01])E([df])E", name)
                if m and (m.group(1), m.group(2)) in (("7", "1"), ("6", "0")):
                    key = "k_rne_vjp<%s, MDH=%s, %s>" % (m.group(1), m.group(2), "double" if m.group(3) == "d" else "float")
                    out[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rne_vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]} for k, v in sorted(runs.items())}
    nj = {"panda": 7, "puma560": 6}
    res = {"what": "DH Panda and Puma560, N = 1e6, sustained ms per launch: fwd rtbhip_rne, all rtbhip_rne_vjp with gq + gqd + gqdd, gq rtbhip_rne_vjp with gq alone; "
                   "*32 the float32 forms", "reps": a.reps, "ring": RING, "legs": legs, "hbm_frac": {}, "backward_over_forward": {}, "fd_forward_launches": {},
           "fd_over_all": {}}
    for r in ROBOTS:
        n = nj[r]
        for leg, row_bytes in (("fwd", 4 * n * 8), ("all", 7 * n * 8), ("gq", 5 * n * 8), ("fwd32", 4 * n * 4), ("all32", 7 * n * 4), ("gq32", 5 * n * 4)):
            res["hbm_frac"][r + "." + leg] = row_bytes * N / (legs[r + "." + leg]["median_ms"] * 1e-3) / HBM
        for s in ("", "32"):
            res["backward_over_forward"][r + s] = legs[r + ".all" + s]["median_ms"] / legs[r + ".fwd" + s]["median_ms"]
            res["fd_over_all"][r + s] = 3 * n * legs[r + ".fwd" + s]["median_ms"] / legs[r + ".all" + s]["median_ms"]
        res["fd_forward_launches"][r] = 3 * n
    res["dynamic_lds_bytes"] = {r: 64 * (4 * nj[r] + 1) * 8 for r in ROBOTS}
    res["code_objects"] = code_object_notes()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("legs", "hbm_frac", "backward_over_forward", "fd_over_all")}, indent=1))


if __name__ == "__main__":
    main()
