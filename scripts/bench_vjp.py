#!/usr/bin/env python3
"""The fused vector-Jacobian product of fkine / jacob0 (rtbhip_fkine_jacob_vjp) against the compositions a user had before it: Panda, N = 1e6.

Legs, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of the last
RING calls are kept alive so that every call gets different buffers:
    a     fused, gT only                      reads q 56 + gT 128, writes gq 56 = 240 B per row
    b     fused, gT and gJ                    + gJ 336 = 576 B per row
    c     the composition for (a): fkine_jacob0 (T and J stored), then the contraction in torch
    d     the composition for (b): (c) + hessian0 (2352 B per row written, read again) and an einsum over it
    a32 / b32   the float32 forms of a / b (half the bytes)
Every repetition is a fresh child process.  `hbm_frac` = the leg's byte model / time / 8 TB/s.  The result file also records what the code
objects of the Panda's kernels ask for (VGPRs, scratch, LDS), read from the built library when the ROCm llvm tools are there.

    python scripts/bench_vjp.py [--reps 5] [--out profiles/vjp_bench.json]
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
BYTES = {"a": 240.0, "b": 576.0, "a32": 120.0, "b32": 288.0}


def child():
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_vjp needs a GPU"
    torch.manual_seed(1)
    ets = rtbhip.models.Panda().ets()
    q = 6.0 * torch.rand((N, 7), dtype=torch.float64, device="cuda") - 3.0
    gT = 2.0 * torch.rand((N, 4, 4), dtype=torch.float64, device="cuda") - 1.0
    gJ = 2.0 * torch.rand((N, 6, 7), dtype=torch.float64, device="cuda") - 1.0
    q32, gT32, gJ32 = q.float(), gT.float(), gJ.float()
    ring = []

    def keep(x):
        ring.append(x)
        if len(ring) > RING:
            ring.pop(0)
        return x

    def fused(q, gT, gJ):
        gq = torch.empty_like(q)
        fn = _lib.lib().rtbhip_fkine_jacob_vjp_f32 if q.dtype == torch.float32 else _lib.lib().rtbhip_fkine_jacob_vjp
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        _lib.check(fn(ets._handle(), ptr(q), N, None, None, ptr(gT), ptr(gJ), ptr(gq), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return keep(gq)

    def composed(with_gJ):
        T, J = ets.fkine_jacob0(q)
        w = torch.cat((gT[:, :3, 3], torch.cross(T[:, :3, :3], gT[:, :3, :3], dim=1).sum(2)), dim=1)
        gq = torch.einsum("nrk,nr->nk", J, w)
        if with_gJ:
            gq = gq + torch.einsum("nrc,nkrc->nk", gJ, ets.hessian0(q))
        return keep(gq)

    steps = {"a": lambda: fused(q, gT, None), "b": lambda: fused(q, gT, gJ), "c": lambda: composed(False), "d": lambda: composed(True),
             "a32": lambda: fused(q32, gT32, None), "b32": lambda: fused(q32, gT32, gJ32)}
    # what is timed is what is tested: the fused legs against their compositions, the float32 legs against the rounded fp64 ones
    assert float((fused(q, gT, None) - composed(False)).abs().max()) <= 1e-10 and float((fused(q, gT, gJ) - composed(True)).abs().max()) <= 1e-10
    assert torch.equal(fused(q32, gT32, gJ32), fused(q32.double(), gT32.double(), gJ32.double()).float())
    out = {}
    for leg, step in steps.items():
        ring.clear()
        out[leg] = benchlib.sustained_ms(step)[0]
    print("BENCH_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_VJP ")][-1]
    return json.loads(line[len("BENCH_VJP "):])


def code_object_notes():
    """{kernel: notes} of the Panda's instantiations (NJ = 7) and the run-time-n kernel, from the gfx950 code objects bundled in the library"""
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
                m = re.search(r"9k_kin_vjpILi7ELb([01])ELb([01])E([df])E", name)
                if m or "k_vjp_from_jac_any" in name:
                    key = ("k_kin_vjp<7, gT=%s, gJ=%s, %s>" % (m.group(1), m.group(2), "double" if m.group(3) == "d" else "float")) if m else \
                          ("k_vjp_from_jac_any<%s>" % ("double" if "IdE" in name else "float"))
                    out[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]} for k, v in sorted(runs.items())}
    res = {"what": "Panda, N = 1e6, sustained ms per call: a fused VJP gT only, b fused gT + gJ, c fkine_jacob0 + torch contraction, "
                   "d c + hessian0 + einsum, a32 / b32 float32 forms of a / b",
           "reps": a.reps, "ring": RING, "legs": legs,
           "hbm_frac": {k: BYTES[k] * N / (legs[k]["median_ms"] * 1e-3) / HBM for k in BYTES},
           "c_over_a": legs["c"]["median_ms"] / legs["a"]["median_ms"], "d_over_b": legs["d"]["median_ms"] / legs["b"]["median_ms"],
           "a_faster_than_c_in_every_run": legs["a"]["max_ms"] < legs["c"]["min_ms"], "b_faster_than_d_in_every_run": legs["b"]["max_ms"] < legs["d"]["min_ms"],
           "dynamic_lds_bytes": {"gT only": 64 * 17 * 8, "with gJ (n = 7)": 32 * 43 * 8},
           "code_objects": code_object_notes()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("legs", "hbm_frac", "c_over_a", "d_over_b")}, indent=1))


if __name__ == "__main__":
    main()
