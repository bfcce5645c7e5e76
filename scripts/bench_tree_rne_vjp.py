#!/usr/bin/env python3
"""The fused adjoint of the link-tree inverse dynamics (rtbhip_tree_rne_vjp) beside the forward kernel it differentiates: UR5 (6 link groups, the
register form k_tree_rne_vjp<6>) and Kinova Gen3 (13 groups, the run-time-n form k_tree_rne_vjp_rt), N = 1e6, float64.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    fwd      rtbhip_tree_rne: the forward kernel the robot is served by (its structure instantiation where it has one), unchanged by the
             adjoint's arrival -- the baseline of the same run
    all      rtbhip_tree_rne_vjp, gq + gqd + gqdd    reads q, qd, qdd, gtau, writes three gradients: 7 n 8 bytes per row
    gq       rtbhip_tree_rne_vjp, gq alone           reads the same four, writes one: 5 n 8 bytes per row
    fd       3 n forward launches back to back: what a one-sided finite-difference gradient of all three inputs costs in forward calls alone
             (forming the perturbed inputs and contracting with gtau is not counted) -- the composition the adjoint replaces
Every repetition is a fresh child process.  `hbm_frac` = the leg's own byte model / time / 8 TB/s.  The lane body computes all three gradients
whichever are asked for -- they share the four sweeps -- so the gq leg saves two stores per element, not arithmetic.
`backward_over_forward` = all / fwd of the same run; `fd_over_all` = fd / all.  The result file also records what the code objects ask for.

    python scripts/bench_tree_rne_vjp.py [--reps 3] [--out profiles/tree_rne_vjp_bench.json]
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
ROBOTS = {"UR5": 6, "KinovaGen3": 13}


def child():
    import numpy as np
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_tree_rne_vjp needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name, n_want in ROBOTS.items():
        rb = rtbhip.urdf.load(name)._tree(())
        n = rb.n
        assert n == n_want, (name, n)
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        qd = 4.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 2.0
        qdd = 4.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 2.0
        g = 2.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 1.0
        gc = np.ascontiguousarray(rb.gravity, dtype=np.float64)
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())

        def vjp(want):
            outs = [torch.empty_like(q) if w else None for w in want]
            _lib.check(_lib.lib().rtbhip_tree_rne_vjp(rb._handle(), ptr(q), ptr(qd), ptr(qdd), N, _lib.host_ptr(gc), ptr(g), ptr(outs[0]), ptr(outs[1]),
                                                      ptr(outs[2]), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return keep(outs)

        def fd():
            for _ in range(3 * n):
                keep(rb.rne(q, qd, qdd))

        steps = {"fwd": lambda: keep(rb.rne(q, qd, qdd)), "all": lambda: vjp((1, 1, 1)), "gq": lambda: vjp((1, 0, 0)), "fd": fd}
        # what is timed is what is tested: gq alone has the all-gradients call's bits, and gqdd is M(q) gtau
        rb.rne(q[:64].contiguous(), qd[:64].contiguous(), qdd[:64].contiguous())
        rtbhip.jit.wait(120.0)                   # the forward leg times the robot's own instantiation, not the general kernel that serves meanwhile
        full = vjp((1, 1, 1))
        assert torch.equal(vjp((1, 0, 0))[0], full[0])
        mg = rb.rne(q[:4096].contiguous(), None, g[:4096].contiguous(), gravity=[0, 0, 0])
        assert float((full[2][:4096] - mg).abs().max()) <= 1e-9 * max(1.0, float(mg.abs().max()))
        for leg, step in steps.items():
            ring.clear()
            out[name + "." + leg] = benchlib.sustained_ms(step)[0]
    print("BENCH_TREE_RNE_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_tree_rne_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_TREE_RNE_VJP ")][-1]
    return json.loads(line[len("BENCH_TREE_RNE_VJP "):])


def code_object_notes():
    """{kernel: notes} of every k_tree_rne_vjp instantiation and of the run-time-n kernel, from the library's gfx950 code objects"""
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
                m = re.search(r"14k_tree_rne_vjpILi(\d)EE", name)
                key = ("k_tree_rne_vjp<%s>" % m.group(1)) if m else ("k_tree_rne_vjp_rt" if "17k_tree_rne_vjp_rt" in name else None)
                if key:
                    out[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return dict(sorted(out.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_rne_vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]} for k, v in sorted(runs.items())}
    res = {"what": "UR5 (6 groups, k_tree_rne_vjp<6>) and Kinova Gen3 (13 groups, k_tree_rne_vjp_rt), N = 1e6, float64, sustained ms per step: fwd "
                   "rtbhip_tree_rne, all rtbhip_tree_rne_vjp with gq + gqd + gqdd, gq rtbhip_tree_rne_vjp with gq alone, fd 3 n forward launches",
           "reps": a.reps, "ring": RING, "legs": legs, "hbm_frac": {}, "backward_over_forward": {}, "fd_forward_launches": {}, "fd_over_all": {}}
    for r, n in ROBOTS.items():
        for leg, row_bytes in (("fwd", 4 * n * 8), ("all", 7 * n * 8), ("gq", 5 * n * 8)):
            res["hbm_frac"][r + "." + leg] = row_bytes * N / (legs[r + "." + leg]["median_ms"] * 1e-3) / HBM
        res["backward_over_forward"][r] = legs[r + ".all"]["median_ms"] / legs[r + ".fwd"]["median_ms"]
        res["fd_over_all"][r] = legs[r + ".fd"]["median_ms"] / legs[r + ".all"]["median_ms"]
        res["fd_forward_launches"][r] = 3 * n
    res["dynamic_lds_bytes"] = {r: 64 * ((4 * n) | 1) * 8 for r, n in ROBOTS.items()}
    res["code_objects"] = code_object_notes()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("legs", "hbm_frac", "backward_over_forward", "fd_over_all")}, indent=1))


if __name__ == "__main__":
    main()
