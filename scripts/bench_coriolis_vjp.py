#!/usr/bin/env python3
"""The fused adjoint of the Coriolis / centripetal matrix (rtbhip_coriolis_vjp, rtbhip_tree_coriolis_vjp) beside the forward kernel it differentiates
and beside the composition it replaces: DH Panda (7 joints, k_coriolis_vjp<7, MDH>), DH Puma560 (6, k_coriolis_vjp<6, DH>), URDF UR5 (6 link
groups, k_tree_coriolis_vjp<6>) and Kinova Gen3 (13 groups, the run-time-n form k_tree_coriolis_vjp_rt), N = 1e6, float64.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    fwd      the forward coriolis call (rtbhip_coriolis / rtbhip_tree_coriolis), the robot's own instantiation where it has one
    vjp      the fused call with both gradients: reads q, qd and gC, writes gq and gqd -- (n^2 + 4 n) 8 bytes per row
    comp     the composition it replaces, at its most favourable: 2 n launches of rtbhip_rne_vjp / rtbhip_tree_rne_vjp at qd +- e_k with zero
             gravity, qdd NULL and gtau = +-1/4 gC[:, :, k] (the polar identity C[:, k] = 1/4 (tau(qd + e_k) - tau(qd - e_k))), asking for gq and
             gqd, on shifted velocities and contiguous gtau columns built OUTSIDE the timed loop, plus the adds.  It uses only entry points that
             exist unchanged before the fused call did: the earlier library's cost, measured in the same run
Every repetition is a fresh child process under its own time limit; the parent stops at the first child that fails.  `hbm_frac` = the fused call's
byte model / time / 8 TB/s; `vjp_over_fwd` and `comp_over_vjp` are ratios of medians; `vjp_beats_comp` says whether the slowest vjp run is faster
than the fastest comp run (the margin exceeds the spread between the processes).

    python scripts/bench_coriolis_vjp.py [--reps 3] [--out profiles/coriolis_vjp_bench.json]
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
REG_MAX = 7          # the largest joint count with a register form in both kernels (DH: 7, trees: 8; no robot here has 8)
ROBOTS = {"DH.Panda": 7, "DH.Puma560": 6, "UR5": 6, "KinovaGen3": 13}


def make(name):
    import rtbhip
    if name.startswith("DH."):
        return getattr(rtbhip.models.DH, name[3:])(), False
    return rtbhip.urdf.load(name)._tree(()), True


def child():
    import numpy as np
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_coriolis_vjp needs a GPU"
    torch.manual_seed(1)
    out = {}
    zero3 = np.zeros(3)
    for name, n_want in ROBOTS.items():
        rb, tree = make(name)
        n = rb.n
        assert n == n_want, (name, n)
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        qd = 4.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 2.0
        g = 2.0 * torch.rand((N, n, n), dtype=torch.float64, device="cuda") - 1.0
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        handle = rb._handle() if tree else rb._dyn_handle()

        def vjp():
            gq, gqd = torch.empty_like(q), torch.empty_like(q)
            fn = _lib.lib().rtbhip_tree_coriolis_vjp if tree else _lib.lib().rtbhip_coriolis_vjp
            _lib.check(fn(handle, ptr(q), ptr(qd), N, ptr(g), ptr(gq), ptr(gqd), 1, stream()))
            return keep((gq, gqd))

        shifted, cols = [], []
        for k in range(n):
            for sign in (1.0, -1.0):
                v = qd.clone()
                v[:, k] += sign
                shifted.append(v)
                cols.append(((0.25 * sign) * g[:, :, k]).contiguous())

        def comp():
            tq = td = None
            for v, gk in zip(shifted, cols):
                gq, gqd = torch.empty_like(q), torch.empty_like(q)
                if tree:
                    _lib.check(_lib.lib().rtbhip_tree_rne_vjp(handle, ptr(q), ptr(v), None, N, _lib.host_ptr(zero3), ptr(gk), ptr(gq), ptr(gqd), None,
                                                              1, stream()))
                else:
                    _lib.check(_lib.lib().rtbhip_rne_vjp(handle, ptr(q), ptr(v), None, N, _lib.host_ptr(zero3), None, ptr(gk), ptr(gq), ptr(gqd), None,
                                                         1, stream()))
                tq = gq if tq is None else tq.add_(gq)
                td = gqd if td is None else td.add_(gqd)
            return keep((tq, td))

        steps = {"fwd": lambda: keep(rb.coriolis(q, qd)), "vjp": vjp, "comp": comp}
        rb.coriolis(q[:64].contiguous(), qd[:64].contiguous())
        rtbhip.jit.wait(120.0)                   # the forward leg times the robot's own instantiation, not the general kernel that serves meanwhile
        # what is timed is what is tested: the two routes to the gradients agree
        a, b = vjp(), comp()
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 2e-9 * max(1.0, float(y.abs().max()))
        for leg, step in steps.items():
            ring.clear()
            out[name + "." + leg] = benchlib.sustained_ms(step)[0]
        del shifted, cols, g, q, qd
        ring.clear()
        torch.cuda.empty_cache()
    print("BENCH_CORIOLIS_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_coriolis_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_CORIOLIS_VJP ")][-1]
    return json.loads(line[len("BENCH_CORIOLIS_VJP "):])


def code_object_notes():
    """{kernel: notes} of every instantiation of the two adjoint kernels and of their run-time-n forms, from the library's gfx950 code objects"""
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
                key = None
                m = re.search(r"14k_coriolis_vjpILi(\d+)ELb([01])EE", name)
                if m:
                    key = "k_coriolis_vjp<%s, %s>" % (m.group(1), "MDH" if m.group(2) == "1" else "DH")
                m = re.search(r"19k_tree_coriolis_vjpILi(\d+)EE", name)
                if m:
                    key = "k_tree_coriolis_vjp<%s>" % m.group(1)
                m = re.search(r"17k_coriolis_vjp_rtILb([01])EE", name)
                if m:
                    key = "k_coriolis_vjp_rt<%s>" % ("MDH" if m.group(1) == "1" else "DH")
                if "22k_tree_coriolis_vjp_rt" in name:
                    key = "k_tree_coriolis_vjp_rt"
                if key:
                    out[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return dict(sorted(out.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coriolis_vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]} for k, v in sorted(runs.items())}
    res = {"what": "DH Panda (7 joints), DH Puma560 (6), URDF UR5 (6 link groups) and Kinova Gen3 (13 groups, the run-time-n form), N = 1e6, float64, "
                   "sustained ms per step: fwd the forward coriolis call, vjp the fused adjoint (gq and gqd), comp 2 n launches of the inverse-dynamics "
                   "adjoint at qd +- e_k (gq and gqd, shifted velocities and contiguous gtau columns built outside the timed loop) plus the adds",
           "reps": a.reps, "ring": RING, "legs": legs, "byte_model_bytes_per_row": {}, "byte_floor_ms": {}, "hbm_frac": {}, "vjp_over_fwd": {},
           "comp_over_vjp": {}, "vjp_beats_comp": {}, "comp_launches": {}}
    for r, n in ROBOTS.items():
        row_bytes = (n * n + 4 * n) * 8
        res["byte_model_bytes_per_row"][r] = row_bytes
        res["byte_floor_ms"][r] = row_bytes * N / HBM * 1e3
        res["hbm_frac"][r] = row_bytes * N / (legs[r + ".vjp"]["median_ms"] * 1e-3) / HBM
        res["vjp_over_fwd"][r] = legs[r + ".vjp"]["median_ms"] / legs[r + ".fwd"]["median_ms"]
        res["comp_over_vjp"][r] = legs[r + ".comp"]["median_ms"] / legs[r + ".vjp"]["median_ms"]
        res["vjp_beats_comp"][r] = legs[r + ".vjp"]["max_ms"] < legs[r + ".comp"]["min_ms"]
        res["comp_launches"][r] = 2 * n
    res["lds_tile_bytes"] = {r: 64 * ((2 * n + (n * n if n <= REG_MAX else n)) | 1) * 8 for r, n in ROBOTS.items()}      # (trees: plus 24 doubles per branch slot)
    res["code_objects"] = code_object_notes()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("legs", "hbm_frac", "vjp_over_fwd", "comp_over_vjp", "vjp_beats_comp")}, indent=1))


if __name__ == "__main__":
    main()
