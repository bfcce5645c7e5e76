#!/usr/bin/env python3
"""The fused all-frame adjoint of fkine_all (rtbhip_link_frames_vjp) beside the forward launch it differentiates and beside the composition it
replaces: Panda (22 transforms) and the URDF UR5 with the marks of their fkine_all, N = 1e6, float64.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    fwd      rtbhip_link_frames: the forward launch, unchanged by the adjoint's arrival -- the baseline of the same run
    bwd      rtbhip_link_frames_vjp: reads q and G (N, nmarks, 4, 4), writes gq: (128 nmarks + 16 q_width) bytes per row
    prefix   what a user had before: one differentiable fkine of a prefix chain per frame with joints -- forward AND backward of the whole loop
             (torch.autograd.backward on the frames with G's slices as their gradients: no arithmetic of the loss is timed)
Every repetition is a fresh child process.  `hbm_frac` = the leg's own byte model / time / 8 TB/s.  `prefix_over_bwd` is the bar: the fused
backward must beat the composition (which also pays for its forward launches -- the fused call's forward is the `fwd` leg, reported beside it as
`prefix_over_fwd_plus_bwd`).

    python scripts/bench_link_frames_vjp.py [--reps 3] [--out profiles/link_frames_vjp_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "robotics-toolbox-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM = 8.0e12
RING = 3
N = 1000000
ROBOTS = ("panda", "ur5")


def chain_and_marks(name):
    """(ETS, marks) of the robot's fkine_all: one walk from the base to the tip, a frame after every link"""
    import rtbhip
    if name == "panda":
        rb = rtbhip.models.Panda()
        k, marks = 0, [0]
        for seg in rb._links():
            k += len(seg)
            marks.append(k)
        return rb._ets, marks
    er = rtbhip.urdf.load("UR5").erobot()
    leaf = max((l for l in er.links if not l.children), key=lambda l: (er.ets(end=l).n, len(er.ets(end=l))))      # the arm's tip (the file has stub leaves too)
    path, l = [], leaf
    while l is not None:
        path.append(l)
        l = l.parent
    k, marks = 0, []
    for l in reversed(path):
        k += len(l.ets)
        marks.append(k)
    return er.ets(end=leaf), marks


def child():
    import numpy as np
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_link_frames_vjp needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name in ROBOTS:
        ets, marks = chain_and_marks(name)
        nm, w = len(marks), ets.q_width
        mk = np.ascontiguousarray(marks, dtype=np.int32)
        q = 6.0 * torch.rand((N, w), dtype=torch.float64, device="cuda") - 3.0
        G = 2.0 * torch.rand((N, nm, 4, 4), dtype=torch.float64, device="cuda") - 1.0
        prefixes = [(m, ets[:k]) for m, k in enumerate(marks) if ets[:k].n > 0]
        Gm = [G[:, m].contiguous() for m, _ in prefixes]
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        def bwd():
            gq = torch.empty_like(q)
            _lib.check(_lib.lib().rtbhip_link_frames_vjp(ets._handle(), C.c_void_p(q.data_ptr()), N, None, _lib.host_ptr(mk), nm, C.c_void_p(G.data_ptr()),
                                                         C.c_void_p(gq.data_ptr()), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return keep(gq)

        def prefix():
            a = q.detach().requires_grad_(True)
            Ts = [pre.eval(a[:, :pre.q_width]) for _, pre in prefixes]
            torch.autograd.backward(Ts, Gm)
            return keep(a.grad)

        # what is timed is what is tested: the fused gradient equals the composition's, and autograd's route to it has the raw call's bits
        fused, comp = bwd(), prefix()
        assert float((fused - comp).abs().max()) <= 1e-10
        a = q.detach().requires_grad_(True)
        torch.autograd.backward([ets.link_frames(a, marks)], [G])
        assert torch.equal(a.grad, fused)
        del a, comp, fused
        steps = {"fwd": lambda: keep(ets.link_frames(q, marks)), "bwd": bwd, "prefix": prefix}
        for leg, step in steps.items():
            ring.clear()
            out[name + "." + leg] = benchlib.sustained_ms(step)[0]
        out[name + ".nmarks"], out[name + ".q_width"], out[name + ".prefix_chains"] = nm, w, len(prefixes)
    print("BENCH_LINK_FRAMES_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_link_frames_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_LINK_FRAMES_VJP ")][-1]
    return json.loads(line[len("BENCH_LINK_FRAMES_VJP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_frames_vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    shape = {k: v[0] for k, v in runs.items() if k.split(".")[1] in ("nmarks", "q_width", "prefix_chains")}
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]}
            for k, v in sorted(runs.items()) if k not in shape}
    res = {"what": "Panda (22 transforms) and URDF UR5, the marks of fkine_all, N = 1e6, float64, sustained ms per call: fwd rtbhip_link_frames, "
                   "bwd rtbhip_link_frames_vjp, prefix one differentiable fkine per frame (forward + backward of the loop)",
           "reps": a.reps, "ring": RING, "shape": shape, "legs": legs, "hbm_frac": {}, "bwd_over_fwd": {}, "prefix_over_bwd": {}, "prefix_over_fwd_plus_bwd": {}}
    for r in ROBOTS:
        nm, w = shape[r + ".nmarks"], shape[r + ".q_width"]
        ms = {leg: legs[r + "." + leg]["median_ms"] for leg in ("fwd", "bwd", "prefix")}
        res["hbm_frac"][r + ".fwd"] = (128 * nm + 8 * w) * N / (ms["fwd"] * 1e-3) / HBM
        res["hbm_frac"][r + ".bwd"] = (128 * nm + 16 * w) * N / (ms["bwd"] * 1e-3) / HBM
        res["bwd_over_fwd"][r] = ms["bwd"] / ms["fwd"]
        res["prefix_over_bwd"][r] = ms["prefix"] / ms["bwd"]
        res["prefix_over_fwd_plus_bwd"][r] = ms["prefix"] / (ms["fwd"] + ms["bwd"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("shape", "legs", "hbm_frac", "bwd_over_fwd", "prefix_over_bwd", "prefix_over_fwd_plus_bwd")}, indent=1))


if __name__ == "__main__":
    main()
