#!/usr/bin/env python3
"""The fused operational-space launch (rtbhip_opspace / rtbhip_tree_opspace) beside the forward inertia launch and beside the composition it
replaces: DH Puma560, DH Panda, URDF UR5 and the Kinova Gen3 arm (gripper left out: 7 joints), N = 1e6, float64.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    jac      the geometric jacob0 launch that feeds every other leg: timed separately, reported, not part of the legs below
    inertia  robot.inertia(q): the forward launch whose passes the fused kernel repeats -- the baseline of the same run
    mx / gx / asada / all   the fused launch asking for Mx, for Gx, for Asada's measure, for all three
    comp_mx / comp_gx / comp_asada / comp_all   the same quantities composed in torch, as the README used to advise: inertia (and gravload),
             torch.linalg.inv (six joints) or pinv, the products by bmm, torch.linalg.eigvalsh of the symmetrised Mx for Asada
`fp64_frac` = the pass count's operations (n passes of the unit-acceleration recursion, + 1 for gravity; ~1.5 kflop a 7-joint pass as
csrc/dyn_kernels.hip counts them, scaled by n / 7) over time over the fp64 vector peak, 78.6 TFLOP/s: the share of peak of the PASSES alone,
the tail's solves and eigenvalue sweeps counted as overhead.  There is no pass / fail number: `comp_over_fused` below 1 means the fused launch
lost.  Every repetition is a fresh child process.  A leg whose single call takes more than a second (the batched SVD behind
torch.linalg.pinv) is timed as one synchronised call after one warm-up call, and listed under `single_call_legs`.

    python scripts/bench_opspace.py [--reps 3] [--out profiles/opspace_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "robotics-toolbox-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FP64_PEAK = 78.6e12
PASS_FLOP_7 = 1500.0
RING = 3
SLOW_S = 1.0
N = 1000000
ROBOTS = ("puma560", "panda", "ur5", "gen3")
FUSED = {"mx": 1, "gx": 2, "asada": 4, "all": 7}


def robot(name):
    """(robot, ets of the end-effector path)"""
    import rtbhip
    if name == "puma560":
        r = rtbhip.models.DH.Puma560()
        return r, r.ets()
    if name == "panda":
        r = rtbhip.models.DH.Panda()
        return r, r.ets()
    r = rtbhip.urdf.load("UR5").erobot() if name == "ur5" else rtbhip.urdf.load("KinovaGen3").erobot(("robotiq_arg2f_base_link",))
    for l in reversed(r.links):
        if r.ets(None, l).n == r.n:
            return r, r._path(None, l)
    raise SystemExit("bench_opspace: no path of %s moves all its joints" % name)


def child():
    import numpy as np
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_opspace needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name in ROBOTS:
        rb, ets = robot(name)
        n = rb.n
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        J = ets.jacob0(q).contiguous()
        fn, handle = rb._opspace_call()
        gv = np.ascontiguousarray(rb._opspace_gravity(None), dtype=np.float64)
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        def fused(want):
            Mx = torch.empty((N, 6, 6), dtype=torch.float64, device="cuda") if want & 1 else None
            Gx = torch.empty((N, 6), dtype=torch.float64, device="cuda") if want & 2 else None
            a = torch.empty((N,), dtype=torch.float64, device="cuda") if want & 4 else None
            p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
            _lib.check(fn(handle, p(q), p(J), N, _lib.host_ptr(gv), 63, p(Mx), p(Gx), p(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return keep((Mx, Gx, a))

        def comp(want):
            X = torch.linalg.inv(J) if n == 6 else torch.linalg.pinv(J)
            Xt = X.transpose(1, 2)
            Mx = Gx = a = None
            if want & 5:
                Mx = Xt @ rb.inertia(q) @ X
            if want & 2:
                Gx = (Xt @ rb.gravload(q).unsqueeze(2)).squeeze(2)
            if want & 4:
                e = torch.linalg.eigvalsh(0.5 * (Mx + Mx.transpose(1, 2)))
                a = e[:, 0] / e[:, -1]
            return keep((Mx, Gx, a))

        # what is timed is what is tested: on the rows both can solve (uniform draws include near-singular configurations) the two agree
        f = fused(7)
        torch.cuda.synchronize()
        print("bench_opspace: %s fused launch done, composing the same in torch" % name, flush=True)
        c = comp(7)
        torch.cuda.synchronize()
        print("bench_opspace: %s composition done" % name, flush=True)
        for x, y in zip(f[:2], c[:2]):
            x, y = x.reshape(N, -1), y.reshape(N, -1)
            assert float(torch.median((x - y).abs().amax(dim=1) / y.abs().amax(dim=1).clamp_min(1e-300))) <= 1e-9
        assert float(torch.median((f[2] - c[2]).abs())) <= 1e-9
        del f, c
        steps = {"jac": lambda: keep(ets.jacob0(q)), "inertia": lambda: keep(rb.inertia(q))}
        for leg, want in FUSED.items():
            steps[leg] = (lambda w=want: fused(w))
            steps["comp_" + leg] = (lambda w=want: comp(w))
        for leg, step in steps.items():
            ring.clear()
            # a leg whose single call takes seconds (the batched SVD behind torch.linalg.pinv) is timed as ONE synchronised call after one
            # warm-up call instead of a 30 ms + 30 ms window of them: the figure is then a host clock around a device synchronise
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > SLOW_S:
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                out[name + "." + leg] = (time.perf_counter() - t0) * 1e3
                out.setdefault("single_call", []).append(name + "." + leg)
            else:
                out[name + "." + leg] = benchlib.sustained_ms(step)[0]
            print("bench_opspace: %s.%s %.4f ms" % (name, leg, out[name + "." + leg]), flush=True)
        out[name + ".n"] = n
    print("BENCH_OPSPACE " + json.dumps(out), flush=True)


def run_child():
    """the child's lines are passed on as they come (a silent parent looks hung to whoever watches the run)"""
    pr = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True)
    last = None
    for line in pr.stdout:
        if line.startswith("BENCH_OPSPACE "):
            last = line
        else:
            sys.stdout.write(line)
            sys.stdout.flush()
    if pr.wait() != 0 or last is None:
        raise SystemExit("bench_opspace: a child process failed (exit %d); nothing further is started" % pr.returncode)
    return json.loads(last[len("BENCH_OPSPACE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opspace_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    single = set()
    for rep in range(a.reps):
        got = run_child()
        single |= set(got.pop("single_call", []))
        for k, v in got.items():
            runs.setdefault(k, []).append(v)
    shape = {k: v[0] for k, v in runs.items() if k.split(".")[1] == "n"}
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]}
            for k, v in sorted(runs.items()) if k not in shape}
    res = {"what": "DH Puma560, DH Panda, URDF UR5, Kinova Gen3 arm; N = 1e6, float64, sustained ms per call: jac jacob0, inertia the forward launch, "
                   "mx / gx / asada / all the fused rtbhip_opspace launch, comp_* inertia (+ gravload) + torch.linalg.inv or pinv + bmm (+ eigvalsh)",
           "reps": a.reps, "ring": RING, "shape": shape, "legs": legs, "single_call_legs": sorted(single), "fused_over_inertia": {}, "comp_over_fused": {}, "fp64_frac": {}}
    for r in ROBOTS:
        n = shape[r + ".n"]
        ms = lambda leg: legs[r + "." + leg]["median_ms"]
        for leg in FUSED:
            res["fused_over_inertia"][r + "." + leg] = ms(leg) / ms("inertia")
            res["comp_over_fused"][r + "." + leg] = ms("comp_" + leg) / ms(leg)
            passes = (n if FUSED[leg] & 5 else 0) + (1 if FUSED[leg] & 2 else 0)          # Gx alone runs the gravity pass only
            res["fp64_frac"][r + "." + leg] = passes * PASS_FLOP_7 * (n / 7.0) * N / (ms(leg) * 1e-3) / FP64_PEAK
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("shape", "legs", "fused_over_inertia", "comp_over_fused", "fp64_frac")}, indent=1))


if __name__ == "__main__":
    main()
