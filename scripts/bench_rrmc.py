#!/usr/bin/env python3
"""The fused resolved-rate step and servo loop (rtbhip_rrmc) beside the composition they replace, on the same commit's other entry points:
models.Panda().ets() and the URDF UR5's ets(), N = 1e6, float64, both methods ("rpy" with jacobe, "angle-axis" with jacob0).

Legs per robot and method, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the
results of the last RING calls are kept alive so that every call gets different buffers (a ring of three output sets):
    step1   rtbhip_rrmc, steps = 1, qd and arrived out: reads q and Tep, writes qd and one flag byte
    loop8   rtbhip_rrmc, steps = 8 with gain dt = 1 towards Tep = fkine(q + 0.3 U(-1, 1)): q_out, arrived and its out -- rows leave the loop as
            they arrive, so this is the cost of the iterations actually taken (`its_mean` says how many)
    comp    one step written with what existed before: the fkine_jacob0 launch (jacobe and an fkine launch for "rpy") that writes and re-reads
            (N, 6, n) and (N, 4, 4), rtbhip_p_servo, torch.linalg.pinv (Panda) or torch.linalg.solve (UR5: six joints), bmm
`comp_x8` is 8 x comp: the composition of the loop is eight such steps and is not run.  Every repetition is a fresh child process.  A leg whose
single call takes more than a second (the batched SVD behind torch.linalg.pinv) is timed as one synchronised call after one warm-up call, and
listed under `single_call_legs` (scripts/bench_opspace.py does the same).
`hbm_frac` = the byte model 8 (3 n + 16) + 5 per row / time / 8 TB/s, for step1 (the loop does up to eight steps of arithmetic on the same bytes).
There is no pass / fail number: `comp_over_step1` below 1 means the fused launch lost.

    python scripts/bench_rrmc.py [--reps 5] [--out profiles/rrmc_bench.json]
"""
import argparse
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

HBM = 8.0e12
RING = 3
N = 1000000
ROBOTS = ("panda", "ur5")
METHODS = ("rpy", "angle-axis")


def chain(name):
    import rtbhip
    return rtbhip.models.Panda().ets() if name == "panda" else rtbhip.urdf.load("UR5").ets()


def child():
    import torch
    import benchlib
    import rtbhip
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_rrmc needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name in ROBOTS:
        ets = chain(name)
        n = ets.n
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        Tep = ets.eval(q + 0.3 * (2.0 * torch.rand_like(q) - 1.0)).reshape(N, 4, 4).contiguous()
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        for method in METHODS:
            def step1():
                return keep(rtbhip.servo.rrmc(ets, q, Tep, method=method))

            def loop8():
                return keep(rtbhip.servo.servo(ets, q, Tep, 0.5, 8, gain=2.0, method=method))

            def comp():
                if method == "rpy":
                    T, J = ets.eval(q), ets.jacobe(q)
                else:
                    T, J = ets.fkine_jacob0(q)
                v, arrived = rtbhip.p_servo(T.reshape(N, 4, 4), Tep, method=method)
                if n == 6:
                    qd = torch.linalg.solve(J, v.unsqueeze(2)).squeeze(2)
                else:
                    qd = torch.bmm(torch.linalg.pinv(J), v.unsqueeze(2)).squeeze(2)
                return keep((qd, arrived))

            # what is timed is what is tested: the fused rate is the composition's on the rows both can solve (uniform draws include near-singular
            # configurations, where two solvers part ways)
            fused = step1()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other = comp()
            torch.cuda.synchronize()
            slow = time.perf_counter() - t0 > 1.0          # (that call was the slow leg's warm-up)
            scale = other[0].abs().amax(dim=1).clamp_min(1e-300)
            assert float(torch.median((fused[0] - other[0]).abs().amax(dim=1) / scale)) <= 1e-9
            assert float((fused[1] == other[1]).double().mean()) > 0.999
            its = loop8()[2]
            out["%s.%s.its_mean" % (name, method)] = float(its.double().mean())
            del fused, other, scale, its
            for leg, step in (("step1", step1), ("loop8", loop8), ("comp", comp)):
                ring.clear()
                key = "%s.%s.%s" % (name, method, leg)
                if leg == "comp" and slow:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    out[key] = (time.perf_counter() - t0) * 1e3
                    out.setdefault("single_call", []).append(key)
                else:
                    out[key] = benchlib.sustained_ms(step)[0]
                print("bench_rrmc: %s %.4f ms" % (key, out[key]), flush=True)
        out[name + ".n"] = n
    print("BENCH_RRMC " + json.dumps(out), flush=True)


def run_child():
    """the child's lines are passed on as they come (a silent parent looks hung to whoever watches the run)"""
    pr = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True)
    last = None
    for line in pr.stdout:
        if line.startswith("BENCH_RRMC "):
            last = line
        else:
            sys.stdout.write(line)
            sys.stdout.flush()
    if pr.wait() != 0 or last is None:
        raise SystemExit("bench_rrmc: a child process failed (exit %d); nothing further is started" % pr.returncode)
    return json.loads(last[len("BENCH_RRMC "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrmc_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs, single = {}, set()
    for rep in range(a.reps):
        got = run_child()
        single |= set(got.pop("single_call", []))
        for k, v in got.items():
            runs.setdefault(k, []).append(v)
    shape = {k: v[0] for k, v in runs.items() if k.endswith(".n")}
    its = {k: statistics.median(v) for k, v in runs.items() if k.endswith(".its_mean")}
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]}
            for k, v in sorted(runs.items()) if k not in shape and k not in its}
    res = {"what": "models.Panda().ets() and URDF UR5 ets(), N = 1e6, float64, sustained ms per call: step1 rtbhip_rrmc steps = 1, loop8 rtbhip_rrmc "
                   "steps = 8 (gain dt = 1), comp fkine / Jacobian launch + rtbhip_p_servo + torch.linalg.pinv (UR5: solve) + bmm; comp_x8 = 8 x comp, not run",
           "reps": a.reps, "ring": RING, "shape": shape, "its_mean": its, "legs": legs, "single_call_legs": sorted(single), "bytes_per_row": {}, "hbm_frac": {}, "comp_over_step1": {},
           "comp_x8_over_loop8": {}}
    for r in ROBOTS:
        n = shape[r + ".n"]
        res["bytes_per_row"][r] = 8 * (3 * n + 16) + 5
        for m in METHODS:
            ms = {leg: legs["%s.%s.%s" % (r, m, leg)]["median_ms"] for leg in ("step1", "loop8", "comp")}
            res["hbm_frac"]["%s.%s.step1" % (r, m)] = res["bytes_per_row"][r] * N / (ms["step1"] * 1e-3) / HBM
            res["comp_over_step1"]["%s.%s" % (r, m)] = ms["comp"] / ms["step1"]
            res["comp_x8_over_loop8"]["%s.%s" % (r, m)] = 8.0 * ms["comp"] / ms["loop8"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("shape", "its_mean", "legs", "single_call_legs", "bytes_per_row", "hbm_frac", "comp_over_step1", "comp_x8_over_loop8")}, indent=1))


if __name__ == "__main__":
    main()
