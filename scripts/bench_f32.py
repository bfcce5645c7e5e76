#!/usr/bin/env python3
"""float32 storage against fp64 on the two bandwidth-bound calls: Panda ETS fkine_jacob0 (N = 1e6) and DH Panda rne (N = 1e7).

Legs, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back), the outputs of the last
RING calls kept alive so that the allocator hands every call a different buffer (a ring of output sets larger than the 256 MiB memory-side cache:
the figure is the streaming one, not the rewrite-in-place one):
    a   fp64 tensors in, fp64 out                               (also with --parent-tree: the same leg on another checkout, e.g. the parent commit)
    b   float32 tensors in, float32 out                         (rtbhip_fkine_jacob_f32 / rtbhip_rne_f32)
    c   what a float32 user did before: q.double() -> fp64 call -> .float()
Every repetition is a fresh child process (its own context, allocator and code-object load); with --parent-tree the two checkouts alternate.
Bytes per configuration: fkine_jacob0 8 qw + 128 + 48 n = 520 (fp64), 260 (float32); rne 32 n = 224, 112.  `hbm_frac` = those bytes / time / 8 TB/s.

    python scripts/bench_f32.py [--reps 5] [--parent-tree DIR] [--out profiles/f32_io_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("BENCH_F32_TREE") or ROOT          # a child timing another checkout (--parent-tree) imports the package from there
for p in (TREE, os.path.join(TREE, "robotics-toolbox-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM = 8.0e12
RING = 3


def child(legs):
    import torch
    import benchlib
    import rtbhip
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_f32 needs a GPU"
    torch.manual_seed(1)
    out = {}
    ets, dh = rtbhip.models.Panda().ets(), rtbhip.models.DH.Panda()
    Nk, Nr = 1000000, 10000000
    q32 = (6.0 * torch.rand((Nk, 7), dtype=torch.float32, device="cuda") - 3.0)
    q64 = q32.double()
    r32 = [(4.0 * torch.rand((Nr, 7), dtype=torch.float32, device="cuda") - 2.0) for _ in range(3)]
    r64 = [x.double() for x in r32] if ("a" in legs or "c" in legs) else None
    ring = []

    def keep(x):
        ring.append(x)
        if len(ring) > RING:
            ring.pop(0)

    steps = {
        ("kin", "a"): lambda: keep(ets.fkine_jacob0(q64)),
        ("kin", "b"): lambda: keep(ets.fkine_jacob0(q32)),
        ("kin", "c"): lambda: keep(tuple(x.float() for x in ets.fkine_jacob0(q32.double()))),
        ("rne", "a"): lambda: keep(dh.rne(*r64)),
        ("rne", "b"): lambda: keep(dh.rne(*r32)),
        ("rne", "c"): lambda: keep(dh.rne(*[x.double() for x in r32]).float()),
    }
    for (call, leg), step in steps.items():
        if leg not in legs:
            continue
        ring.clear()
        ms, reps, warm = benchlib.sustained_ms(step)
        out["%s_%s" % (call, leg)] = ms
    if "b" in legs and "a" in legs:            # what is timed is what is tested: the float32 outputs are the rounded fp64 ones
        T32, J32 = ets.fkine_jacob0(q32)
        T64, J64 = ets.fkine_jacob0(q64)
        assert torch.equal(T32, T64.float()) and torch.equal(J32, J64.float())
        assert torch.equal(dh.rne(*r32), dh.rne(*r64).float())
    print("BENCH_F32 " + json.dumps(out), flush=True)


def run_child(tree, legs):
    env = dict(os.environ)
    env.pop("BENCH_F32_TREE", None)
    if tree:
        env["BENCH_F32_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", legs], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_f32: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_F32 ")][-1]
    return json.loads(line[len("BENCH_F32 "):])


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "runs_ms": [round(x, 5) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="another checkout with its library built (the parent commit): its fp64 legs alternate with this one's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f32_io_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    runs = {}
    for rep in range(a.reps):
        if a.parent_tree:
            for k, v in run_child(os.path.abspath(a.parent_tree), "a").items():
                runs.setdefault("parent_" + k, []).append(v)
        for k, v in run_child(None, "abc").items():
            runs.setdefault(k, []).append(v)
    res = {"what": "float32 storage vs fp64, sustained ms per call; Panda ETS fkine_jacob0 N=1e6 (kin), DH Panda rne N=1e7 (rne); "
                   "a fp64, b float32, c q.double() -> fp64 call -> .float(); parent_*_a = leg a on the parent commit's checkout",
           "reps": a.reps, "ring": RING, "legs": {k: spread(v) for k, v in sorted(runs.items())}}
    L = res["legs"]
    byt = {"kin": (520.0 * 1e6, 260.0 * 1e6), "rne": (224.0 * 1e7, 112.0 * 1e7)}
    for call in ("kin", "rne"):
        am, bm, cm = (L["%s_%s" % (call, x)]["median_ms"] for x in "abc")
        res[call] = {"a_over_b": am / bm, "c_over_b": cm / bm,
                     "b_faster_than_c_by_ms": cm - bm, "c_spread_ms": L[call + "_c"]["spread_ms"], "b_spread_ms": L[call + "_b"]["spread_ms"],
                     "b_beats_c_beyond_spread": (L[call + "_c"]["min_ms"] - L[call + "_b"]["max_ms"]) > 0 and (cm - bm) > L[call + "_c"]["spread_ms"],
                     "hbm_frac_a": byt[call][0] / (am * 1e-3) / HBM, "hbm_frac_b": byt[call][1] / (bm * 1e-3) / HBM}
        if a.parent_tree:
            pm = L["parent_%s_a" % call]
            res[call]["a_vs_parent_a_ms"] = am - pm["median_ms"]
            res[call]["parent_a_spread_ms"] = pm["spread_ms"]
            res[call]["a_within_parent_spread"] = abs(am - pm["median_ms"]) <= max(pm["spread_ms"], L[call + "_a"]["spread_ms"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("kin", "rne")}, indent=1))


if __name__ == "__main__":
    main()
