#!/usr/bin/env python3
"""The fused implicit-function adjoint of the inverse kinematics (rtbhip_ik_vjp) beside the forward solve it differentiates and beside the
composition it replaces: the DH-free Panda (models.Panda().ets()) and the URDF UR5's ets(), N = 1e6, float64.

Legs per robot, each timed with benchlib.sustained_ms (>= 30 ms warm-up, >= 30 ms inside ONE event pair, launches back to back); the results of
the last RING calls are kept alive so that every call gets different buffers:
    fwd    ETS.ik_LM(Tep, q0=q + 0.1 noise): the forward solve, unchanged by the adjoint's arrival -- the baseline of the same run
    bwd    rtbhip_ik_vjp asking for gTep, as the backward pass of rtbhip/autograd.py does: reads q, gq, Tep and success, writes gTep --
           8 (n + n + 16 + 16) + 4 bytes per row
    comp   the same gradient written in torch: a jacob0 launch that writes and re-reads (N, 6, n), J J^T by bmm, torch.linalg.solve on the batch
           of 6 x 6 systems, the products, the skew block, the success mask
Tep = fkine(q) of uniform q, so q is a solution and no solve is needed for the two backward legs.  Every repetition is a fresh child process.
`hbm_frac` = the bwd leg's byte model / time / 8 TB/s.  There is no pass / fail number: `comp_over_bwd` below 1 means the fused launch lost.

    python scripts/bench_ik_vjp.py [--reps 3] [--out profiles/ik_vjp_bench.json]
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


def chain(name):
    import rtbhip
    return rtbhip.models.Panda().ets() if name == "panda" else rtbhip.urdf.load("UR5").ets()


def child():
    import torch
    import benchlib
    import rtbhip
    from rtbhip import _lib
    assert torch.cuda.is_available() and rtbhip.device_count() > 0, "bench_ik_vjp needs a GPU"
    torch.manual_seed(1)
    out = {}
    for name in ROBOTS:
        ets = chain(name)
        n = ets.n
        q = 6.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 3.0
        gq = 2.0 * torch.rand((N, n), dtype=torch.float64, device="cuda") - 1.0
        Tep = ets.eval(q).reshape(N, 4, 4).contiguous()
        q0 = q + 0.1 * torch.randn_like(q)
        ok = torch.ones((N,), dtype=torch.int32, device="cuda")
        ring = []

        def keep(x):
            ring.append(x)
            if len(ring) > RING:
                ring.pop(0)
            return x

        def bwd():
            gT = torch.empty((N, 4, 4), dtype=torch.float64, device="cuda")
            p = lambda x: C.c_void_p(x.data_ptr())
            _lib.check(_lib.lib().rtbhip_ik_vjp(ets._handle(), p(q), N, p(Tep), p(ok), None, 0.0, p(gq), p(gT), None,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return keep(gT)

        def comp():
            J = ets.jacob0(q)
            y = torch.linalg.solve(J @ J.transpose(1, 2), J @ gq.unsqueeze(2)).squeeze(2) * ok.unsqueeze(1)
            gT = torch.zeros((N, 4, 4), dtype=torch.float64, device="cuda")
            gT[:, :3, 3] = y[:, :3]
            gT[:, :3, :3] = 0.5 * torch.cross(y[:, 3:].unsqueeze(2).expand(N, 3, 3), Tep[:, :3, :3], dim=1)
            return keep(gT)

        # what is timed is what is tested: the fused gradient is the composition's on the rows both can solve (uniform draws include
        # near-singular configurations, where two solvers of a 6 x 6 system part ways), and autograd's route to it has the raw call's bits
        fused, other = bwd(), comp()
        scale = other.abs().amax(dim=(1, 2)).clamp_min(1e-300)
        assert float(torch.median((fused - other).abs().amax(dim=(1, 2)) / scale)) <= 1e-9
        del fused, other, scale
        steps = {"fwd": lambda: keep(ets.ik_LM(Tep, q0=q0, joint_limits=False)), "bwd": bwd, "comp": comp}
        for leg, step in steps.items():
            ring.clear()
            out[name + "." + leg] = benchlib.sustained_ms(step)[0]
        out[name + ".n"] = n
    print("BENCH_IK_VJP " + json.dumps(out), flush=True)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench_ik_vjp: a child process failed (exit %d); nothing further is started" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_IK_VJP ")][-1]
    return json.loads(line[len("BENCH_IK_VJP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_vjp_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    runs = {}
    for rep in range(a.reps):
        for k, v in run_child().items():
            runs.setdefault(k, []).append(v)
    shape = {k: v[0] for k, v in runs.items() if k.split(".")[1] == "n"}
    legs = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 5) for x in v]}
            for k, v in sorted(runs.items()) if k not in shape}
    res = {"what": "models.Panda().ets() and URDF UR5 ets(), N = 1e6, float64, sustained ms per call: fwd ETS.ik_LM, bwd rtbhip_ik_vjp (gTep), "
                   "comp jacob0 + bmm + torch.linalg.solve + products + skew block",
           "reps": a.reps, "ring": RING, "shape": shape, "legs": legs, "bytes_per_row": {}, "hbm_frac": {}, "bwd_over_fwd": {}, "comp_over_bwd": {}}
    for r in ROBOTS:
        n = shape[r + ".n"]
        ms = {leg: legs[r + "." + leg]["median_ms"] for leg in ("fwd", "bwd", "comp")}
        res["bytes_per_row"][r] = 8 * (2 * n + 32) + 4
        res["hbm_frac"][r + ".bwd"] = res["bytes_per_row"][r] * N / (ms["bwd"] * 1e-3) / HBM
        res["bwd_over_fwd"][r] = ms["bwd"] / ms["fwd"]
        res["comp_over_bwd"][r] = ms["comp"] / ms["bwd"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("shape", "legs", "bytes_per_row", "hbm_frac", "bwd_over_fwd", "comp_over_bwd")}, indent=1))


if __name__ == "__main__":
    main()
