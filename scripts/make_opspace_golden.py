#!/usr/bin/env python3
"""Writes tests/golden/opspace_reference.npz: what the REFERENCE's own classes return for the operational-space dynamics, recorded once so that
the tests can hold the NumPy restatement (tests/opspace_cases.py) and the device to it where the reference is not installed.

Runs only where the reference checkout and its compiled extensions are available (oracle/ref_classes.py, oracle/_ref): the reference's DHRobot,
Dynamics mixin and models/DH/{Puma560, Panda}.py are executed unmodified on the reference's fknm / frne.  Robots: Puma560 and the DH Panda, at qn
(qr for the Panda), qz and six seeded rows.  Per robot X the file holds

    X_q (8, n)          the configurations
    X_J (8, 6, n)       jacob0(q): the geometric Jacobian, what representation=None selects and what Asada's measure uses
    X_Mx (8, 6, 6)      inertia_x(q, representation=None)         X_Gx (8, 6)     gravload_x(q, representation=None)
    X_asada_all / _trans / _rot (8,)    manipulability(q, method="asada", axes=...)

A row at which the reference raises (numpy.linalg.inv at an exactly singular Jacobian) is recorded as NaN.  Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def rows_of(robot, seed):
    rng = np.random.default_rng(seed)
    named = robot.qn if hasattr(robot, "qn") else robot.qr
    return np.vstack([np.asarray(named, dtype=np.float64), np.zeros(robot.n), rng.uniform(-2.5, 2.5, (6, robot.n))])


def record(robot, name, seed, out):
    q = rows_of(robot, seed)
    n = robot.n
    keys = {"J": (6, n), "Mx": (6, 6), "Gx": (6,), "asada_all": (), "asada_trans": (), "asada_rot": ()}
    rec = {k: np.full((len(q),) + s, np.nan) for k, s in keys.items()}
    calls = {"J": lambda qk: robot.jacob0(qk), "Mx": lambda qk: robot.inertia_x(qk, representation=None),
             "Gx": lambda qk: robot.gravload_x(qk, representation=None),
             "asada_all": lambda qk: robot.manipulability(qk, method="asada", axes="all"),
             "asada_trans": lambda qk: robot.manipulability(qk, method="asada", axes="trans"),
             "asada_rot": lambda qk: robot.manipulability(qk, method="asada", axes="rot")}
    for i, qk in enumerate(q):
        for k, f in calls.items():
            try:
                rec[k][i] = np.real(np.asarray(f(qk), dtype=np.complex128)) if k.startswith("asada") else np.asarray(f(qk), dtype=np.float64)
            except np.linalg.LinAlgError:
                pass
    out[name + "_q"] = q
    for k, v in rec.items():
        out[name + "_" + k] = v


def main():
    from oracle import ref_classes, ref_harness
    ns = ref_classes.load_dh(ref_harness._load("fknm"), ref_harness._load("frne"), "ref-dh")
    out = {}
    record(ns.Puma560(), "puma560", 11, out)
    record(ns.PandaDH(), "panda", 12, out)
    path = os.path.join(ROOT, "tests", "golden", "opspace_reference.npz")
    np.savez(path, **out)
    print("wrote %s: %s" % (path, ", ".join("%s %s" % (k, v.shape) for k, v in out.items())))


if __name__ == "__main__":
    main()
