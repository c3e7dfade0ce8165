#!/usr/bin/env python3
"""What the expression-defined flux "function" costs on the device, measured in ONE process, after warm-up.

The 2-D KPP case on the 2.5 M gridpoint lattice (1581 x 1581 nodes on [-2, 2] x [-2.5, 1.5], Dirichlet all round,
3.5 pi inside the unit circle and 0.25 pi outside), one forward Euler update = prepare_state_vector + step. Three fluxes
     kpp            the built-in RYUJIN_FLUX_KPP: the baseline
     sin;cos        the same flux as RYUJIN_FLUX_FUNCTION, "sin(u); cos(u)"
     buckley        Buckley-Leverett in both directions, "u*u/(u*u + 0.25*(1-u)*(1-u))" (state 1 inside, 0 outside)
each with sc_use_averaged_entropy off and on: six contexts on the same offline data that ALTERNATE in every pass.
Per context and pass: milliseconds per update (wall clock around `--steps` updates with a synchronisation at either end),
the device time of the step-2 kernel and of step 3 -- boundary pairs, diagonal, tau_max -- (the library's event pairs,
ryujin_hip_get_timers_accum: ms[0] and ms[2]) and of the pre-pass (an event pair around `--steps` prepare_state_vector
calls). The figure is the median pass with min - max.
Usage: flux_function_timing.py [--steps 20] [--passes 5] [--warmup 5] [--cells 1580]   (prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryujin_amd import HyperbolicModule, capi, offline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--cells", type=int, default=1580)
args = ap.parse_args()
lib = capi.load_hip()

BUCKLEY = "u*u/(u*u + 0.25*(1-u)*(1-u))"
FLUXES = [("kpp", None), ("sin;cos", "sin(u); cos(u)"), ("buckley", BUCKLEY + "; " + BUCKLEY)]

off = offline.SyntheticOffline(offline.rectangle_2d(args.cells, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
x = np.asarray(off.positions).reshape(-1, 2)
inside = (x * x).sum(axis=1) < 1.0
b_i = np.asarray(off.b_i).astype(np.int64)


class Driver:
    def __init__(self, name, expression, averaged):
        p = capi.Params()
        lib.ryujin_hip_default_params(C.byref(p), capi.EQ_SCALAR_CONSERVATION, 2)
        p.sc_flux = capi.FLUX_KPP
        p.sc_use_averaged_entropy = 1 if averaged else 0
        p.cfl = 0.5
        self.label = f"{name}, averaged entropy {'on' if averaged else 'off'}"
        self.m = HyperbolicModule(off, p, backend="hip")
        if expression:
            self.m.flux_configure_function(expression, 1e-10)
        U = np.where(inside, 1.0, 0.0) if name == "buckley" else np.where(inside, 3.5 * np.pi, 0.25 * np.pi)
        U = U.reshape(-1, 1)
        self.dirichlet = U[b_i]
        self.old, self.new = self.m.new_state_vector(U), self.m.new_state_vector()
        lib.ryujin_hip_set_timers(self.m._ctx, 1)
        self.wall, self.step2, self.step3, self.prepass = [], [], [], []

    def updates(self, n):
        for _ in range(n):
            self.m.prepare_state_vector(self.old, 0.0, self.dirichlet)
            self.m.step(self.old, [], [], self.new)
            self.old, self.new = self.new, self.old
        lib.ryujin_hip_synchronize(self.m._ctx)

    def measure(self, warmup):
        ctx = self.m._ctx
        ms, count, e = (C.c_double * 8)(), C.c_uint(0), C.c_double()
        self.updates(warmup)
        lib.ryujin_hip_get_timers_accum(ctx, ms, C.byref(count), 1)
        w0 = time.perf_counter()
        self.updates(args.steps)
        self.wall.append((time.perf_counter() - w0) * 1e3 / args.steps)
        lib.ryujin_hip_get_timers_accum(ctx, ms, C.byref(count), 1)
        self.step2.append(ms[0] / max(count.value, 1))
        self.step3.append(ms[2] / max(count.value, 1))
        lib.ryujin_hip_event_record(ctx, 0)
        for _ in range(args.steps):
            self.m.prepare_state_vector(self.old, 0.0, self.dirichlet)
        lib.ryujin_hip_event_record(ctx, 1)
        assert lib.ryujin_hip_event_elapsed_ms(ctx, C.byref(e)) == 0
        self.prepass.append(e.value / args.steps)


drivers = [Driver(name, expression, averaged) for averaged in (False, True) for name, expression in FLUXES]
for p in range(args.passes):
    for d in drivers:
        d.measure(args.warmup if p == 0 else 1)
for d in drivers:
    assert np.isfinite(d.old.download()).all(), d.label


def cell(v):
    return f"{np.median(v):.4f} ({min(v):.4f} - {max(v):.4f})"


print(f"<!-- scripts/flux_function_timing.py --steps {args.steps} --passes {args.passes} --warmup {args.warmup} "
      f"--cells {args.cells} -->\n")
print(f"### {off.n_owned} gridpoints, {off.n_bdry} boundary map entries, {args.passes} passes x {args.steps} updates\n")
print("| flux | ms per update, wall clock | pre-pass (prepare_state_vector), device events | step-2 kernel, device events "
      "| step 3, device events | step2_interpreted |")
print("|---|---|---|---|---|---|")
for d in drivers:
    print(f"| {d.label} | {cell(d.wall)} | {cell(d.prepass)} | {cell(d.step2)} | {cell(d.step3)} | "
          f"{d.m.flux_info()['step2_interpreted']} |")
base = {False: drivers[0], True: drivers[3]}
print()
for q, d in enumerate(drivers):
    b = base[q >= 3]
    if d is b:
        continue
    print(f"- {d.label}: update {np.median(d.wall) / np.median(b.wall):.2f} x the built-in kpp, pre-pass "
          f"{np.median(d.prepass) / np.median(b.prepass):.2f} x, step-2 kernel "
          f"{np.median(d.step2) / np.median(b.step2):.2f} x, step 3 {np.median(d.step3) / np.median(b.step3):.2f} x")
