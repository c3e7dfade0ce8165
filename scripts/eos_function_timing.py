#!/usr/bin/env python3
"""What the expression-defined equation of state "function" of EulerAEOS costs on the device, measured in ONE process,
after warm-up.

Two meshes: the Mach-3 step of the step2d_aeos workload (mach3_step_2d(995), 2.5 M gridpoints) and a 256 x 256 node
square. Three equations of state, each as the closed-form member and as the same member written as four expressions
     polytropic     the reference's default expressions, "(1.4 - 1.0) * rho * e"       7 instructions
     nasg           Noble-Abel stiffened gas                                            17 instructions
     jwl            Jones-Wilkins-Lee: two exp per evaluation                           49 instructions
six contexts per mesh on the same offline data that ALTERNATE in every pass, on a smooth admissible state. Per context
and pass:
     pre-pass       an event pair around `--steps` prepare_state_vector calls: boundary conditions, cycle 0
                    (k_precompute_aeos0 or k_precompute_aeos0_function), cycle 1. Everything but cycle 0 is the same
                    code on the same data, so the DIFFERENCE of a pair of rows is the difference of the two kernels.
     update         wall clock around `--steps` forward Euler updates (prepare_state_vector + step), synchronised at
                    either end
     interpolate    an event pair around `--steps` initial_values_interpolate calls of the `uniform` state: closed-form
                    specific_internal_energy(rho, p) against the sie program
The figure is the median pass with min - max.
Usage: eos_function_timing.py [--steps 20] [--passes 5] [--warmup 5] [--cells 995]   (prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_eos_function as he  # noqa: E402  (the members as expressions)
from ryujin_amd import HyperbolicModule, capi, offline  # noqa: E402
from ryujin_amd.initial_states import aeos_from_primitive_state  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--cells", type=int, default=995)
args = ap.parse_args()
lib = capi.load_hip()


def smooth_state(positions):
    x = np.asarray(positions, dtype=np.float64)
    phase = x[:, 0] + 2.0 * x[:, 1]
    rho = 1.2 + 0.6 * np.sin(2.0 * np.pi * phase)
    e = 5.0 + 1.5 * np.cos(3.0 * phase + 0.3)
    vel = np.stack([0.3 * np.sin(2.0 * phase), 0.3 * np.sin(2.0 * phase + 1.0)], axis=1)
    return aeos_from_primitive_state(rho, vel, e)


class Driver:
    def __init__(self, off, name, function):
        p = capi.Params()
        lib.ryujin_hip_default_params(C.byref(p), capi.EQ_EULER_AEOS, 2)
        he.member_params(p, name)
        p.cfl = 0.3
        self.label = f"{name}, {'expressions' if function else 'closed form'}"
        self.m = HyperbolicModule(off, p, backend="hip")
        if function:
            self.m.eos_configure_function(**({} if name == "polytropic" else he.member_expressions(p)))
        self.m.initial_values_configure("uniform", primitive_state=(1.4, 3.0, 1.0))
        U = smooth_state(off.positions)
        self.dirichlet = U[np.asarray(off.b_i).astype(np.int64)] if off.n_bdry else None
        self.old, self.new, self.scratch = self.m.new_state_vector(U), self.m.new_state_vector(), self.m.new_state_vector()
        self.wall, self.prepass, self.interpolate = [], [], []

    def updates(self, n):
        for _ in range(n):
            self.m.prepare_state_vector(self.old, 0.0, self.dirichlet)
            self.m.step(self.old, [], [], self.new)
            self.old, self.new = self.new, self.old
        lib.ryujin_hip_synchronize(self.m._ctx)

    def events(self, call):
        ctx, e = self.m._ctx, C.c_double()
        lib.ryujin_hip_event_record(ctx, 0)
        for _ in range(args.steps):
            call()
        lib.ryujin_hip_event_record(ctx, 1)
        assert lib.ryujin_hip_event_elapsed_ms(ctx, C.byref(e)) == 0
        return e.value / args.steps

    def measure(self, warmup):
        self.updates(warmup)
        w0 = time.perf_counter()
        self.updates(args.steps)
        self.wall.append((time.perf_counter() - w0) * 1e3 / args.steps)
        self.prepass.append(self.events(lambda: self.m.prepare_state_vector(self.old, 0.0, self.dirichlet)))
        self.interpolate.append(self.events(lambda: self.m.initial_values_interpolate(self.scratch, 0.0)))


def cell(v):
    return f"{np.median(v):.4f} ({min(v):.4f} - {max(v):.4f})"


print(f"<!-- scripts/eos_function_timing.py --steps {args.steps} --passes {args.passes} --warmup {args.warmup} "
      f"--cells {args.cells} -->\n")
for title, spec in (("the step2d_aeos mesh", offline.mach3_step_2d(args.cells)),
                    ("256 x 256 nodes", offline.rectangle_2d(255, (-1.0, -1.0), (1.0, 1.0), bc=capi.BC_DIRICHLET))):
    off = offline.SyntheticOffline(spec)
    drivers = [Driver(off, name, function) for name in ("polytropic", "nasg", "jwl") for function in (False, True)]
    for p in range(args.passes):
        for d in drivers:
            d.measure(args.warmup if p == 0 else 1)
    for d in drivers:
        assert np.isfinite(d.old.download()).all(), d.label
    print(f"### {title}: {off.n_owned} gridpoints, {off.n_bdry} boundary map entries, {args.passes} passes x "
          f"{args.steps} calls\n")
    print("| equation of state | pressure program | pre-pass, device events, ms | update, wall clock, ms "
          "| interpolate of `uniform`, device events, ms |")
    print("|---|---|---|---|---|")
    for d in drivers:
        info = d.m.eos_info()
        assert info["precompute_interpreted"] == (1 if info["kind"] == capi.EOS_FUNCTION else 0)
        print(f"| {d.label} | {info['n_instructions'][0]} instructions | {cell(d.prepass)} | {cell(d.wall)} | "
              f"{cell(d.interpolate)} |")
    print()
    for closed, function in zip(drivers[0::2], drivers[1::2]):
        dp = np.median(function.prepass) - np.median(closed.prepass)
        print(f"- {function.label}: k_precompute_aeos0_function - k_precompute_aeos0 = {dp:+.4f} ms "
              f"({dp * 1e6 / off.n_owned:+.3f} ns per gridpoint), pre-pass "
              f"{np.median(function.prepass) / np.median(closed.prepass):.2f} x, update "
              f"{np.median(function.wall) / np.median(closed.wall):.3f} x, interpolate "
              f"{np.median(function.interpolate) / np.median(closed.interpolate):.2f} x the closed form")
    print()
    for d in drivers:
        d.m.close()
