#!/usr/bin/env python3
"""What the Riemann-data, shock-front, ramp-up and Noh states cost on the device, measured in ONE process, after
warm-up; modelled on scripts/initial_values_timing.py. Device events where a kernel is timed, wall clock for whole
Runge-Kutta steps (the host is what differs); `--passes` passes (default three), median with min - max.

1. initial_values_interpolate of 2.5 M points (1581 x 1581 nodes): `shock front`, `ramp up`, `noh` against `uniform`.
2. prepare_state_vector_iv per call on the 256 x 256 box, `ramp up` against `uniform` (device events over 200 calls;
   the Dirichlet kernel is the only kernel of the call that differs).
3. One ERK33 step on the 256 x 256 box
   a. with `ramp up` inflow: time_step_iv against time_step_fn with the numpy restatement as callback;
   b. with `shock front`: time_step_iv of the built-in state against time_step_iv of the same state written as a
      `function` expression (ramp up cannot be written that way: it blends two conserved states).
Usage: initial_values_library_timing.py [--steps 40] [--passes 3] [--warmup 10]   (prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryujin_amd import HyperbolicModule, capi, offline  # noqa: E402
from ryujin_amd import initial_states as ist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
lib = capi.load_hip()
e = C.c_double()

RAMP = dict(primitive_state_initial=(1.4, 0.5, 1.0), primitive_state_final=(1.4, 3.0, 1.0), time_initial=0.0,
            time_final=2.0)
SHOCK = dict(primitive_state=(1.4, 0.0, 1.0), mach_number=2.0, position=(-2.0, 0.0))
CONFIGURE = {
    "uniform": lambda m: m.initial_values_configure("uniform", primitive_state=(1.4, 0.5, 1.0)),
    "shock front": lambda m: m.initial_values_configure("shock front", **SHOCK),
    "ramp up": lambda m: m.initial_values_configure("ramp up", **RAMP),
    "noh": lambda m: m.initial_values_configure("noh"),
}


def fmt(v, digits=4):
    return f"{np.median(v):.{digits}f} ({min(v):.{digits}f} - {max(v):.{digits}f})"


def med(v):
    return float(np.median(v))


def box(n):
    off = offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    return off, HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")


def events(m, body):
    lib.ryujin_hip_synchronize(m._ctx)
    lib.ryujin_hip_event_record(m._ctx, 0)
    body()
    lib.ryujin_hip_event_record(m._ctx, 1)
    assert lib.ryujin_hip_event_elapsed_ms(m._ctx, C.byref(e)) == 0
    return e.value


def rk_steps(m, state, temps, n, t, fn=None):
    for _ in range(n):
        if fn is None:
            t += m.time_step("erk 33", state, temps, "device", t=t)
        else:
            t += m.time_step("erk 33", state, temps, t=t, dirichlet_fn=fn)
    lib.ryujin_hip_synchronize(m._ctx)
    return t


def measure_interpolate():
    off, m = box(1580)
    sv = m.new_state_vector()
    dev = {k: [] for k in CONFIGURE}
    for p in range(args.passes + 1):
        for key, configure in CONFIGURE.items():
            configure(m)
            ms = events(m, lambda: m.initial_values_interpolate(sv, 0.25))
            if p > 0:  # the first pass is the warm-up
                dev[key].append(ms)
    print(f"\n### interpolate: {off.n_relevant} points, {args.passes} passes\n")
    print("| state | ms, median (min - max), device events | ratio to uniform | GB/s (48 B per point) |")
    print("|---|---|---|---|")
    for key in CONFIGURE:
        print(f"| {key} | {fmt(dev[key])} | {med(dev[key]) / med(dev['uniform']):.2f} | "
              f"{off.n_relevant * 48 / (med(dev[key]) * 1e-3) / 1e9:.0f} |")
    m.close()
    off.close()


def ramp_up_numpy(bpos):
    """the numpy restatement of `ramp up` at the boundary positions, as a callback of time_step_fn"""
    n = len(bpos)
    vel_i, vel_f = np.zeros((n, 2)), np.zeros((n, 2))
    vel_i[:, 0], vel_f[:, 0] = RAMP["primitive_state_initial"][1], RAMP["primitive_state_final"][1]

    def fn(t):
        a = ist.euler_from_primitive(np.full(n, RAMP["primitive_state_initial"][0]), vel_i,
                                     np.full(n, RAMP["primitive_state_initial"][2]))
        b = ist.euler_from_primitive(np.full(n, RAMP["primitive_state_final"][0]), vel_f,
                                     np.full(n, RAMP["primitive_state_final"][2]))
        return ist.ramp_up_blend(a, b, t, RAMP["time_initial"], RAMP["time_final"])
    return fn


def shock_front_expressions():
    (rho_L, u_L, p_L), S3 = ist.euler_shock_front_constants(SHOCK["primitive_state"], SHOCK["mach_number"], 1.4)
    rho_R, u_R, p_R = SHOCK["primitive_state"]
    pick = lambda r, l: f"if(x - {S3!r} * t > 0, {r!r}, {l!r})"  # noqa: E731
    return [pick(rho_R, rho_L), pick(u_R, u_L), "0", pick(p_R, p_L)]


def measure_box():
    off, m = box(256)
    m.cfl = 0.3
    bpos = off.b_positions
    calls = 200
    # 2. the Dirichlet kernel per call
    state = m.new_state_vector()
    CONFIGURE["uniform"](m)
    m.initial_values_interpolate(state, 0.0)
    prepare = {"uniform": [], "ramp up": []}
    for p in range(args.passes + 1):
        for key in prepare:
            CONFIGURE[key](m)
            ms = events(m, lambda: [m.prepare_state_vector(state, 0.5, "device") for _ in range(calls)]) / calls
            if p > 0:
                prepare[key].append(ms)
    print(f"\n### Dirichlet kernel, 256 x 256 box: {off.n_bdry} boundary map entries, {args.passes} passes\n")
    print(f"| prepare_state_vector_iv per call (device events over {calls} calls) | ms, median (min - max) |")
    print("|---|---|")
    for key, v in prepare.items():
        print(f"| {key} | {fmt(v)} |")
    print(f"\nramp up - uniform = {(med(prepare['ramp up']) - med(prepare['uniform'])) * 1e3:.2f} us per call.")

    # 3a. ERK33 with ramp up inflow
    temps = [m.new_state_vector() for _ in range(3)]
    CONFIGURE["ramp up"](m)
    m.initial_values_interpolate(state, 0.0)
    fn = ramp_up_numpy(bpos)
    step = {"iv": [], "fn numpy": []}
    t = 0.0
    for p in range(args.passes + 1):
        for key, callback in (("iv", None), ("fn numpy", fn)):
            t = rk_steps(m, state, temps, args.warmup if p == 0 else 2, t, callback)
            w0 = time.perf_counter()
            t = rk_steps(m, state, temps, args.steps, t, callback)
            if p > 0:
                step[key].append((time.perf_counter() - w0) * 1e3 / args.steps)
    assert np.isfinite(state.download()).all() and RAMP["time_initial"] < t < RAMP["time_final"]
    print(f"\n### ERK33 step, ramp up inflow, 256 x 256 box: {off.n_owned} gridpoints, {args.passes} passes x "
          f"{args.steps} steps, t = {t:.3f} at the end (inside the ramp)\n")
    print("| driver | ms per RK step, wall clock, median pass (min - max) |")
    print("|---|---|")
    for key, v in step.items():
        print(f"| {key} | {fmt(v)} |")
    print(f"\nfn numpy / iv = {med(step['fn numpy']) / med(step['iv']):.2f}.")

    # 3b. ERK33 with the shock front, built-in against the function expression
    configure = {"built-in": CONFIGURE["shock front"],
                 "function": lambda mod: mod.initial_values_configure_function(shock_front_expressions(),
                                                                               position=SHOCK["position"])}
    configure["built-in"](m)
    m.initial_values_interpolate(state, 0.0)
    step = {k: [] for k in configure}
    t = 0.0
    for p in range(args.passes + 1):
        for key in configure:
            configure[key](m)
            t = rk_steps(m, state, temps, args.warmup if p == 0 else 2, t)
            w0 = time.perf_counter()
            t = rk_steps(m, state, temps, args.steps, t)
            if p > 0:
                step[key].append((time.perf_counter() - w0) * 1e3 / args.steps)
    assert np.isfinite(state.download()).all()
    print(f"\n### ERK33 step, shock front, 256 x 256 box, {args.passes} passes x {args.steps} steps\n")
    print("| state | ms per RK step, wall clock, median pass (min - max) |")
    print("|---|---|")
    for key, v in step.items():
        print(f"| time_step_iv, {key} | {fmt(v)} |")
    print(f"\nfunction / built-in = {med(step['function']) / med(step['built-in']):.3f}.")
    m.close()
    off.close()


print(f"<!-- scripts/initial_values_library_timing.py --steps {args.steps} --passes {args.passes} "
      f"--warmup {args.warmup} -->")
measure_interpolate()
measure_box()
