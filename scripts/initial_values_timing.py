#!/usr/bin/env python3
"""What the device-resident InitialValues buy, measured in ONE process per invocation, after warm-up.

1. Milliseconds per Runge-Kutta step (ERK33, wall clock: the host is what differs), three cases
     leblanc-1d     the l6 Le Blanc tube, 1601 nodes, 2 boundary entries
     vortex-256     the isentropic vortex on 256 x 256 cells, Dirichlet all round (latency-bound)
     vortex-1024    the same on 1024 x 1024 cells
   and four drivers that ALTERNATE in every pass
     iv             ryujin_hip_time_step_iv: Dirichlet data evaluated on the device, nothing waits for tau
     fn numpy       ryujin_hip_time_step_fn with the numpy restatement (ryujin_amd.initial_states) as callback: what
                    users had before
     fn cached      ryujin_hip_time_step_fn with a callback that returns an array prepared beforehand: the wait for
                    tau, the ctypes round trip, the permutation and the copy over PCIe WITHOUT the numpy evaluation
     none           ryujin_hip_time_step_n with the Dirichlet data of the previous call kept: no time dependence at
                    all, the floor
   plus the numpy callback alone (three calls per step). `--passes` passes of `--steps` steps per driver; the figure
   is the median pass with min - max.
2. initial_values_interpolate on a 1581 x 1581 mesh (2.5 M points) against the numpy evaluation followed by
   state_upload of the same state: device events for the kernel, wall clock for both.
3. `--trace-target`: nothing but 200 steps of time_step_iv on vortex-256, to be run under
   `rocprofv3 --kernel-trace --stats -- python scripts/initial_values_timing.py --trace-target` for the Dirichlet
   kernel's own time (no counters are collected in that run).
4. `--function-state`: the expression-defined "function" state (ryujin_hip_initial_values_configure_function) with
   the isentropic vortex written as expressions, against the built-in state, the drivers alternating in one process:
   prepare_state_vector_iv per call on the 256 x 256 mesh (device events over 200 calls; the Dirichlet kernel is the
   only kernel of the call that differs), ERK33 wall clock per step there (iv function, iv built-in, fn numpy), and
   interpolate of 2.5 M points (device events). Only this part runs; profiles/initial_values_function_timing.md.
Usage: initial_values_timing.py [--steps 40] [--passes 5] [--warmup 10] [--skip-large] [--function-state]
(prints markdown)"""
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
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--skip-large", action="store_true")
ap.add_argument("--trace-target", action="store_true")
ap.add_argument("--function-state", action="store_true")
args = ap.parse_args()
lib = capi.load_hip()


def params(equation, dim, **edits):
    p = capi.Params()
    lib.ryujin_hip_default_params(C.byref(p), equation, dim)
    for k, v in edits.items():
        setattr(p, k, v)
    return p


def leblanc():
    off = offline.SyntheticOffline(offline.MeshSpec(1, (1600,), (0.0,), (1.0,),
                                                    (capi.BC_DIRICHLET, capi.BC_DIRICHLET)))
    m = HyperbolicModule(off, params(capi.EQ_EULER, 1, gamma=1.66666666666667, limiter_relaxation_factor=8.0),
                         backend="hip")
    m.initial_values_configure("leblanc", position=(0.326732673267,))
    return off, m, 0.1, lambda x, t: ist.euler_leblanc(x, t, position=0.326732673267)


def vortex(n):
    def make():
        off = offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
        m = HyperbolicModule(off, params(capi.EQ_EULER, 2), backend="hip")
        m.initial_values_configure("isentropic vortex", direction=(1.0, 1.0), position=(-1.0, -1.0), mach_number=1.0,
                                   beta=5.0)
        return off, m, 0.3, lambda x, t: ist.euler_isentropic_vortex(x, t)
    return make


def rk_steps(m, state, temps, cfl, n, t0, mode, fn=None):
    t = t0
    for _ in range(n):
        if mode == "iv":
            t += m.time_step("erk 33", state, temps, "device", t=t)
        elif mode == "fn":
            t += m.time_step("erk 33", state, temps, t=t, dirichlet_fn=fn)
        else:
            t += m.time_step("erk 33", state, temps, None)
    lib.ryujin_hip_synchronize(m._ctx)
    return t


def measure_case(label, make):
    off, m, cfl, exact = make()
    m.cfl = cfl
    bpos = off.b_positions
    state = m.new_state_vector()
    m.initial_values_interpolate(state, 0.0)
    temps = [m.new_state_vector() for _ in range(3)]
    cached = exact(bpos, 0.0)
    drivers = [("iv", "iv", None), ("fn numpy", "fn", lambda t: exact(bpos, t)),
               ("fn cached", "fn", lambda t: cached), ("none", "none", None)]
    samples = {k: [] for k, *_ in drivers}
    samples["numpy callback alone, 3 calls"] = []
    t = 0.0
    for p in range(args.passes):
        for key, mode, fn in drivers:
            t = rk_steps(m, state, temps, cfl, args.warmup if p == 0 else 2, t, mode, fn)
            w0 = time.perf_counter()
            t = rk_steps(m, state, temps, cfl, args.steps, t, mode, fn)
            samples[key].append((time.perf_counter() - w0) * 1e3 / args.steps)
        w0 = time.perf_counter()
        for _ in range(args.steps):
            for c in (0.0, 1.0, 2.0):
                exact(bpos, t + c * 1e-3)
        samples["numpy callback alone, 3 calls"].append((time.perf_counter() - w0) * 1e3 / args.steps)
    assert np.isfinite(state.download()).all()
    med = {k: float(np.median(v)) for k, v in samples.items()}
    print(f"\n### {label}: {off.n_owned} gridpoints, {off.n_bdry} boundary map entries, {args.passes} passes x "
          f"{args.steps} steps\n")
    print("| driver | ms per RK step, median pass (min - max) | ratio to iv |")
    print("|---|---|---|")
    for k, v in samples.items():
        print(f"| {k} | {med[k]:.4f} ({min(v):.4f} - {max(v):.4f}) | {med[k] / med['iv']:.2f} |")
    print(f"\nfn numpy / iv = {med['fn numpy'] / med['iv']:.2f}; of the {med['fn numpy'] - med['iv']:.4f} ms the callback "
          f"path costs per step, the numpy evaluation is {med['numpy callback alone, 3 calls']:.4f} ms, the wait for tau "
          f"with the ctypes round trip, the permutation and the copy {med['fn cached'] - med['iv']:.4f} ms "
          f"(fn cached - iv); iv - none = {med['iv'] - med['none']:.4f} ms is what the time dependence costs on the "
          f"device.")
    m.close()
    off.close()


def measure_interpolate():
    n = 1580
    off = offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, params(capi.EQ_EULER, 2), backend="hip")
    m.initial_values_configure("isentropic vortex", direction=(1.0, 1.0), position=(-1.0, -1.0), mach_number=1.0)
    sv = m.new_state_vector()
    pos = off.positions
    dev, wall, host_eval, host_upload = [], [], [], []
    e = C.c_double()
    for p in range(args.passes + 1):
        lib.ryujin_hip_synchronize(m._ctx)
        w0 = time.perf_counter()
        lib.ryujin_hip_event_record(m._ctx, 0)
        m.initial_values_interpolate(sv, 0.25)
        lib.ryujin_hip_event_record(m._ctx, 1)
        assert lib.ryujin_hip_event_elapsed_ms(m._ctx, C.byref(e)) == 0
        w1 = time.perf_counter()
        U = ist.euler_isentropic_vortex(pos, 0.25)
        w2 = time.perf_counter()
        sv.upload(U)
        lib.ryujin_hip_synchronize(m._ctx)
        w3 = time.perf_counter()
        if p > 0:  # the first pass is the warm-up
            dev.append(e.value)
            wall.append((w1 - w0) * 1e3)
            host_eval.append((w2 - w1) * 1e3)
            host_upload.append((w3 - w2) * 1e3)
    f = lambda v: f"{np.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"  # noqa: E731
    total = np.median(host_eval) + np.median(host_upload)
    print(f"\n### interpolate: {off.n_relevant} points, {args.passes} passes\n")
    print("| | ms, median (min - max) |")
    print("|---|---|")
    print(f"| initial_values_interpolate, kernel (device events) | {f(dev)} |")
    print(f"| initial_values_interpolate, wall clock until the events are read | {f(wall)} |")
    print(f"| numpy evaluation | {f(host_eval)} |")
    print(f"| state_upload | {f(host_upload)} |")
    print(f"\nnumpy + upload / interpolate (wall) = {total / np.median(wall):.0f}; the kernel writes "
          f"{off.n_relevant * 32 / 1e6:.0f} MB and reads {off.n_relevant * 16 / 1e6:.0f} MB: "
          f"{off.n_relevant * 48 / (np.median(dev) * 1e-3) / 1e9:.0f} GB/s.")
    m.close()
    off.close()


def vortex_expressions(mach=1.0, beta=5.0, gamma=1.4):
    """ryujin_amd.initial_states.euler_isentropic_vortex_primitive, statement by statement"""
    xb = f"(x - {mach!r} * t)"
    f = f"({beta!r} / (2 * _pi) * exp(0.5 - 0.5 * ({xb} * {xb} + y * y)))"
    T = f"(1 - ({gamma!r} - 1) / (2 * {gamma!r}) * {f} * {f})"
    rho = f"pow({T}, 1 / ({gamma!r} - 1))"
    return [rho, f"{mach!r} - {f} * y", f"{f} * {xb}", f"pow({rho}, {gamma!r})"]


def measure_function_state():
    frame = dict(direction=(1.0, 1.0), position=(-1.0, -1.0))
    configure = {
        "built-in": lambda m: m.initial_values_configure("isentropic vortex", mach_number=1.0, beta=5.0, **frame),
        "function": lambda m: m.initial_values_configure_function(vortex_expressions(), **frame),
    }
    e = C.c_double()

    def events(m, body):
        lib.ryujin_hip_synchronize(m._ctx)
        lib.ryujin_hip_event_record(m._ctx, 0)
        body()
        lib.ryujin_hip_event_record(m._ctx, 1)
        assert lib.ryujin_hip_event_elapsed_ms(m._ctx, C.byref(e)) == 0
        return e.value

    f = lambda v: f"{np.median(v):.4f} ({min(v):.4f} - {max(v):.4f})"  # noqa: E731

    # a. prepare_state_vector_iv per call, b. ERK33 per step: vortex-256
    off = offline.SyntheticOffline(offline.rectangle_2d(256, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, params(capi.EQ_EULER, 2), backend="hip")
    m.cfl = 0.3
    configure["built-in"](m)
    state = m.new_state_vector()
    m.initial_values_interpolate(state, 0.0)
    temps = [m.new_state_vector() for _ in range(3)]
    bpos = off.b_positions
    exact = lambda t: ist.euler_isentropic_vortex(bpos, t)  # noqa: E731
    calls = 200
    prepare = {k: [] for k in configure}
    step = {"iv function": [], "iv built-in": [], "fn numpy": []}
    t = 0.0
    for p in range(args.passes + 1):
        for key in configure:
            configure[key](m)
            ms = events(m, lambda: [m.prepare_state_vector(state, t, "device") for _ in range(calls)]) / calls
            t = rk_steps(m, state, temps, 0.3, args.warmup if p == 0 else 2, t, "iv")
            w0 = time.perf_counter()
            t = rk_steps(m, state, temps, 0.3, args.steps, t, "iv")
            wall = (time.perf_counter() - w0) * 1e3 / args.steps
            if p > 0:
                prepare[key].append(ms)
                step["iv " + key].append(wall)
        t = rk_steps(m, state, temps, 0.3, 2, t, "fn", exact)
        w0 = time.perf_counter()
        t = rk_steps(m, state, temps, 0.3, args.steps, t, "fn", exact)
        if p > 0:
            step["fn numpy"].append((time.perf_counter() - w0) * 1e3 / args.steps)
    assert np.isfinite(state.download()).all()
    print(f"\n### function state, vortex-256: {off.n_owned} gridpoints, {off.n_bdry} boundary map entries, "
          f"{args.passes} passes\n")
    print("| | ms, median pass (min - max) |")
    print("|---|---|")
    for key in configure:
        print(f"| prepare_state_vector_iv per call, {key} (device events over {calls} calls) | {f(prepare[key])} |")
    for key, v in step.items():
        print(f"| ERK33 wall clock per step, {key} ({args.steps} steps) | {f(v)} |")
    med = lambda v: float(np.median(v))  # noqa: E731
    print(f"\nDirichlet kernel, function - built-in = "
          f"{(med(prepare['function']) - med(prepare['built-in'])) * 1e3:.2f} us per call; ERK33 step: iv function / "
          f"iv built-in = {med(step['iv function']) / med(step['iv built-in']):.3f}, fn numpy / iv function = "
          f"{med(step['fn numpy']) / med(step['iv function']):.3f}.")
    m.close()
    off.close()

    # c. interpolate, 2.5 M points
    off = offline.SyntheticOffline(offline.rectangle_2d(1580, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, params(capi.EQ_EULER, 2), backend="hip")
    sv = m.new_state_vector()
    dev = {k: [] for k in configure}
    for p in range(args.passes + 1):
        for key in configure:
            configure[key](m)
            ms = events(m, lambda: m.initial_values_interpolate(sv, 0.25))
            if p > 0:
                dev[key].append(ms)
    print(f"\n### function state, interpolate: {off.n_relevant} points, {args.passes} passes\n")
    print("| | ms, median (min - max), device events |")
    print("|---|---|")
    for key in configure:
        print(f"| initial_values_interpolate, {key} | {f(dev[key])} |")
    print(f"\nfunction / built-in = {med(dev['function']) / med(dev['built-in']):.2f}.")
    m.close()
    off.close()


if args.function_state:
    print(f"<!-- scripts/initial_values_timing.py --function-state --steps {args.steps} --passes {args.passes} "
          f"--warmup {args.warmup} -->")
    measure_function_state()
    sys.exit(0)

if args.trace_target:
    off, m, cfl, _ = vortex(256)()
    m.cfl = cfl
    state = m.new_state_vector()
    m.initial_values_interpolate(state, 0.0)
    rk_steps(m, state, [m.new_state_vector() for _ in range(3)], cfl, 200, 0.0, "iv")
    m.close()
    sys.exit(0)

print(f"<!-- scripts/initial_values_timing.py --steps {args.steps} --passes {args.passes} --warmup {args.warmup} -->")
measure_case("leblanc-1d", leblanc)
measure_case("vortex-256", vortex(256))
if not args.skip_large:
    measure_case("vortex-1024", vortex(1024))
measure_interpolate()
