#!/usr/bin/env python3
"""What the shallow-water states that bring their own bathymetry cost on the device, measured in ONE process, after
warm-up; modelled on scripts/initial_values_library_timing.py. Device events where a kernel is timed, wall clock for the
host's work and for whole Runge-Kutta steps; `--passes` passes (default three), median with min - max.

1. initial_values_interpolate_initial_precomputed on the mesh of the sw2d workload (1825 x 1825 nodes) for `hou test`
   and `three bumps dam break`, against what it replaces: the numpy restatement of the bed at the node positions
   (wall clock) plus the upload of the array (wall clock of a synchronous host-to-device copy of the same size).
2. initial_values_interpolate on the same mesh: the two states against `uniform`.
3. The Dirichlet kernel per call (prepare_state_vector_iv, device events over 200 calls) on a 1-D mesh with Dirichlet
   ends and on the 256 x 256 box: `flow over bump` (transcritical, t = 1: Cardano's formula with pow, acos and two cos)
   against `uniform`.
4. One ERK33 step on the 256 x 256 box with `flow over bump` Dirichlet inflow: time_step_iv against time_step_fn with
   the numpy restatement as callback.
Usage: initial_values_bathymetry_timing.py [--size 1824] [--steps 40] [--passes 3] [--warmup 10]   (prints markdown)"""
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
ap.add_argument("--size", type=int, default=1824)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
lib = capi.load_hip()
e = C.c_double()
SW = capi.EQ_SHALLOW_WATER

# state -> (the tank in the frame of the state, numpy restatement of the bed)
BEDS = {
    "hou test": (((-400.0, -150.0), (500.0, 150.0)), ist.sw_hou_test_bathymetry),
    "three bumps dam break": (((0.0, 0.0), (75.0, 30.0)), ist.sw_three_bumps_dam_break_bathymetry),
}


def fmt(v, digits=4):
    return f"{np.median(v):.{digits}f} ({min(v):.{digits}f} - {max(v):.{digits}f})"


def med(v):
    return float(np.median(v))


def params(dim):
    p = capi.Params()
    lib.ryujin_hip_default_params(C.byref(p), SW, dim)
    p.gravity = 9.81
    return p


def events(m, body):
    lib.ryujin_hip_synchronize(m._ctx)
    lib.ryujin_hip_event_record(m._ctx, 0)
    body()
    lib.ryujin_hip_event_record(m._ctx, 1)
    assert lib.ryujin_hip_event_elapsed_ms(m._ctx, C.byref(e)) == 0
    return e.value


def measure_beds():
    print(f"\n### the bed on the sw2d mesh, {args.passes} passes\n")
    print("| state | nodes | interpolate_initial_precomputed, ms, device events | GB/s (24 B per node) | numpy restatement, "
          "ms, wall | upload of the array, ms, wall | (numpy + upload) / device |")
    print("|---|---|---|---|---|---|---|")
    rows = {}
    for name, ((lower, upper), restatement) in BEDS.items():
        off = offline.SyntheticOffline(offline.rectangle_2d(args.size, lower, upper, bc=capi.BC_SLIP))
        m = HyperbolicModule(off, params(2), backend="hip")
        sv = m.new_state_vector()
        dev, host, upload = [], [], []
        interp = {"uniform": [], name: []}
        for p in range(args.passes + 1):
            m.initial_values_configure(name)
            ms = events(m, m.initial_values_interpolate_initial_precomputed)
            w0 = time.perf_counter()
            Z = restatement(off.positions)
            w1 = time.perf_counter()
            # the upload this replaces: one synchronous copy of n_relevant doubles (a state vector's upload, scaled)
            U = np.zeros((off.n_relevant, m.k))
            U[:, 0] = Z
            w2 = time.perf_counter()
            sv.upload(U)
            lib.ryujin_hip_synchronize(m._ctx)
            w3 = time.perf_counter()
            for key in interp:
                if key == "uniform":
                    m.initial_values_configure("uniform", primitive_state=(1.0, 0.5))
                else:
                    m.initial_values_configure(name)
                t_ms = events(m, lambda: m.initial_values_interpolate(sv, 0.0))
                if p > 0:
                    interp[key].append(t_ms)
            if p > 0:  # the first pass is the warm-up
                dev.append(ms)
                host.append((w1 - w0) * 1e3)
                upload.append((w3 - w2) * 1e3 / m.k)
        m.initial_values_configure(name)
        m.initial_values_interpolate_initial_precomputed()
        assert np.array_equal(m.initial_precomputed(), Z) or np.abs(m.initial_precomputed() - Z).max() < 1e-12
        print(f"| {name} | {off.n_relevant} | {fmt(dev)} | {off.n_relevant * 24 / (med(dev) * 1e-3) / 1e9:.0f} | "
              f"{fmt(host, 1)} | {fmt(upload, 2)} | {(med(host) + med(upload)) / med(dev):.0f} |")
        rows[name] = (off.n_relevant, interp)
        m.close()
        off.close()
    print(f"\n### interpolate on the same mesh, {args.passes} passes\n")
    print("| state | ms, median (min - max), device events | ratio to uniform on the same context |")
    print("|---|---|---|")
    for name, (n, interp) in rows.items():
        print(f"| uniform (context of {name}) | {fmt(interp['uniform'])} | 1.00 |")
        print(f"| {name} | {fmt(interp[name])} | {med(interp[name]) / med(interp['uniform']):.2f} |")


def rk_steps(m, state, temps, n, t, fn=None):
    for _ in range(n):
        if fn is None:
            t += m.time_step("erk 33", state, temps, "device", t=t)
        else:
            t += m.time_step("erk 33", state, temps, t=t, dirichlet_fn=fn)
    lib.ryujin_hip_synchronize(m._ctx)
    return t


def bump_numpy(bpos):
    """the numpy restatement of `flow over bump` at the boundary positions, as a callback of time_step_fn"""
    n, dim = bpos.shape

    def fn(t):
        hq, _ = ist.sw_flow_over_bump(bpos, t)
        out = np.zeros((n, dim + 1))
        out[:, :2] = hq
        return out
    return fn


def measure_dirichlet():
    calls = 200
    meshes = {
        "1-D, 4096 cells, Dirichlet ends": offline.SyntheticOffline(offline.MeshSpec(
            1, (4096,), (0.0,), (25.0,), (capi.BC_DIRICHLET, capi.BC_DIRICHLET))),
        "256 x 256 box": offline.SyntheticOffline(offline.rectangle_2d(256, (0.0, 0.0), (25.0, 25.0),
                                                                       bc=capi.BC_DIRICHLET)),
    }
    configure = {"uniform": lambda m: m.initial_values_configure("uniform", primitive_state=(0.4, 0.45)),
                 "flow over bump": lambda m: m.initial_values_configure("flow over bump")}
    print(f"\n### Dirichlet kernel, prepare_state_vector_iv per call (device events over {calls} calls), "
          f"{args.passes} passes\n")
    print("| mesh | boundary map entries | uniform, ms | flow over bump at t = 1, ms | difference, us |")
    print("|---|---|---|---|---|")
    for label, off in meshes.items():
        m = HyperbolicModule(off, params(off.dim), backend="hip")
        state = m.new_state_vector()
        configure["uniform"](m)
        m.initial_values_interpolate(state, 0.0)
        prepare = {k: [] for k in configure}
        for p in range(args.passes + 1):
            for key in prepare:
                configure[key](m)
                ms = events(m, lambda: [m.prepare_state_vector(state, 1.0, "device") for _ in range(calls)]) / calls
                if p > 0:
                    prepare[key].append(ms)
        print(f"| {label} | {off.n_bdry} | {fmt(prepare['uniform'])} | {fmt(prepare['flow over bump'])} | "
              f"{(med(prepare['flow over bump']) - med(prepare['uniform'])) * 1e3:.2f} |")
        if off.dim == 2:
            # 4. ERK33 with flow over bump inflow
            m.cfl = 0.3
            temps = [m.new_state_vector() for _ in range(3)]
            configure["flow over bump"](m)
            m.initial_values_interpolate_initial_precomputed()
            m.initial_values_interpolate(state, 0.0)
            fn = bump_numpy(off.b_positions)
            step = {"iv": [], "fn numpy": []}
            t = 0.0
            for p in range(args.passes + 1):
                for key, callback in (("iv", None), ("fn numpy", fn)):
                    t = rk_steps(m, state, temps, args.warmup if p == 0 else 2, t, callback)
                    w0 = time.perf_counter()
                    t = rk_steps(m, state, temps, args.steps, t, callback)
                    if p > 0:
                        step[key].append((time.perf_counter() - w0) * 1e3 / args.steps)
            assert np.isfinite(state.download()).all()
            print(f"\n### ERK33 step, flow over bump inflow over the device-made bed, 256 x 256 box: {off.n_owned} "
                  f"gridpoints, {args.passes} passes x {args.steps} steps, t = {t:.3f} at the end\n")
            print("| driver | ms per RK step, wall clock, median pass (min - max) |")
            print("|---|---|")
            for key, v in step.items():
                print(f"| {key} | {fmt(v)} |")
            print(f"\nfn numpy / iv = {med(step['fn numpy']) / med(step['iv']):.2f}.")
        m.close()
        off.close()


print(f"<!-- scripts/initial_values_bathymetry_timing.py --size {args.size} --steps {args.steps} "
      f"--passes {args.passes} --warmup {args.warmup} -->")
measure_beds()
measure_dirichlet()
