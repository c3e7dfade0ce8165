#!/usr/bin/env python3
"""Device time of ryujin_hip_quantities_accumulate on the developed state of bench.py's C2 workload (2-D Euler, 2.5 M
gridpoints), next to one SSPRK33 time step measured IN THE SAME PROCESS and context, and next to the way the series was
obtained before: state_download() and a numpy mean on the host per step.

  (a) full-interior `space_averaged`                 40 B per point  (U 32 + weight 8; one contiguous run: no index)
  (b) full-interior `time_averaged space_averaged`  296 B per point  (+ previous values read and written 64 + 64,
                                                                      sums read and written 128)
  (c) the boundary map, `time_averaged space_averaged` (gather path, repeated corner indices)
  (d) all three at once
  step       one ryujin_hip_time_step (SSPRK33: three updates, one host synchronisation)
  step + (a) the same with (a) enqueued after each
  download   state_download() alone, and with the numpy mean of the primitive state and its squares

The variants ALTERNATE: `--passes` passes, in each of them every variant runs `--calls` calls between two device events
(passes x calls >= 200 per figure); the figure is the median pass, with min - max. The host-side baseline is wall
clock. The condition that is checked: what (a) adds to a time step is less than the download alone.
Usage: quantities_timing.py [--calls 40] [--passes 5] [--warmup 10] [--updates N]   (prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryujin_amd import HyperbolicModule, capi, offline, quantities  # noqa: E402
from ryujin_amd.workloads import Ssprk33Stages, benchmark_workload, developed_state  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--updates", type=int, default=0, help="updates on the benchmark mesh (0: the workload's own)")
args = ap.parse_args()
assert args.calls * args.passes >= 200
lib = capi.load_hip()
T, S = capi.Q_TIME_AVERAGED, capi.Q_SPACE_AVERAGED

wl = benchmark_workload("step2d")
off = offline.SyntheticOffline(wl.make_spec(wl.resolution, 1, 0))
U0, _, _ = developed_state(wl, off)
m = HyperbolicModule(off, equation=wl.equation, backend="hip")
m.cfl = 0.9
ctx = m._ctx
dirichlet = wl.dirichlet_fn(off.b_positions) if (wl.dirichlet_fn is not None and off.n_bdry) else None
drv = Ssprk33Stages(m, U0, dirichlet)
for _ in range(((args.updates or wl.develop_updates) + 2) // 3):
    drv.rk_step()

lengths = np.diff(off.row_starts.astype(np.int64))
interior = quantities.select_interior_points(0.0, off.positions, lengths, off.n_owned)
entries = quantities.select_boundary_entries(0.0, off.b_i, off.b_positions, off.n_owned)
w_interior, b_index, b_weight = off.mi[interior], off.b_i[entries], off.b_mass[entries]
clock = [0.0]


def manifolds(which):
    m.quantities_reset()
    if which in ("a", "d"):
        m.quantities_add_manifold(interior, w_interior, S)
    if which in ("b", "d"):
        m.quantities_add_manifold(interior, w_interior, T | S)
    if which in ("c", "d"):
        m.quantities_add_manifold(b_index, b_weight, T | S)


def accumulate():
    clock[0] += 0.125
    m.quantities_accumulate(drv.U, clock[0])


def step_and_accumulate():
    drv.rk_step()
    m.quantities_accumulate(drv.U, drv.t)


def device_ms(fn, calls):
    lib.ryujin_hip_synchronize(ctx)
    lib.ryujin_hip_event_record(ctx, 0)
    for _ in range(calls):
        fn()
    lib.ryujin_hip_event_record(ctx, 1)
    e = C.c_double()
    assert lib.ryujin_hip_event_elapsed_ms(ctx, C.byref(e)) == 0
    return e.value / calls


def download_only():
    return drv.U.download()


def download_and_mean():
    U = drv.U.download()[: off.n_owned]
    rho = U[:, 0]
    v = U[:, 1:3] / rho[:, None]
    p = (m.params.gamma - 1.0) * (U[:, 3] - 0.5 * (U[:, 1] ** 2 + U[:, 2] ** 2) / rho)
    prim = np.column_stack([rho, v, p])
    w = w_interior / w_interior.sum()
    return (w[:, None] * prim).sum(0), (w[:, None] * prim ** 2).sum(0)


def host_ms(fn, calls):
    lib.ryujin_hip_synchronize(ctx)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


variants = [("a", "(a) interior, space_averaged", accumulate, "a", device_ms, args.calls),
            ("b", "(b) interior, time_averaged space_averaged", accumulate, "b", device_ms, args.calls),
            ("c", "(c) boundary map, time_averaged space_averaged", accumulate, "c", device_ms, args.calls),
            ("d", "(d) all three", accumulate, "d", device_ms, args.calls),
            ("step", "time step (SSPRK33), no quantities", drv.rk_step, None, device_ms, args.calls),
            ("step+a", "time step with (a) enqueued after it", step_and_accumulate, "a", device_ms, args.calls),
            ("download", "state_download() alone", download_only, None, host_ms, max(4, args.calls // 10)),
            ("download+mean", "state_download() + numpy mean", download_and_mean, None, host_ms,
             max(4, args.calls // 10))]
samples = {key: [] for key, *_ in variants}
for p in range(args.passes):
    for key, _, fn, which, timer, calls in variants:
        if which is not None:
            manifolds(which)
        else:
            m.quantities_reset()
        for _ in range(args.warmup if p == 0 else 2):
            fn()
        samples[key].append(timer(fn, calls))

med = {k: float(np.median(v)) for k, v in samples.items()}
step = med["step"]
n = len(interior)
model = {"a": 40.0 * n, "b": 296.0 * n}
print(f"<!-- {off.n_owned} gridpoints, {len(b_index)} boundary map entries, {args.passes} passes x {args.calls} calls -->")
print("| variant | ms per call, median pass (min - max) | fraction of a time step | fraction of an update (step / 3) | "
      "GB/s by the byte model |")
print("|---|---|---|---|---|")
for key, label, *_ in variants:
    v = samples[key]
    gbs = f"{model[key] / (med[key] * 1e-3) / 1e9:.0f}" if key in model else ""
    print(f"| {label} | {med[key]:.4f} ({min(v):.4f} - {max(v):.4f}) | {med[key] / step:.3f} | "
          f"{med[key] / (step / 3.0):.3f} | {gbs} |")
added = med["step+a"] - step
spread = max(samples["step"]) - min(samples["step"])
print()
print(f"(a) enqueued after every time step adds {added:.4f} ms ({added / step * 100.0:.2f} % of the step); the run-to-run "
      f"spread of the time step without it in this run is {spread:.4f} ms ({spread / step * 100.0:.2f} %).")
ok = added < med["download"] and med["a"] < med["download"]
print(f"Condition: (a) after every step ({max(added, med['a']):.4f} ms, the larger of the added time and the call alone) "
      f"< state_download() alone ({med['download']:.4f} ms): {'MET' if ok else 'NOT MET'} "
      f"(factor {med['download'] / max(added, med['a'], 1e-9):.0f}).")
m.close()
off.close()
sys.exit(0 if ok else 1)
