#!/usr/bin/env python3
"""What the device-resident compute_error() costs, measured in ONE process, after warm-up.

1. ryujin_hip_error_norms_compute on its own, on the developed state of bench.py's C2 workload (the forward-facing
   step, 2.5 M gridpoints, 4 components; the analytic vector is the uniform inflow state): both JxW forms, device
   events around `--calls` calls (the call returns numbers, so every call ends with a stream synchronisation and a
   copy of 33 doubles: the event time contains that round trip) and the wall clock, three passes, the median pass;
   next to step 5 of the update from the library's own event pairs, same process and context.
   "own bytes" per cell for dofs_per_cell = 4, n_q = 9, n components, padded state width KP:
       16 (indices) + 72 (JxW per point) or 8 (cell measure) + 2 * 8 KP (U and A, every node once -- a node belongs
       to four cells, each node's two padded states are fetched from HBM once and from the cache otherwise)
   plus the nodal kernel's 2 * 8 KP per gridpoint.
2. compute_error() end to end (prepare_state_vector with device Dirichlet data, initial_values_interpolate into the
   scratch vector, compute) on the isentropic vortex on 1580 x 1580 cells (2.5 M gridpoints, a lattice, so that the
   host path exists), wall clock, against the host path it replaces: state download + numpy evaluation of the exact
   solution + norms_2d of tests/test_oracle_golden_verification.py per component.
Usage: error_norms_timing.py [--calls 20] [--warmup 5] [--skip-host]   (prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ryujin_amd import HyperbolicModule, capi, error_norms, offline  # noqa: E402
from ryujin_amd import initial_states as ist  # noqa: E402
from ryujin_amd.workloads import Ssprk33Stages, benchmark_workload, developed_state  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()
lib = capi.load_hip()


def timed(ctx, fn, calls):
    dev, wall = [], []
    for _ in range(3):
        lib.ryujin_hip_synchronize(ctx)
        w0 = time.perf_counter()
        lib.ryujin_hip_event_record(ctx, 0)
        for _ in range(calls):
            fn()
        lib.ryujin_hip_event_record(ctx, 1)
        e = C.c_double()
        assert lib.ryujin_hip_event_elapsed_ms(ctx, C.byref(e)) == 0
        wall.append((time.perf_counter() - w0) * 1e3 / calls)
        dev.append(e.value / calls)
    return float(np.median(dev)), min(dev), max(dev), float(np.median(wall))


def compute_alone():
    wl = benchmark_workload("step2d")
    off = offline.SyntheticOffline(wl.make_spec(wl.resolution, 1, 0))
    U0, _, _ = developed_state(wl, off)
    m = HyperbolicModule(off, equation=wl.equation, backend="hip")
    m.cfl = 0.9
    ctx = m._ctx
    dirichlet = wl.dirichlet_fn(off.b_positions) if (wl.dirichlet_fn is not None and off.n_bdry) else None
    drv = Ssprk33Stages(m, U0, dirichlet)
    for _ in range((wl.develop_updates + 2) // 3):
        drv.rk_step()
    lib.ryujin_hip_set_timers(ctx, 1)
    tmp, n_upd = (C.c_double * 8)(), C.c_uint()
    for _ in range(6):
        drv.update()
    lib.ryujin_hip_get_timers_accum(ctx, tmp, C.byref(n_upd), 1)
    for _ in range(30):
        drv.update()
    lib.ryujin_hip_get_timers_accum(ctx, tmp, C.byref(n_upd), 0)
    step5 = tmp[5] / n_upd.value
    lib.ryujin_hip_set_timers(ctx, 0)
    while drv.stage != 0:
        drv.update()

    analytic = m.new_state_vector(ist.euler_uniform(off.positions))
    shape, weights = error_norms.q1_tables(2)
    cells = off.cells
    kp = (m.k + 1) // 2 * 2
    print(f"\n### compute() alone: C2, {off.n_owned} gridpoints, {len(cells)} cells, {m.k} components; step 5 of the "
          f"update {step5:.4f} ms\n")
    print("| JxW | own bytes / cell + / gridpoint | compute [ms], events (min - max) | wall [ms] | TB/s by own bytes | "
          "compute / step 5 |")
    print("|---|---|---|---|---|---|")
    for label, jxw, w, per_cell_bytes in (("per cell (affine)", np.full(len(cells), off.cell_measure), weights, 8),
                                          ("per point", error_norms.q1_jxw(off.positions, cells), None, 72)):
        m.error_norms_configure(cells, shape, jxw, w)
        fn = lambda: m.error_norms_compute(drv.U, analytic)  # noqa: E731
        for _ in range(args.warmup):
            out = fn()
        ms, lo, hi, wall = timed(ctx, fn, args.calls)
        cell_b, node_b = 16 + per_cell_bytes, 2 * 8 * kp
        total = cell_b * len(cells) + 2 * node_b * off.n_owned  # the cell kernel's nodes once, the nodal kernel's again
        print(f"| {label} | {cell_b} + {2 * node_b} | {ms:.4f} ({lo:.4f} - {hi:.4f}) | {wall:.4f} | "
              f"{total / (ms * 1e-3) / 1e12:.2f} | {ms / step5:.2f} |", flush=True)
        print(f"<!-- consolidated {out[0]} -->", flush=True)
    m.close()
    off.close()


def end_to_end():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    n = 1580
    off = offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m.initial_values_configure("isentropic vortex", direction=(1.0, 1.0), position=(-1.0, -1.0), mach_number=1.0,
                               beta=5.0)
    shape, weights = error_norms.q1_tables(2)
    m.error_norms_configure(off.cells, shape, np.full(off.n_cells, off.cell_measure), weights)
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    temps = [m.new_state_vector() for _ in range(3)]
    t = 0.0
    for _ in range(5):
        t += m.time_step("erk 33", sv, temps, "device", t=t)
    device = []
    for p in range(args.calls + args.warmup):
        lib.ryujin_hip_synchronize(m._ctx)
        w0 = time.perf_counter()
        out, _ = m.compute_error(sv, t)
        if p >= args.warmup:
            device.append((time.perf_counter() - w0) * 1e3)
    print(f"\n### compute_error() end to end: isentropic vortex, {off.n_owned} gridpoints, t = {t:.5f}\n")
    print("| path | ms, median (min - max) |")
    print("|---|---|")
    f = lambda v: f"{np.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"  # noqa: E731
    print(f"| compute_error() on the device (prepare_state_vector + interpolate + compute), wall | {f(device)} |")
    if not args.skip_host:
        from test_oracle_golden_verification import norms_2d
        pos, bpos = off.positions, off.b_positions
        order = np.lexsort((pos[:, 0], pos[:, 1]))
        h = 10.0 / n
        download, total = [], []
        for _ in range(3):
            w0 = time.perf_counter()
            m.prepare_state_vector(sv, t, ist.euler_isentropic_vortex(bpos, t))
            w1 = time.perf_counter()
            U = sv.download()
            download.append((time.perf_counter() - w1) * 1e3)
            A = ist.euler_isentropic_vortex(pos, t)
            linf = l1 = l2 = 0.0
            for c in range(4):
                a = A[order, c].reshape(n + 1, n + 1).T
                e = (U[order, c] - A[order, c]).reshape(n + 1, n + 1).T
                (l1a, l2a), (l1e, l2e) = norms_2d(a, h), norms_2d(e, h)
                linf += np.abs(e).max() / np.abs(a).max()
                l1 += l1e / l1a
                l2 += l2e / l2a
            total.append((time.perf_counter() - w0) * 1e3)
        print(f"| host path: prepare_state_vector + download + numpy exact solution + norms_2d, wall | {f(total)} |")
        print(f"| of which the state download | {f(download)} |")
        print(f"\nhost / device = {np.median(total) / np.median(device):.0f}; download alone / device = "
              f"{np.median(download) / np.median(device):.1f}. Device {out}, host {(linf, l1, l2)}.")
    m.close()
    off.close()


print(f"<!-- scripts/error_norms_timing.py --calls {args.calls} --warmup {args.warmup} -->")
compute_alone()
end_to_end()
