#!/usr/bin/env python3
"""What one output cycle of the device-resident VTUOutput costs, measured in ONE process per mesh, after warm-up.

Setting: the 3-D radial-contrast mesh of `bench.py --workload sedov3d` (201^3 = 8.12 M gridpoints unless --size is
given) and the 2-D forward-facing-step mesh of `bench.py` (2.5 M gridpoints); the state is the workload's initial
state (the values do not enter the cost). Quantities: the conserved state and the pressure. Two manifold sets per mesh,
configured one after the other in the same process and context: a plane (a line in 2-D) and a sphere (a circle).
  configure  ryujin_hip_output_configure: wall clock (it uploads the positions and the cells, evaluates the level sets,
             compacts, and ends synchronised), --repeat times, median and range
  (a)        output_extract with level sets, Float32
  (b)        output_extract of the full field, Float32
             both: device events around --calls calls (the call returns the values, so every call ends with the copy
             to the host and a stream synchronisation: the event time contains that round trip) and the wall clock,
             three passes, the median pass with the range of the passes
  (c)        the way it is done without this feature: StateVector.download() -- all of U in double precision -- then
             numpy: the pressure, the gather at the selected nodes, the conversion to Float32 (c1); and, once per
             configuration, the numpy selection of the cut cells and their nodes from the level-set values (c2)
Usage: vtu_output_timing.py [--size N] [--calls 10] [--warmup 3] [--repeat 3] [--skip-3d] [--skip-2d]
(prints markdown)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ryujin_amd import HyperbolicModule, capi, offline  # noqa: E402
from ryujin_amd.workloads import benchmark_workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=0, help="cells per direction of the 3-D mesh (default: the workload's)")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--skip-3d", action="store_true")
ap.add_argument("--skip-2d", action="store_true")
args = ap.parse_args()
lib = capi.load_hip()
EPS = np.finfo(np.float64).eps


def timed(ctx, fn, calls):
    """(median device ms, min, max, median wall ms) per call over three passes"""
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


def wall_ms(fn, repeat):
    t = []
    for _ in range(repeat):
        w0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - w0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def numpy_selection(cells, F):
    """the cell filter of vtu_output.template.h:167-188 and the node list, with numpy"""
    f = F[:, cells]
    selected = ((f >= -100.0 * EPS).any(axis=2) & (f <= 100.0 * EPS).any(axis=2)).any(axis=0)
    cell_ids = np.flatnonzero(selected)
    flags = np.zeros(F.shape[1], dtype=bool)
    flags[cells[cell_ids].reshape(-1)] = True
    return cell_ids, np.flatnonzero(flags)


def run(key, size, manifold_sets):
    wl = benchmark_workload(key, size=size) if size else benchmark_workload(key)
    print(f"\n(setting up {key} ...)", flush=True)
    w0 = time.perf_counter()
    off = offline.SyntheticOffline(wl.make_spec(wl.resolution, 1, 0))
    dim = off.dim
    m = HyperbolicModule(off, equation=wl.equation, backend="hip")
    ctx = m._ctx
    positions = np.ascontiguousarray(off.positions)
    cells = np.ascontiguousarray(off.cells, dtype=np.uint32)
    state = m.new_state_vector(wl.U0_fn(positions))
    names = [*capi.output_names(wl.equation, dim)["conserved"], "p"]
    gamma = m.params.gamma
    print(f"\n### {wl.name}: {off.n_relevant} gridpoints, {len(cells)} cells, quantities {names} "
          f"(set-up {time.perf_counter() - w0:.0f} s)\n")
    print("| manifold | cells cut | nodes | configure [ms] | (a) level sets, dev / wall [ms] | "
          "(b) full Float32, dev / wall [ms] | (c1) download + numpy [ms] | (c2) numpy selection [ms] | "
          "(c1) / (a) wall |")
    print("|---|---|---|---|---|---|---|---|---|")
    full = None
    for label, manifolds in manifold_sets:
        cfg = wall_ms(lambda: m.output_configure(names, cells, manifolds, positions), args.repeat)
        n_cells, n_nodes = m.output_info()
        _, node_ids, _ = m.output_selection()
        for _ in range(args.warmup):
            m.output_extract(state, True, "float32")
            m.output_extract(state, False, "float32")
        a = timed(ctx, lambda: m.output_extract(state, True, "float32"), args.calls)
        if full is None:
            full = timed(ctx, lambda: m.output_extract(state, False, "float32"), max(2, args.calls // 3))

        def host_path():
            U = state.download()
            sel = U[node_ids]
            m2 = (sel[:, 1:1 + dim] ** 2).sum(axis=1)
            p = (gamma - 1.0) * (sel[:, 1 + dim] - 0.5 * m2 / sel[:, 0])
            return np.concatenate([sel.T, p[None]]).astype(np.float32)

        host = host_path()
        device = m.output_extract(state, True, "float32")
        assert host.shape == device.shape and np.allclose(host, device, rtol=1e-5, atol=1e-6, equal_nan=True)
        c1 = wall_ms(host_path, args.repeat)
        F = np.stack([m.output_levelset_values(q) for q in range(len(manifolds))])
        c2 = wall_ms(lambda: numpy_selection(cells, F), 1)
        assert np.array_equal(numpy_selection(cells, F)[1], node_ids)
        print(f"| {label}: `{'`, `'.join(manifolds)}` | {n_cells} | {n_nodes} | {cfg[0]:.1f} ({cfg[1]:.1f} .. {cfg[2]:.1f}) "
              f"| {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) / {a[3]:.3f} | {full[0]:.2f} ({full[1]:.2f} .. {full[2]:.2f}) / "
              f"{full[3]:.2f} | {c1[0]:.1f} ({c1[1]:.1f} .. {c1[2]:.1f}) | {c2[0]:.0f} | {c1[0] / a[3]:.0f} x |",
              flush=True)
    m.close()


print(f"# VTUOutput timing ({lib.ryujin_hip_version().decode()}; calls {args.calls}, warm-up {args.warmup}, "
      f"repeat {args.repeat})")
if not args.skip_3d:
    run("sedov3d", args.size, [("plane", ["x - 0.013"]), ("sphere", ["x*x + y*y + z*z - 0.25"])])
if not args.skip_2d:
    run("step2d", 0, [("line", ["x - 1.2013"]), ("circle", ["(x - 1.5)*(x - 1.5) + (y - 0.5)*(y - 0.5) - 0.09"])])
