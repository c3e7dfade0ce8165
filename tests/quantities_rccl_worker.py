"""Worker of the Quantities RCCL leg on a ONE-GPU box (tests/test_gpu_quantities.py): one process per rank on device 0,
tests/cpp/librccl_stub.so LD_PRELOADed in front of RCCL as in tests/test_rccl_stub.py, so that the library's own
ncclAllReduce(sum) of the 1 + 2k weighted sums runs. Rank and world size come from the environment, the unique id and
the results go through files.

usage: quantities_rccl_worker.py <out prefix> <cells per unit>      (every rank stores <prefix>.rank<r>.npz)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rccl_rendezvous import join_ranks  # noqa: E402
from ryujin_amd import HyperbolicModule, capi, offline, quantities  # noqa: E402

TIMES = (0.25, 0.3125, 0.5, 1.0)
X_CUT = 1.2  # the manifold: the interior nodes with x <= X_CUT -- none of them on the last rank
OPTIONS = capi.Q_INSTANTANEOUS | capi.Q_TIME_AVERAGED | capi.Q_SPACE_AVERAGED


def partition_state(positions, s=0):
    """a state that differs across the x-slabs, and its successors s = 1, 2, ... (uploaded, not stepped)"""
    x, y = positions[:, 0], positions[:, 1]
    rho = 1.4 + 0.2 * np.sin(2.0 * x + y + 0.3 * s) + 0.5 * np.exp(-40.0 * ((x - 2.6) ** 2 + (y - 0.6) ** 2))
    u = 3.0 + 0.3 * np.cos(3.0 * y - 0.2 * s) * x
    v = 0.2 * np.sin(2.0 * x) + 0.1 * x * y * (1.0 + s)
    p = 1.0 + 0.1 * np.cos(x - 2.0 * y) + 0.05 * s
    return np.stack([rho, rho * u, rho * v, p / 0.4 + 0.5 * rho * (u * u + v * v)], axis=1)


def cut_level_set(positions):
    return np.where(positions[:, 0] <= X_CUT, 0.0, 1.0)


def select(off):
    lengths = np.diff(off.row_starts.astype(np.int64))
    return quantities.select_interior_points(cut_level_set, off.positions, lengths, off.n_owned)


def main():
    out_prefix, cells = sys.argv[1], int(sys.argv[2])
    lib, comm, rank, world = join_ranks()
    off = offline.SyntheticOffline(offline.mach3_step_2d(cells, n_ranks=world, rank=rank))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm, device=0)
    index = select(off)
    mid = m.quantities_add_manifold(index, off.mi[index], OPTIONS)
    none = m.quantities_add_manifold([], [], capi.Q_SPACE_AVERAGED)  # empty on all ranks
    state = m.new_state_vector()
    before = m.exchange_info()
    for s, t in enumerate(TIMES):
        state.upload(partition_state(off.positions, s))
        m.quantities_accumulate(state, t)
    after = m.exchange_info()
    assert after["n_allreduces"] == before["n_allreduces"] + 2 * len(TIMES)  # one per manifold and call
    averaged, t_begin, t_end = m.quantities_time_averaged(mid)
    np.savez(f"{out_prefix}.rank{rank}.npz", index=index, series=m.quantities_time_series(mid),
             series_none=m.quantities_time_series(none), instantaneous=m.quantities_instantaneous(mid, state, TIMES[-1]),
             averaged=averaged, interval=np.array([t_begin, t_end]))
    m.close()
    lib.ryujin_hip_comm_destroy(comm)


if __name__ == "__main__":
    main()
