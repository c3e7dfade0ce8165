"""Worker of the error-norms RCCL leg on a ONE-GPU box (tests/test_gpu_error_norms.py): one process per rank on device
0, tests/cpp/librccl_stub.so LD_PRELOADed in front of RCCL as in tests/test_rccl_stub.py, so that the library's own
ncclAllReduce of the integrals (sum) and of the nodal maxima (max) runs. Rank and world size come from the
environment, the unique id and the results go through files.

usage: error_norms_rccl_worker.py <out prefix> <cells per unit>      (every rank stores <prefix>.rank<r>.npz)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from quantities_rccl_worker import partition_state  # noqa: E402
from rccl_rendezvous import join_ranks  # noqa: E402
from ryujin_amd import HyperbolicModule, capi, error_norms, offline  # noqa: E402

X_CUT = 1.2   # the cells whose lower corner has x < X_CUT -- none of them on the last of three ranks
X_ALL = 1e30  # every cell


def state(positions):
    return partition_state(positions, 0)


def analytic(positions):
    """a second smooth state that differs across the x-slabs; every component has a non-zero norm"""
    return partition_state(positions, 1)


def select_cells(off, x_cut):
    cells = off.cells
    return np.ascontiguousarray(cells[off.positions[cells[:, 0].astype(np.int64), 0] < x_cut])


def main():
    out_prefix, cells_per_unit = sys.argv[1], int(sys.argv[2])
    lib, comm, rank, world = join_ranks()
    off = offline.SyntheticOffline(offline.mach3_step_2d(cells_per_unit, n_ranks=world, rank=rank))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm, device=0)
    cells = select_cells(off, X_ALL)
    shape, weights = error_norms.q1_tables(2)
    m.error_norms_configure(cells, shape, np.full(len(cells), off.cell_measure), weights)
    sv, av = m.new_state_vector(state(off.positions)), m.new_state_vector(analytic(off.positions))
    before = m.exchange_info()
    out_n, detail_n = m.error_norms_compute(sv, av, None, True)
    out_p, detail_p = m.error_norms_compute(sv, av, None, False)
    after = m.exchange_info()
    assert after["n_allreduces"] == before["n_allreduces"] + 2  # one reduction over the ranks per call
    np.savez(f"{out_prefix}.rank{rank}.npz", cells=cells, out_normalized=np.array(out_n), detail_normalized=detail_n,
             out_plain=np.array(out_p), detail_plain=detail_p)
    m.close()
    lib.ryujin_hip_comm_destroy(comm)


if __name__ == "__main__":
    main()
