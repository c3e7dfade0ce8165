"""Worker of the postprocessor's RCCL leg on a ONE-GPU box (tests/test_gpu_postprocessor.py): one process per rank on
device 0, tests/cpp/librccl_stub.so LD_PRELOADed in front of RCCL as in tests/test_rccl_stub.py, so that the library's
own ncclSend / ncclRecv ghost exchange and its ncclAllReduce(max) / (min) of the bounds run. Rank and world size come
from the environment, the unique id and the results go through files.

usage: postprocessor_rccl_worker.py <out prefix> <cells per unit>      (every rank stores <prefix>.rank<r>.npz)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rccl_rendezvous import join_ranks  # noqa: E402
from ryujin_amd import HyperbolicModule, capi, offline  # noqa: E402

SCHLIEREN, VORTICITY, BETA = ("rho", "p"), ("v_1",), 10.0


def partition_state(positions):
    """a state that differs across the x-slabs: the strongest gradients sit in the last one"""
    x, y = positions[:, 0], positions[:, 1]
    rho = 1.4 + 0.2 * np.sin(2.0 * x + y) + 0.5 * np.exp(-40.0 * ((x - 2.6) ** 2 + (y - 0.6) ** 2))
    u = 3.0 + 0.3 * np.cos(3.0 * y) * x
    v = 0.2 * np.sin(2.0 * x) + 0.1 * x * y
    p = 1.0 + 0.1 * np.cos(x - 2.0 * y)
    return np.stack([rho, rho * u, rho * v, p / 0.4 + 0.5 * rho * (u * u + v * v)], axis=1)


def main():
    out_prefix, cells = sys.argv[1], int(sys.argv[2])
    lib, comm, rank, world = join_ranks()
    off = offline.SyntheticOffline(offline.mach3_step_2d(cells, n_ranks=world, rank=rank))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm, device=0)
    stale = partition_state(off.positions)
    stale[off.n_owned:] = 0.0  # the ghost range is NOT current: compute() has to exchange it
    state = m.new_state_vector(stale)
    before = m.exchange_info()
    norm = m.postprocess(state, schlieren=SCHLIEREN, vorticity=VORTICITY, beta=BETA)
    raw, bounds, after = m.postprocess_download(raw=True), m.postprocess_bounds(), m.exchange_info()
    assert after["n_exchanges"] == before["n_exchanges"] + 1 and after["n_allreduces"] == before["n_allreduces"] + 1
    names = list(norm)
    np.savez(f"{out_prefix}.rank{rank}.npz", U=state.download(), names=np.array(names),
             norm=np.stack([norm[k] for k in names]), raw=np.stack([raw[k] for k in names]),
             bounds=np.array([bounds[k] for k in names]))
    m.close()
    lib.ryujin_hip_comm_destroy(comm)


if __name__ == "__main__":
    main()
