"""How a worker process of a one-GPU RCCL leg joins its ranks (tests/test_rccl_stub.launch starts them with
tests/cpp/librccl_stub.so LD_PRELOADed in front of RCCL): rank and world size from the environment, the unique id
through a file in $RYUJIN_RCCL_STUB_DIR, every rank on device 0."""
import ctypes as C
import os
import time

from ryujin_amd import capi


def join_ranks():
    """Returns (lib, comm, rank, world); the caller ends with lib.ryujin_hip_comm_destroy(comm)."""
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    capi.load_synth()
    lib = capi.load_hip()
    # the double is what the library's RCCL calls bind to (LD_PRELOAD): RCCL proper would refuse ranks that share a device
    err = C.CDLL(None).ncclGetErrorString
    err.restype = C.c_char_p
    assert b"rccl stub" in err(4), "tests/cpp/librccl_stub.so is not in front of librccl.so"
    uid = C.create_string_buffer(capi.UNIQUE_ID_BYTES)
    uid_file = os.path.join(os.environ["RYUJIN_RCCL_STUB_DIR"], "unique_id")
    if rank == 0:
        assert lib.ryujin_hip_comm_unique_id(uid) == 0, lib.ryujin_hip_last_error()
        with open(uid_file + ".tmp", "wb") as f:
            f.write(uid.raw)
        os.rename(uid_file + ".tmp", uid_file)
    else:
        while not os.path.exists(uid_file):
            time.sleep(0.01)
        uid = C.create_string_buffer(open(uid_file, "rb").read(), capi.UNIQUE_ID_BYTES)
    comm = C.c_void_p()
    assert lib.ryujin_hip_comm_init(C.byref(comm), uid, rank, world, 0) == 0, lib.ryujin_hip_last_error()
    return lib, comm, rank, world
