"""The reduction of a few doubles over the ranks of the in-process transport on the CPU
(ryujin_amd/csrc/rank_reduce.hpp): the fold that the postprocessor, Quantities, the error norms and
ryujin_hip_state_integrals share, and the rendezvous of the rank threads around it -- the one piece of the host runtime
in which threads share memory without a stream ordering it. Host logic only: no GPU, no HIP runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "rank_reduce_cases")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "rank_reduce_cases.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src, "-o", BIN], check=True)
    return BIN


def _run(checker, mode):
    out = subprocess.run([checker, mode], capture_output=True, text=True, timeout=60)  # a lost wake-up fails, not hangs
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_fold_matches_the_serial_loop_bit_for_bit(checker):
    """{3, Sum}, {8, Max}{8, Min} and {20, Sum}{10, Max} over 1, 2, 3 and 8 ranks against the loop the call sites had:
    sums from +0. in rank order (-0. on every rank gives +0.), maxima and minima from rank 0's value (of +0. and -0. the
    one of rank 0 stays)"""
    _run(checker, "fold")


def test_three_threads_through_500_consecutive_reductions(checker):
    """every thread gets the serial fold's bits in every round: no scratch row is overwritten before a slow rank has
    read it, whichever layout follows which"""
    _run(checker, "rendezvous")


def test_abort_releases_the_ranks_that_wait(checker):
    """two ranks wait in reduce(), a third thread awaits a counter, the last rank calls abort() instead of joining them:
    all three waits end with RankGroupAborted (status RYUJIN_ERR_COMM in the library) and its message"""
    _run(checker, "abort")
