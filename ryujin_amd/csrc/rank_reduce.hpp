// The host half of the in-process transport (LocalGroup in ryujin_hip.hip): the rendezvous of the rank threads and the
// one reduction of a few doubles over the ranks that the postprocessor, Quantities, the error norms and
// ryujin_hip_state_integrals share. Host standard library only -- no HIP, no context -- so that the one piece of
// threaded host code that is not stream ordered can be checked on a CPU (tests/cpp/rank_reduce_cases.cc).
#ifndef RYUJIN_HIP_RANK_REDUCE_HPP
#define RYUJIN_HIP_RANK_REDUCE_HPP

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <initializer_list>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace ryujin_hip
{
  enum class RankReduceOp { Sum, Max, Min };

  /* `count` consecutive doubles reduced with `op`; a row is a sequence of segments */
  struct RankReduceSegment {
    int count;
    RankReduceOp op;
  };

  constexpr int kRankReduceMaxValues = 32; /* the longest row (the error norms: 20 sums and 10 maxima) */

  /* a wait ended because another rank of the group failed (HostRendezvous::abort); status RYUJIN_ERR_COMM */
  struct RankGroupAborted : std::runtime_error {
    RankGroupAborted()
        : std::runtime_error("in-process transport: another rank of the group failed")
    {
    }
  };

  /* out[q] = the rows' entries q of ranks 0, 1, ..., n_ranks - 1 folded in that order, the same on every rank: a sum
   * starts from +0. (so that -0. on every rank gives +0.), a maximum or minimum from the value of rank 0. `out` is
   * no row of `rows`. */
  inline void rank_reduce_fold(const double *rows, const int n_ranks, const int stride,
                               std::initializer_list<RankReduceSegment> segments, double *out)
  {
    int q = 0;
    for (const RankReduceSegment &s : segments)
      for (const int end = q + s.count; q < end; ++q) {
        double v = s.op == RankReduceOp::Sum ? 0. : rows[q];
        for (int r = s.op == RankReduceOp::Sum ? 0 : 1; r < n_ranks; ++r) {
          const double w = rows[(size_t)r * stride + q];
          v = s.op == RankReduceOp::Sum ? v + w : (s.op == RankReduceOp::Max ? std::max(v, w) : std::min(v, w));
        }
        out[q] = v;
      }
  }

  struct HostRendezvous {
    int n_ranks;
    std::mutex mtx;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long generation = 0;
    bool aborted = false;        /* a rank failed: the others must not wait for it */
    std::vector<double> scratch; /* [n_ranks][kRankReduceMaxValues] rows of reduce() */

    explicit HostRendezvous(int n)
        : n_ranks(n)
        , scratch((size_t)n * kRankReduceMaxValues, 0.)
    {
    }

    /* publish / await a generation counter */
    void publish(std::vector<unsigned long> &counter, int rank, unsigned long value)
    {
      {
        std::lock_guard<std::mutex> lock(mtx);
        counter[rank] = value;
      }
      cv.notify_all();
    }
    void await(const std::vector<unsigned long> &counter, int rank, unsigned long value)
    {
      std::unique_lock<std::mutex> lock(mtx);
      cv.wait(lock, [&] { return aborted || counter[rank] >= value; });
      if (aborted && counter[rank] < value)
        throw RankGroupAborted();
    }
    void abort()
    {
      {
        std::lock_guard<std::mutex> lock(mtx);
        aborted = true;
      }
      cv.notify_all();
    }

    void barrier()
    {
      std::unique_lock<std::mutex> lock(mtx);
      const unsigned long gen = generation;
      if (++arrived == n_ranks) {
        arrived = 0;
        ++generation;
        cv.notify_all();
      } else {
        cv.wait(lock, [&] { return aborted || generation != gen; });
        if (aborted && generation == gen)
          throw RankGroupAborted();
      }
    }

    /* values[0 .. n) of every rank -> their fold (rank_reduce_fold) on every rank; n is the length of the segments.
     * Every rank of the group calls it with the same segments. The rows are written and read outside the mutex: the
     * first barrier orders every write before every read, the second every read before the writes of the next call. */
    void reduce(const int rank, double *values, const int n, std::initializer_list<RankReduceSegment> segments)
    {
      int length = 0;
      for (const RankReduceSegment &s : segments)
        length += s.count;
      if (n != length || n > kRankReduceMaxValues)
        throw std::invalid_argument("rank reduction: the segments do not cover the row");
      std::copy(values, values + n, scratch.begin() + (size_t)rank * kRankReduceMaxValues);
      barrier();
      rank_reduce_fold(scratch.data(), n_ranks, kRankReduceMaxValues, segments, values);
      barrier();
    }
  };
} // namespace ryujin_hip

#endif
