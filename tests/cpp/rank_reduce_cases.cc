// CPU check of the reduction over the ranks of the in-process transport (ryujin_amd/csrc/rank_reduce.hpp).
//   rank_reduce_cases fold         rank_reduce_fold against a serial loop written out here, bit for bit: the three layouts
//                                  in use, 1, 2, 3 and 8 ranks, and the signed zeros
//   rank_reduce_cases rendezvous   3 threads through 500 consecutive HostRendezvous::reduce calls, cycling through the
//                                  layouts: every thread gets the serial fold's bits in every round
//   rank_reduce_cases abort        two threads wait in reduce, the third calls abort() instead: both return with
//                                  RankGroupAborted, and so does a thread that awaits a counter nobody publishes
// Exit status 0 and "ok", or one line per failure and status 1.
// (test infrastructure; built by tests/test_rank_reduce.py)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rank_reduce.hpp"

using namespace ryujin_hip;
using Op = RankReduceOp;

namespace
{
  constexpr int kLayouts = 3;
  /* the rows of ryujin_hip_state_integrals (K = 3; Quantities: 1 + 2 K), of the postprocessor (kPostprocessMaxQuantities
   * maxima and minima) and of the error norms (kErrorNormsSums sums, 2 kErrorNormsMaxComponents maxima) */
  constexpr int kLength[kLayouts] = {3, 16, 30};

  Op op_of(const int layout, const int q)
  {
    if (layout == 1)
      return q < 8 ? Op::Max : Op::Min;
    return layout == 0 || q < 20 ? Op::Sum : Op::Max;
  }

  void fold(const int layout, const double *rows, const int n_ranks, const int stride, double *out)
  {
    if (layout == 0)
      rank_reduce_fold(rows, n_ranks, stride, {{3, Op::Sum}}, out);
    else if (layout == 1)
      rank_reduce_fold(rows, n_ranks, stride, {{8, Op::Max}, {8, Op::Min}}, out);
    else
      rank_reduce_fold(rows, n_ranks, stride, {{20, Op::Sum}, {10, Op::Max}}, out);
  }

  void reduce(HostRendezvous &g, const int layout, const int rank, double *values)
  {
    if (layout == 0)
      g.reduce(rank, values, 3, {{3, Op::Sum}});
    else if (layout == 1)
      g.reduce(rank, values, 16, {{8, Op::Max}, {8, Op::Min}});
    else
      g.reduce(rank, values, 30, {{20, Op::Sum}, {10, Op::Max}});
  }

  /* what the four call sites computed before they shared the header */
  void serial(const int layout, const double *rows, const int n_ranks, const int stride, double *out)
  {
    for (int q = 0; q < kLength[layout]; ++q) {
      double v;
      if (op_of(layout, q) == Op::Sum) {
        v = 0.;
        for (int r = 0; r < n_ranks; ++r)
          v += rows[r * stride + q];
      } else {
        v = rows[q];
        for (int r = 1; r < n_ranks; ++r) {
          const double w = rows[r * stride + q];
          v = op_of(layout, q) == Op::Max ? std::max(v, w) : std::min(v, w);
        }
      }
      out[q] = v;
    }
  }

  /* a double of either sign over twelve decades that depends on (rank, round, q): the order of a sum matters */
  double value(const int rank, const int round, const int q)
  {
    uint64_t z = ((uint64_t)rank << 40) + ((uint64_t)round << 16) + (uint64_t)q + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    double v = (double)(z >> 11) / (double)(1ull << 53) - 0.5;
    for (unsigned k = (z & 0xf) % 12; k > 0; --k)
      v *= 10.;
    return v;
  }

  int failures = 0;

  void expect(const bool ok, const std::string &what)
  {
    if (!ok) {
      ++failures;
      std::printf("FAILED: %s\n", what.c_str());
    }
  }

  bool same_bits(const double *a, const double *b, const int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

  void fold_cases()
  {
    for (const int n_ranks : {1, 2, 3, 8})
      for (int layout = 0; layout < kLayouts; ++layout)
        for (const int stride : {kLength[layout], kRankReduceMaxValues}) {
          std::vector<double> rows((size_t)n_ranks * stride, 7.);
          for (int r = 0; r < n_ranks; ++r)
            for (int q = 0; q < kLength[layout]; ++q)
              rows[r * stride + q] = value(r, n_ranks, q);
          double got[kRankReduceMaxValues], want[kRankReduceMaxValues];
          fold(layout, rows.data(), n_ranks, stride, got);
          serial(layout, rows.data(), n_ranks, stride, want);
          expect(same_bits(got, want, kLength[layout]), "fold: layout " + std::to_string(layout) + ", " +
                                                            std::to_string(n_ranks) + " ranks, stride " +
                                                            std::to_string(stride));
        }

    const double plus = 0., minus = -0.;
    for (const int n_ranks : {1, 2, 3, 8}) {
      /* -0. on every rank: the sum is +0. (Quantities, state_integrals), the maximum and minimum -0. */
      std::vector<double> rows((size_t)n_ranks * kRankReduceMaxValues, minus);
      double got[kRankReduceMaxValues], want[kRankReduceMaxValues];
      for (int layout = 0; layout < kLayouts; ++layout) {
        fold(layout, rows.data(), n_ranks, kRankReduceMaxValues, got);
        serial(layout, rows.data(), n_ranks, kRankReduceMaxValues, want);
        expect(same_bits(got, want, kLength[layout]), "fold of -0.: layout " + std::to_string(layout));
        for (int q = 0; q < kLength[layout]; ++q)
          expect(same_bits(&got[q], op_of(layout, q) == Op::Sum ? &plus : &minus, 1),
                 "-0. on " + std::to_string(n_ranks) + " ranks: layout " + std::to_string(layout) + ", entry " +
                     std::to_string(q));
      }
    }
    /* +0. and -0. in a maximum and a minimum: neither is less than the other, the value of rank 0 stays */
    for (const bool minus_first : {false, true}) {
      std::vector<double> rows(3 * 16);
      for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 16; ++q)
          rows[r * 16 + q] = (r == 0) == minus_first ? minus : plus;
      double got[16], want[16];
      fold(1, rows.data(), 3, 16, got);
      serial(1, rows.data(), 3, 16, want);
      expect(same_bits(got, want, 16), "fold of signed zeros");
      for (int q = 0; q < 16; ++q)
        expect(same_bits(&got[q], minus_first ? &minus : &plus, 1), "signed zeros: entry " + std::to_string(q));
    }

    /* segments that do not cover the row are refused before anything is written */
    HostRendezvous alone(1);
    double v[4] = {1., 2., 3., 4.};
    bool refused = false;
    try {
      alone.reduce(0, v, 4, {{3, Op::Sum}});
    } catch (const std::invalid_argument &) {
      refused = true;
    }
    expect(refused, "reduce with n != length of the segments");
    alone.reduce(0, v, 3, {{3, Op::Sum}});
    expect(v[0] == 1. && v[1] == 2. && v[2] == 3. && v[3] == 4., "reduce over one rank");
  }

  void rendezvous_cases()
  {
    constexpr int n_ranks = 3, rounds = 500;
    HostRendezvous g(n_ranks);
    std::atomic<int> mismatches{0};
    std::vector<std::thread> threads;
    for (int rank = 0; rank < n_ranks; ++rank)
      threads.emplace_back([&, rank] {
        for (int round = 0; round < rounds; ++round) {
          const int layout = round % kLayouts, n = kLength[layout];
          double rows[n_ranks * kRankReduceMaxValues], want[kRankReduceMaxValues];
          for (int r = 0; r < n_ranks; ++r)
            for (int q = 0; q < n; ++q)
              rows[r * kRankReduceMaxValues + q] = value(r, round, q);
          serial(layout, rows, n_ranks, kRankReduceMaxValues, want);
          double *mine = rows + rank * kRankReduceMaxValues;
          reduce(g, layout, rank, mine);
          if (!same_bits(mine, want, n))
            ++mismatches;
        }
      });
    for (auto &t : threads)
      t.join();
    expect(mismatches == 0, std::to_string(mismatches.load()) + " of " + std::to_string(n_ranks * rounds) +
                                " reductions differ from the serial fold");
  }

  void abort_cases()
  {
    HostRendezvous g(3);
    std::atomic<int> aborted{0}, other{0};
    std::vector<unsigned long> counter(3, 0);
    std::vector<std::thread> threads;
    for (int rank = 0; rank < 2; ++rank)
      threads.emplace_back([&, rank] {
        double values[3] = {1., 2., 3.};
        try {
          reduce(g, 0, rank, values);
          ++other;
        } catch (const RankGroupAborted &) {
          ++aborted;
        } catch (...) {
          ++other;
        }
      });
    threads.emplace_back([&] {
      try {
        g.await(counter, 2, 1);
        ++other;
      } catch (const RankGroupAborted &) {
        ++aborted;
      } catch (...) {
        ++other;
      }
    });
    for (;;) { /* until both ranks wait in the first barrier of reduce */
      std::unique_lock<std::mutex> lock(g.mtx);
      if (g.arrived == 2)
        break;
      lock.unlock();
      std::this_thread::yield();
    }
    g.abort();
    for (auto &t : threads)
      t.join();
    expect(aborted == 3 && other == 0, "abort(): " + std::to_string(aborted.load()) + " of 3 waits ended with " +
                                           "RankGroupAborted, " + std::to_string(other.load()) + " otherwise");
    expect(std::string(RankGroupAborted().what()) == "in-process transport: another rank of the group failed",
           "the message of RankGroupAborted");
  }
} // namespace

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fold")
    fold_cases();
  else if (mode == "rendezvous")
    rendezvous_cases();
  else if (mode == "abort")
    abort_cases();
  else {
    std::fprintf(stderr, "usage: rank_reduce_cases fold | rendezvous | abort\n");
    return 2;
  }
  if (failures == 0)
    std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
