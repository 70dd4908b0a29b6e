// Prints lstm_epoch_rule() (csrc/lstm_route.hpp) as a table, one JSON line per (count, T, capturing): the epoch the
// launch gets, the engine's count after it, whether the buffer is zeroed first.  Host code, no HIP, nothing but the
// route header: tests/test_lstm_epoch_cpu.py builds it with the host compiler and walks event sequences over it.
//   lstm_epoch_dump COUNT_LO COUNT_HI T_MAX      (counts as unsigned 32-bit numbers, both ends included; T = 1..T_MAX)
#include <cstdio>
#include <cstdlib>

#include "lstm_route.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const unsigned long lo = std::strtoul(argv[1], nullptr, 10), hi = std::strtoul(argv[2], nullptr, 10);
  const int tmax = std::atoi(argv[3]);
  if (lo > hi || hi > 0xFFFFFFFFul || tmax < 1) return 2;
  for (unsigned long c = lo; c <= hi; ++c)
    for (int T = 1; T <= tmax; ++T)
      for (int cap = 0; cap < 2; ++cap) {
        const m2s::LstmEpoch e = m2s::lstm_epoch_rule((unsigned)c, T, cap != 0);
        std::printf("{\"count\": %lu, \"T\": %d, \"capturing\": %d, \"ep\": %u, \"new\": %u, \"zero\": %d}\n", c, T, cap, e.ep,
                    e.count, e.zero ? 1 : 0);
      }
  std::printf("{\"wrap\": %u}\n", m2s::LSTM_EPOCH_WRAP);
  return 0;
}
