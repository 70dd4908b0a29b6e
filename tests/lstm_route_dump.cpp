// Prints lstm_plan() (csrc/lstm_route.hpp) for a grid of calls, one JSON line per (dtype, H, B).  Host code, no
// HIP, nothing but the route header: tests/test_lstm_route_cpu.py builds it with the host compiler.
//   lstm_route_dump PERSISTENT MID X3 X3G SMALL_B MID_CH  DTYPE,DTYPE,..  H,H,..  B,B,..
// (the six values as Switches holds them; dtype: the m2s_dtype number)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lstm_route.hpp"

static std::vector<int> ints(const char* s) {
  std::vector<int> v;
  for (const char* p = s; *p;) {
    char* e;
    v.push_back((int)std::strtol(p, &e, 10));
    p = *e ? e + 1 : e;
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  const m2s::LstmSwitches w{std::atoi(argv[1]) != 0, std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0,
                            std::atoi(argv[4]) != 0, std::atoi(argv[5]),      std::atoi(argv[6])};
  const char* const routes[] = {"step", "small", "x3g", "x3", "mid", "persistent"};
  for (int dtype : ints(argv[7]))
    for (int H : ints(argv[8]))
      for (int B : ints(argv[9])) {
        const m2s::LstmPlan p = m2s::lstm_plan(w, dtype, B, H);
        std::printf("{\"dtype\": %d, \"H\": %d, \"B\": %d, \"route\": \"%s\", \"inst\": %d, \"name\": \"%s\", "
                    "\"terms\": %d, \"engine_sync\": %d}\n",
                    dtype, H, B, routes[(int)p.route], p.inst, p.name, p.terms, p.engine_sync ? 1 : 0);
      }
  return 0;
}
