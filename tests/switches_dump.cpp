// Prints Switches::from_env() (csrc/switches.hpp) of this process's environment as one JSON object: "names", the
// M2S_* variables in the order from_env() reads them (reported by from_env() itself), and "values", every member.
// Host code, no HIP: tests/test_switches_cpu.py builds it with the host compiler and runs it under chosen
// environments.
#include <cstdio>
#include <string>
#include <vector>

#include "switches.hpp"

int main() {
  std::vector<std::string> names;
  const m2s::Switches w = m2s::Switches::from_env([&](const char* n) { names.push_back(n); });
  std::printf("{\"names\": [");
  for (size_t i = 0; i < names.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", names[i].c_str());
  std::printf("], \"values\": {");
  bool first = true;
  auto put = [&](const char* k, int v) {
    std::printf("%s\"%s\": %d", first ? "" : ", ", k, v);
    first = false;
  };
#define B(m) put(#m, w.m ? 1 : 0)
#define I(m) put(#m, w.m)
  B(ir_fused), B(ir_ws), B(ir_ws_s2), B(irws_f32), B(stem_fused), B(f8_er), B(se_y8), B(f8_er2), B(er8_x8);
  B(f8_expand), B(f8_s2), B(se_fused), B(er_fused), B(se_sp), B(se_ws), B(er_mrg), B(ir_s2band), B(er_s2_fused);
  B(sews_rev);
  I(irws_min), I(sews_min_cus), I(irws_parts), I(stem_parts), B(sews_half), I(se_ws_cfg), I(se_sp_waves);
  B(lstm_persistent), B(lstm_mid), B(lstm_x3), B(lstm_x3g), I(lstm_small_b), I(lstm_mid_ch);
  B(mrf_fused), B(mrf_halo), B(mrf_pair), B(mrf_chain), B(mrf_pair128), B(f8_mrf64), B(f8_mrf32), B(mrf_batch);
  I(conv.ksplit), I(conv.ksplit_max), I(conv.ksplit_minst), B(conv.bn64), I(conv.stages);
  std::printf("}}\n");
  return 0;
}
