// Stand-alone dump of the vocoder's route table (tests/test_voc_route_cpu.py builds and runs it; no GPU needed):
//   voc_route_dump <generator dump> <generator config> <dtype 0..3>
// reads the M2S_* switches from the environment as an engine does, asks voc_pack_wants which copies the packer
// stages, packs the generator with them (the dump and config formats of tests/pack_digest.cpp) and prints one JSON
// line per upsampling stage: every field of the stage's record (csrc/voc_route.hpp) by name ("rb" and "rb_record"
// are empty off the PerResblock route), conv_pre's hand-off,
// and per resblock what voc_pack_wants asked for ("wants") beside what the packed plan holds ("packed"), each as a
// string of f (rb1_fused fragments), h (conv1d_halo fragments) and q (e4m3 rows).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "model.hpp"

namespace {

template <class T>
T get(FILE* f) {
  T v;
  if (std::fread(&v, sizeof(T), 1, f) != 1) {
    std::fprintf(stderr, "voc_route_dump: truncated dump\n");
    std::exit(2);
  }
  return v;
}

struct Dump {
  std::vector<std::string> names;
  std::vector<std::vector<float>> data;
  std::vector<m2s_tensor> tensors;
};

void load(const char* path, Dump& d) {
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "voc_route_dump: cannot open %s\n", path);
    std::exit(2);
  }
  const uint32_t n = get<uint32_t>(f);
  d.names.resize(n);
  d.data.resize(n);
  d.tensors.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    d.names[i].resize(get<uint32_t>(f));
    if (std::fread(&d.names[i][0], 1, d.names[i].size(), f) != d.names[i].size()) std::exit(2);
    m2s_tensor& t = d.tensors[i];
    t.elem = M2S_ELEM_F32;
    t.ndim = (int)get<uint32_t>(f);
    if (t.ndim < 0 || t.ndim > 4) std::exit(2);
    size_t numel = 1;
    for (int k = 0; k < 4; ++k) t.shape[k] = 0;
    for (int k = 0; k < t.ndim; ++k) numel *= (size_t)(t.shape[k] = get<int64_t>(f));
    d.data[i].resize(numel);
    if (numel && std::fread(d.data[i].data(), sizeof(float), numel, f) != numel) std::exit(2);
  }
  std::fclose(f);
  for (uint32_t i = 0; i < n; ++i) {  // after the vectors stopped moving
    d.tensors[i].name = d.names[i].c_str();
    d.tensors[i].data = d.data[i].data();
  }
}

m2s_hifigan_h config(const char* csv) {
  m2s_hifigan_h h{};
  int* out = reinterpret_cast<int*>(&h);
  size_t i = 0;
  for (const char* p = csv; *p && i < sizeof(h) / sizeof(int); ++i) {
    char* end;
    out[i] = (int)std::strtol(p, &end, 10);
    p = *end == ',' ? end + 1 : end;
  }
  if (i != sizeof(h) / sizeof(int)) {
    std::fprintf(stderr, "voc_route_dump: config has %zu of %zu ints\n", i, sizeof(h) / sizeof(int));
    std::exit(2);
  }
  return h;
}

const char* const kMrf[] = {"Pair", "HaloBatched", "GemmBatched", "F8", "PerResblock"};
const char* const kRb[] = {"Convs", "Fused"};

std::string copies(bool f, bool h, bool q) { return std::string(f ? "f" : "") + (h ? "h" : "") + (q ? "q" : ""); }
const char* tf(bool b) { return b ? "true" : "false"; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: voc_route_dump generator.bin config dtype\n");
    return 2;
  }
  try {
    Dump gen;
    load(argv[1], gen);
    const m2s_hifigan_h h = config(argv[2]);
    const int dtype = std::atoi(argv[3]);
    const m2s::StateDict sd = m2s::make_state_dict(gen.tensors.data(), (int)gen.tensors.size());
    const m2s::Switches sw = m2s::Switches::from_env();
    const m2s::VocPackWants wants = m2s::voc_pack_wants(h, dtype, sw);
    const m2s::VocRoute t = m2s::voc_route(h, dtype, sw, wants);
    m2s::Arena ar;
    m2s::VocoderPlan plan;
    m2s::pack_vocoder(sd, h, dtype, wants, ar, plan);
    const int nk = h.n_kernels;
    for (size_t i = 0; i < t.stages.size(); ++i) {
      const m2s::StageRoute& r = t.stages[i];
      std::string rb, rec, want, packed;
      for (int j = 0; j < nk; ++j) {
        const char* sep = j ? ", " : "";
        const m2s::RbWants& w = wants.rbs[i * nk + j];
        const m2s::RB& p = plan.rbs[i * nk + j];
        const size_t np = p.dil.size();
        if (r.mrf == m2s::MrfRoute::PerResblock) {
          rb += std::string(sep) + "\"" + kRb[(int)r.rb[j]] + "\"";
          rec += std::string(sep) + "\"" + r.rb_record[j] + "\"";
        }
        want += std::string(sep) + "\"" + copies(w.frag, w.halo, w.q8) + "\"";
        packed += std::string(sep) + "\"" +
                  copies(p.f1_off.size() == np && p.f2_off.size() == np, p.h1_off.size() == np && p.h2_off.size() == np,
                         p.q1.size() == np && p.q2.size() == np) +
                  "\"";
        // a partly packed copy would read as absent above
        if ((p.f1_off.size() % np) || (p.h1_off.size() % np) || (p.q1.size() % np)) throw std::runtime_error("partly packed resblock");
      }
      std::printf(
          "{\"stage\": %zu, \"C\": %d, \"mrf\": \"%s\", \"rb\": [%s], \"chain_wanted\": %s, \"pre_act_out\": %s, "
          "\"in_act\": %s, \"ups_act_out\": %s, \"mrf_act_out\": %s, \"record\": \"%s\", \"rb_record\": [%s], "
          "\"wants\": [%s], \"packed\": [%s]}\n",
          i, plan.ups[i].cout, kMrf[(int)r.mrf], rb.c_str(), tf(r.chain_wanted), tf(t.pre_act_out), tf(r.in_act),
          tf(r.ups_act_out), tf(r.mrf_act_out), r.record, rec.c_str(), want.c_str(), packed.c_str());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "voc_route_dump: %s\n", e.what());
    return 1;
  }
  return 0;
}
