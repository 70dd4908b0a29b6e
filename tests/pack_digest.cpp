// Stand-alone check of the weight packers (tests/test_pack_cpu.py builds and runs it; no GPU needed):
//   pack_digest <acoustic dump> <generator dump> <generator config> <resblock-2 dump> <resblock-2 config>
// packs the acoustic model and the generator for every dtype, the generator also with resblock "2" and with the
// e4m3 C = 64 / C = 32 switches, and prints per arena {"bytes", "fnv1a"} (64-bit FNV-1a of the staged bytes) as JSON.
// Dump: uint32 count, then per tensor uint32 name length, name, uint32 ndim, int64 shape[ndim], fp32 data.
// Config: m2s_hifigan_h as comma-separated ints in declaration order (the 8 x 8 dilation table row by row).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "model.hpp"

namespace {

struct Dump {
  std::vector<std::string> names;
  std::vector<std::vector<float>> data;
  std::vector<m2s_tensor> tensors;
};

template <class T>
T get(FILE* f) {
  T v;
  if (std::fread(&v, sizeof(T), 1, f) != 1) {
    std::fprintf(stderr, "pack_digest: truncated dump\n");
    std::exit(2);
  }
  return v;
}

void load(const char* path, Dump& d) {
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "pack_digest: cannot open %s\n", path);
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
    std::fprintf(stderr, "pack_digest: config has %zu of %zu ints\n", i, sizeof(h) / sizeof(int));
    std::exit(2);
  }
  return h;
}

bool first = true;
void report(const std::string& name, const m2s::Arena& ar) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < ar.bytes(); ++i) h = (h ^ ar.host()[i]) * 1099511628211ull;
  std::printf("%s\n  \"%s\": {\"bytes\": %zu, \"fnv1a\": \"%016llx\"}", first ? "{" : ",", name.c_str(), ar.bytes(),
              (unsigned long long)h);
  first = false;
}

const char* const kDtype[4] = {"fp32", "bf16", "bf16x3", "fp8"};  // M2S_DT_F32 .. M2S_DT_FP8

void vocoder(const std::string& name, const m2s::StateDict& sd, const m2s_hifigan_h& h, int dtype, bool mrf64, bool mrf32) {
  m2s::Arena ar;
  m2s::VocoderPlan p;
  m2s::Switches sw;  // the defaults, whatever the environment holds
  sw.f8_mrf64 = mrf64;
  sw.f8_mrf32 = mrf32;
  m2s::pack_vocoder(sd, h, dtype, m2s::voc_pack_wants(h, dtype, sw), ar, p);
  report(name, ar);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: pack_digest acoustic.bin generator.bin config generator_r2.bin config_r2\n");
    return 2;
  }
  try {
    Dump ac, g1, g2;
    load(argv[1], ac);
    load(argv[2], g1);
    load(argv[4], g2);
    const m2s::StateDict sa = m2s::make_state_dict(ac.tensors.data(), (int)ac.tensors.size());
    const m2s::StateDict s1 = m2s::make_state_dict(g1.tensors.data(), (int)g1.tensors.size());
    const m2s::StateDict s2 = m2s::make_state_dict(g2.tensors.data(), (int)g2.tensors.size());
    const m2s_hifigan_h h1 = config(argv[3]), h2 = config(argv[5]);
    static_assert(M2S_DT_F32 == 0 && M2S_DT_FP8 == 3, "dtype order");
    for (int dt = 0; dt < 4; ++dt) {
      m2s::Arena ar;
      m2s::AcousticPlan p;
      m2s::pack_acoustic(sa, 64, 640, dt, ar, p);
      report(std::string("acoustic_") + kDtype[dt], ar);
    }
    for (int dt = 0; dt < 4; ++dt) vocoder(std::string("vocoder_") + kDtype[dt], s1, h1, dt, false, false);
    for (int dt = 0; dt < 4; ++dt) vocoder(std::string("vocoder_r2_") + kDtype[dt], s2, h2, dt, false, false);
    vocoder("vocoder_fp8_mrf64", s1, h1, M2S_DT_FP8, true, false);
    vocoder("vocoder_fp8_mrf32", s1, h1, M2S_DT_FP8, false, true);
    vocoder("vocoder_fp8_mrf64_mrf32", s1, h1, M2S_DT_FP8, true, true);
    std::printf("\n}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pack_digest: %s\n", e.what());
    return 1;
  }
  return 0;
}
