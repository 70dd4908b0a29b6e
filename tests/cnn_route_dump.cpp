// Stand-alone dump of the CNN's route table (tests/test_cnn_route_cpu.py builds and runs it; no GPU needed):
//   cnn_route_dump <acoustic dump> <dtype 0..3> <cus> <x8 0|1> <nc>x<H>x<W> ...
// packs the acoustic model for the dtype (the dump format of tests/pack_digest.cpp), reads the M2S_* switches from
// the environment as an engine does, and prints for every pass shape one JSON line per backbone block: the shape, the
// block's index and type, the pass's stem route and every field of the block's record (csrc/cnn_route.hpp) by name.
// x8 = 1: the pass has its e4m3 hand-off buffers wherever an engine would (an fp8 engine with M2S_F8_EXPAND or
// M2S_F8_ER on: Acoustic::effnet_x8); 0: it has none.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "model.hpp"

namespace {

template <class T>
T get(FILE* f) {
  T v;
  if (std::fread(&v, sizeof(T), 1, f) != 1) {
    std::fprintf(stderr, "cnn_route_dump: truncated dump\n");
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
    std::fprintf(stderr, "cnn_route_dump: cannot open %s\n", path);
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

const char* const kStem[] = {"StemB0", "Stem"};
const char* const kEr[] = {"Unfused", "ErSp", "Ers2Sp", "Er8", "Er", "Er8w", "Er2", "Ers2"};
const char* const kFront[] = {"IrWs", "Pwdw", "IrWsS2", "PwdwS2", "S2Band", "Unfused"};
const char* const kSe[] = {"Excite", "Convs"};
const char* const kPwl[] = {"SeWsF8", "SeGemmF8", "SeWs", "SeGemmSp", "Conv"};
const char* const kType[] = {"cn", "er", "ir"};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: cnn_route_dump acoustic.bin dtype cus x8 NCxHxW ...\n");
    return 2;
  }
  try {
    Dump ac;
    load(argv[1], ac);
    const int dtype = std::atoi(argv[2]), cus = std::atoi(argv[3]);
    const m2s::StateDict sd = m2s::make_state_dict(ac.tensors.data(), (int)ac.tensors.size());
    m2s::Arena ar;
    m2s::AcousticPlan plan;
    m2s::pack_acoustic(sd, 64, 640, dtype, ar, plan);
    const m2s::Switches sw = m2s::Switches::from_env();
    const bool have_x8 = std::atoi(argv[4]) != 0 && dtype == M2S_DT_FP8 && (sw.f8_expand || sw.f8_er);
    for (int i = 5; i < argc; ++i) {
      int nc, H, W;
      if (std::sscanf(argv[i], "%dx%dx%d", &nc, &H, &W) != 3) {
        std::fprintf(stderr, "cnn_route_dump: bad shape %s\n", argv[i]);
        return 2;
      }
      const m2s::CnnRoute t = m2s::cnn_route(plan.blocks, sw, dtype, nc, H, W, cus, have_x8, false);
      for (size_t k = 0; k < t.blocks.size(); ++k) {
        const m2s::BlockRoute& r = t.blocks[k];
        const m2s::Block& b = plan.blocks[k];
        std::printf(
            "{\"nc\": %d, \"H\": %d, \"W\": %d, \"block\": %zu, \"name\": \"blocks.%d.%d\", \"type\": \"%s\", \"stem\": \"%s\", "
            "\"oh\": %d, \"ow\": %d, \"nh\": %d, \"nw\": %d, \"qt\": %d, \"ql\": %d, "
            "\"er\": \"%s\", \"front\": \"%s\", \"se\": \"%s\", \"pwl\": \"%s\", "
            "\"f8\": %s, \"mid_f32\": %s, \"x8_in\": %s, \"convert8\": %s, \"y8_out\": %s, \"ld8\": %d, "
            "\"record\": \"%s\", \"f8x_kp\": %d}\n",
            nc, H, W, k, b.stage, b.rep, kType[b.type], kStem[(int)t.stem], r.oh, r.ow, r.nh, r.nw, r.qt, r.ql,
            kEr[(int)r.er], kFront[(int)r.front], kSe[(int)r.se], kPwl[(int)r.pwl], r.f8 ? "true" : "false",
            r.mid_f32 ? "true" : "false", r.x8_in ? "true" : "false", r.convert8 ? "true" : "false",
            r.y8_out ? "true" : "false", r.ld8, r.record, b.f8x_kp);
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cnn_route_dump: %s\n", e.what());
    return 1;
  }
  return 0;
}
