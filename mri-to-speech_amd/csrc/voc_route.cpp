// The vocoder's route table (voc_route.hpp): which copies the packer stages, the ladder of an MRF stage, then the
// LeakyReLU hand-offs between the routes the stages chose.  Host code only: no launch, no HIP call.
#include "voc_route.hpp"

#include "model.hpp"

namespace m2s {
namespace {

// resblock j of stage i: its channels, kernel size and dilations as the config has them
struct RbShape {
  int C, k, np;
  const int* dil;
};
RbShape rb_shape(const m2s_hifigan_h& h, int i, int j) {
  return {h.upsample_initial_channel >> (i + 1), h.resblock_kernel_sizes[j], h.n_dilations[j], h.resblock_dilation_sizes[j]};
}

// launch-record prefix of run_conv's kernel (conv_igemm.hip launch_conv)
const char* conv_record(int dtype) { return dtype == M2S_DT_F32 ? "conv_igemm_kernel" : "conv_gemm_kernel"; }

}  // namespace

void check_generator_config(const m2s_hifigan_h& h, int dtype) {
  M2S_CHECK(dtype == M2S_DT_F32 || dtype == M2S_DT_BF16 || dtype == M2S_DT_BF16X3 || dtype == M2S_DT_FP8, "bad dtype");
  M2S_CHECK(h.resblock == 1 || h.resblock == 2, "resblock must be 1 or 2");
  M2S_CHECK(h.n_up >= 1 && h.n_up <= 8 && h.n_kernels >= 1 && h.n_kernels <= 8, "bad generator config");
  for (int j = 0; j < h.n_kernels; ++j)
    M2S_CHECK(h.n_dilations[j] >= 1 && h.n_dilations[j] <= 8, "resblock dilations: 1..8 per kernel size");
}

VocPackWants voc_pack_wants(const m2s_hifigan_h& h, int dtype, const Switches& sw) {
  check_generator_config(h, dtype);
  const bool fsplit = dtype == M2S_DT_BF16X3;
  const bool pair128 = sw.mrf_pair && sw.mrf_pair128;  // split: the C = 128 stage gets conv1d_halo fragments too
  VocPackWants w;
  for (int i = 0; i < h.n_up; ++i)
    for (int j = 0; j < h.n_kernels; ++j) {
      const RbShape s = rb_shape(h, i, j);
      const int co = s.C, kk = s.k;
      RbWants r;
      // the fused ResBlock1 kernel's copy (fp8 engines: the fused bf16 ResBlock1 at C = 32 / 64, e4m3 convs at the
      // wider stages)
      r.frag = (dtype == M2S_DT_BF16 || dtype == M2S_DT_FP8 || fsplit) && h.resblock == 1 &&
               rb1_fused_supported(co, chan_stride(co), kk, s.dil, s.np, kk * co, fsplit);
      // fp8: the C = 128 / 256 (and, f8_mrf64, C = 64; f8_mrf32, C = 32) resblock convs as e4m3 bytes for conv1d_f8
      // (K = 128 block-scaled MFMA; C = 64: two taps a K step)
      r.q8 = dtype == M2S_DT_FP8 && h.resblock == 1 &&
             ((co >= 128 && !r.frag) || (co == 64 && sw.f8_mrf64) || (co == 32 && sw.f8_mrf32)) && conv1d_f8_supported(co, kk);
      r.halo = fsplit && h.resblock == 1 && !r.frag;
      // C = 64: the per-conv kernel and the fused pair share the fragments; C = 128 (pair128): the fused pair's only
      for (int d = 0; d < s.np; ++d)
        r.halo = r.halo && (conv1d_halo_sp_supported(co, chan_stride(co), kk, s.dil[d]) ||
                            (pair128 && co == 128 && conv1d_halo_pair_supported(co, chan_stride(co), kk, s.dil[d])));
      w.rbs.push_back(r);
    }
  return w;
}

VocRoute voc_route(const m2s_hifigan_h& h, int dtype, const Switches& sw, const VocPackWants& wants) {
  // the engine as dispatch_act's activation type has it: sp_t for bf16x3, bf16_t for bf16 and fp8, float for fp32
  const bool split = dtype == M2S_DT_BF16X3, bf16 = dtype == M2S_DT_BF16 || dtype == M2S_DT_FP8, not_f32 = dtype != M2S_DT_F32;
  check_generator_config(h, dtype);
  const int nk = h.n_kernels;
  M2S_CHECK(wants.rbs.size() == (size_t)h.n_up * nk, "voc_route: one RbWants per resblock");
  VocRoute t;
  t.stages.resize(h.n_up);

  // first pass: the ladders
  for (int i = 0; i < h.n_up; ++i) {
    StageRoute& r = t.stages[i];
    const RbWants* const w = &wants.rbs[(size_t)i * nk];
    const int C = rb_shape(h, i, 0).C;
    auto every = [&](auto pred) {  // pred(resblock j, its shape) for every resblock of the stage
      for (int j = 0; j < nk; ++j)
        if (!pred(j, rb_shape(h, i, j))) return false;
      return true;
    };
    auto every_conv = [&](bool (*supported)(int, int, int, int)) {
      return every([&](int, const RbShape& s) {
        for (int d = 0; d < s.np; ++d)
          if (!supported(C, chan_stride(C), s.k, s.dil[d])) return false;
        return true;
      });
    };
    // the resblocks batched per launch (split only).  The fused ResBlock1 kernel keeps a stage that has it: asked of
    // the first resblock alone, as the parent did
    const bool fused0 = not_f32 && sw.mrf_fused && w[0].frag;
    const bool batched = split && sw.mrf_batch && !fused0 && h.resblock == 1 && nk <= CONV_BATCH && C >= 32 && C % 32 == 0 &&
                         every([&](int, const RbShape& s) { return s.np == h.n_dilations[0]; });
    if (batched) {
      // input rows staged once per tile (conv1d_halo.hip) where the whole stage has the fragments for it
      bool halo = sw.mrf_halo && every([&](int j, const RbShape&) { return w[j].halo; });
      // each (c1, c2) pair in one launch where every pair of the stage is within the pair kernel's reach; a stage with
      // one that is not runs as a whole on the launches per conv.  Settled before halo narrows: C = 128 has the
      // fragments for the pair kernel only
      const bool pair = halo && sw.mrf_pair && split && (C == 64 || sw.mrf_pair128) && every_conv(conv1d_halo_pair_supported);
      halo = halo && every_conv(conv1d_halo_sp_supported);
      r.mrf = pair ? MrfRoute::Pair : halo ? MrfRoute::HaloBatched : MrfRoute::GemmBatched;
      r.chain_wanted = pair && sw.mrf_chain;
      r.record = pair ? "conv1d_halo_pair_kernel" : halo ? "conv1d_halo_sp_kernel" : "conv_gemm_kernel";
    } else if (bf16 && every([&](int j, const RbShape&) { return w[j].q8; })) {
      // every resblock of the stage must carry e4m3 weights (q8 is decided per resblock: k <= 31)
      r.mrf = MrfRoute::F8;
      r.record = "gemm128_kernel";
    } else {
      r.mrf = MrfRoute::PerResblock;
      for (int j = 0; j < nk; ++j) {
        r.rb[j] = not_f32 && sw.mrf_fused && w[j].frag ? RbRoute::Fused : RbRoute::Convs;
        r.rb_record[j] = r.rb[j] == RbRoute::Fused ? "rb1_fused_kernel" : conv_record(dtype);
      }
    }
  }

  // second pass: the hand-offs.  Only a batched stage's kernels read and store lrelu'd tensors (and conv_pre's
  // epilogue in a split engine); conv_post takes F.leaky_relu's default slope 0.01 on the raw S
  t.pre_act_out = split;
  for (int i = 0; i < h.n_up; ++i) {
    StageRoute& r = t.stages[i];
    r.ups_act_out = r.batched();
    r.mrf_act_out = r.batched() && i + 1 < h.n_up;
    r.in_act = i == 0 ? t.pre_act_out : t.stages[i - 1].mrf_act_out;
  }
  return t;
}

}  // namespace m2s
