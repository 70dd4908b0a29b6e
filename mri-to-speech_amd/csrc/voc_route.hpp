// Which kernels the HiFi-GAN generator's MRF stages run: one record per upsampling stage, planned once per engine.
// voc_pack_wants() says which extra copies of a resblock's weights the packer stages (pack_vocoder.cpp packs what it
// says); voc_route() chooses each stage's route from the config, the engine dtype, the switches and those copies.
// Both are pure functions (they call the kernels' *_supported predicates and no HIP API: tests/voc_route_dump.cpp
// prints the table without a device).  Neither depends on a call's B or T, so the Vocoder constructor builds the
// table once and vocoder.cpp executes its records.  DESIGN.md "The vocoder route table" has the ladders as tables.
//
// Two passes.  The first runs each stage's ladder, first match wins.  The second settles the LeakyReLU hand-offs
// from the routes on both sides: a batched stage reads lrelu(x) from its upsampler and, where an upsampler follows,
// stores lrelu(S) from its last accumulation, so that upsampler does not re-apply LeakyReLU to its operand
// fragments every K step; conv_pre does the same for stage 0 in a split engine.
//
// What the executor still decides, because it needs what the table does not take:
//  - whether a Pair stage's last pairs run chained in one launch: chain_wanted is the switch half;
//    conv1d_halo_pair_fills(C, B, L) asks the device for the kernel's resident workgroup slots and needs the call's
//    shape;
//  - the order of the resblocks inside a batched launch (longest K first, from the packed convs' kp).
#pragma once

#include <vector>

#include "../../include/m2s.h"
#include "switches.hpp"

namespace m2s {

// The extra copies of one resblock's convs beside the conv_gemm packing every resblock gets
struct RbWants {
  bool frag = false;  // rb1_fused's fragment order (RB::f1, f2)
  bool halo = false;  // conv1d_halo's fragment order (RB::h1, h2): the per-conv kernel and the fused pair share it
  bool q8 = false;    // e4m3 rows for conv1d_f8 (RB::q1, q2)
};
struct VocPackWants {
  std::vector<RbWants> rbs;  // resblock j of stage i at i * n_kernels + j, as VocoderPlan::rbs
};
// M2S_E_ARG for a dtype the engines do not have or a config outside the arrays' bounds: resblock 1 or 2, 1..8 stages
// and kernel sizes, 1..8 dilations each.  Every reader of `h` below starts with it
void check_generator_config(const m2s_hifigan_h& h, int dtype);
VocPackWants voc_pack_wants(const m2s_hifigan_h& h, int dtype, const Switches& sw);

enum class MrfRoute {
  Pair,         // split: each (c1, c2) pair in one launch, batched over the resblocks (conv1d_halo_pair_kernel)
  HaloBatched,  // split: a launch per conv, batched over the resblocks, input rows staged once (conv1d_halo_sp)
  GemmBatched,  // split: the same launches on conv_gemm
  F8,           // fp8: e4m3 operands (conv1d_f8)
  PerResblock   // resblock by resblock, each on StageRoute::rb
};
enum class RbRoute { Convs, Fused };  // run_conv pairs, or one rb1_fused launch for the resblock and its share of the MRF sum

struct StageRoute {
  MrfRoute mrf = MrfRoute::PerResblock;
  RbRoute rb[8] = {};         // PerResblock: per resblock (unused on the other routes)
  bool chain_wanted = false;  // Pair: M2S_MRF_CHAIN; the executor adds conv1d_halo_pair_fills
  bool in_act = false;        // the upsampler's input already holds lrelu(x): its producer stored it so
  bool ups_act_out = false;   // the upsampler stores lrelu(x): the stage's convs read it as is
  bool mrf_act_out = false;   // the stage's last accumulation stores lrelu(S) for the next upsampler
  // prefix of the launch records of the stage's MRF convs; PerResblock: "" here, per resblock in rb_record
  const char* record = "";
  const char* rb_record[8] = {};
  bool batched() const { return mrf == MrfRoute::Pair || mrf == MrfRoute::HaloBatched || mrf == MrfRoute::GemmBatched; }
};

struct VocRoute {
  bool pre_act_out = false;  // conv_pre stores lrelu(x)
  std::vector<StageRoute> stages;  // one per upsampling stage
};

VocRoute voc_route(const m2s_hifigan_h& h, int dtype, const Switches& sw, const VocPackWants& wants);

}  // namespace m2s
