// The M2S_* environment switches: every one the host side consults, with its default, and the one function that
// reads them.  Host code only (no HIP header): a plain C++ program can include it (tests/switches_dump.cpp).
//
// One lifetime: an engine (Acoustic, Vocoder) calls Switches::from_env() once, in its constructor, and keeps the
// result (`const Switches sw_`); the plan files read sw_ and hand each launcher the values it consults as plain
// arguments.  No .hip file reads the environment for a switch, so an engine keeps the values it was created under
// whatever the process environment holds later, a route decision and the launch it selects see the same value, and
// two engines of one process may differ in any switch.  (Before: M2S_KSPLIT / _MAX / _MINST, M2S_IRWS_PARTS,
// M2S_STEM_PARTS and M2S_SEWS_HALF were read at every launch; M2S_CG_BN64, M2S_CG_STAGES, M2S_SE_WS_CFG,
// M2S_SE_SP_WAVES, M2S_LSTM_SMALL_B and M2S_LSTM_MID_CH at their first use in the process and then frozen.
// DESIGN.md §28.)
//
// Outside this table: M2S_PROF_DETAIL (the profiler's record names, process-wide: prof.cpp) and M2S_IR_WS_TRACE
// (a diagnostic buffer of IRWS_TRACE builds: ir_ws.hip, stem_b0.hip).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace m2s {

// What the conv_gemm family consults (conv_gemm.hip plan_ksplit, launch_kind_xf), passed down from run_conv /
// launch_conv_gemm* / conv_gemm_er_supported by reference.  A default-constructed one is the defaults.
struct ConvTune {
  // Split K where the tiles fill under half a round of the chip's workgroup slots (conv_gemm.hip plan_ksplit).
  // M2S_KSPLIT=n forces n ranges (A/B, tests; 1 = never split); <= 0: the rule
  int ksplit = 0;
  int ksplit_max = 8;    // M2S_KSPLIT_MAX: most K ranges the rule takes (A/B of the split count, tools/ab_env.py)
  int ksplit_minst = 4;  // M2S_KSPLIT_MINST: fewest K steps a range keeps
  bool bn64 = false;  // M2S_CG_BN64=1, A/B: the split MRF convs on 128 x 64 tiles (3 stages, 2 per CU)
  int stages = 0;     // M2S_CG_STAGES=3 / 4, A/B: 3 or 4 stages at one workgroup per CU (101 / 135 KB) instead of
                      // 2 stages at two
};

struct Switches {
  // ---- CNN routes (acoustic_cnn.cpp) ----
  bool ir_fused = true;  // bf16: fused conv_pw + conv_dw + SE squeeze (env M2S_IR_FUSED=0 disables)
  bool ir_ws = true;     // split fp32: the persistent warp-specialised form of it (env M2S_IR_WS=0 disables)
  // ... with the roles handed off through LDS on every shape (env M2S_IR_WS=handoff; A/B, tests), where the default
  // runs 16-wide and 8 x 8 stride-1 maps per wave, the depthwise on the expand's accumulators (ir_ws_wave.hpp,
  // DESIGN §33, §35)
  bool irws_handoff = false;
  bool ir_ws_s2 = true;  // ... also for the stride-2 block at 16x16 (env M2S_IR_WS_S2=0: ir_pwdw_s2)
  // ir_ws -> se_ws hand-off of the expanded map as plain fp32 rows instead of split pairs (env M2S_IRWS_F32=0: split)
  bool irws_f32 = true;
  bool stem_fused = true;  // bf16: stem + blocks.0 in one kernel (env M2S_STEM_FUSED=0 disables)
  bool f8_er = true;            // fp8: EdgeResidual blocks.1.1/.2 on e4m3 (env M2S_F8_ER=0: bf16 er_fused)
  bool se_y8 = true;            // fp8: the SE GEMM also stores the next expand's e4m3 operand (env M2S_SE_Y8=0:
                                // launch_rows_e4m3 converts it; the same bytes, test_fp8_se_y8_e4m3_handoff_is_exact)
  bool f8_er2 = true;           // fp8: EdgeResidual blocks.2.1/.2 on e4m3 (er8w_fused; env M2S_F8_ER2=0: bf16 er2_fused)
  bool er8_x8 = true;           // ... their input as e4m3 bytes from the producer (env M2S_ER8_X8=0: converted
                                // in er8_fused; the same bytes, test_fp8_er8_e4m3_handoff_is_exact)
  bool f8_expand = true;        // fp8: the stride-1 IR expand on e4m3 (env M2S_F8_EXPAND=0: bf16 expand)
  bool f8_s2 = true;            // fp8: the stride-2 IR blocks (blocks.3.0 ir_s2band, blocks.5.0 ir_pwdw_s2) with e4m3
                                // depthwise output + e4m3 SE GEMM (env M2S_F8_S2=0: bf16)
  bool se_fused = true;    // bf16: SE excitation in one kernel (env M2S_SE_FUSED=0: two GEMMs)
  bool er_fused = true;    // bf16: EdgeResidual 32->128->32 in one kernel (env M2S_ER_FUSED=0 disables)
  bool se_sp = false;      // split: SE-gated conv_pwl on gemm128.hip (env M2S_SE_SP=1; default conv_gemm's in-LDS
                           // scaling: the two measured equal, 7.85 vs 7.88 ms per step, profiles/r03o_se_sp_ab.txt)
  bool se_ws = true;       // split: SE-gated conv_pwl on the warp-specialised flag ring (se_ws.hip; env M2S_SE_WS=0:
                           // conv_gemm's barrier ring; 8.03 -> 7.17 ms per step, gpurun_out s4a)
  bool er_mrg = true;      // split EdgeResidual blocks.1: merged W_hi / W_lo ring stages (env M2S_ER_MRG=0: one per
                           // slot; 2088 vs 2164 us per launch, gpurun_out r03er)
  bool ir_s2band = true;   // blocks.3.0: fused banded conv_pw + stride-2 depthwise (env M2S_IR_S2BAND=0: unfused)
  bool er_s2_fused = true;  // split blocks.2.0: conv_pwl as conv_exp's epilogue GEMM, the 128-channel map stays in LDS
                            // (conv_gemm.hip EP = 1; env M2S_ER_S2_FUSED=0: the two conv_gemm launches)
  bool sews_rev = true;     // se_ws walks its tiles newest-first, behind ir_ws's forward walk: the end of the expanded
                            // map is still in the Infinity Cache (env M2S_SEWS_REV=0: forward; bit-identical results;
                            // 6.83 -> 6.58 ms of se_ws per 1920 frames)

  // ---- CNN launch shaping ----
  // Small passes (the reference CLI's one clip, configs[1]'s 8 x 4): the persistent one-workgroup-per-image (ir_ws)
  // and one-tile-per-CU (se_ws) kernels fill a few dozen CUs there, so below these sizes the pass runs the grid forms
  // (ir_pwdw / ir_pwdw_s2, the split-K conv_gemm SE GEMM).  Env M2S_IRWS_MIN (images per pass) / M2S_SEWS_MIN (se_ws
  // tiles, in CUs: 1 = one full round) override.
  int irws_min = 512;
  int sews_min_cus = 1;
  // ir_ws tail balancing: M2S_IRWS_PARTS=n, A/B: n = n slice ranges (1 = no tail split), <= 0 = the launcher's rule
  int irws_parts = 0;
  // stem_b0 small batches: M2S_STEM_PARTS=n forces n tile-row ranges a strip (tests, A/B); 0 = the launcher's rule.
  // (A set variable is kept as max(1, atoi): the launcher clamps to 1 .. tiles_y, so "0" always meant 1.)
  int stem_parts = 0;
  // se_ws tail balancing in half tiles (M2S_SEWS_HALF=1, off by default: se_ws.hip launch_cfg has the measurement)
  bool sews_half = false;
  int se_ws_cfg = 0;    // se_ws tile / ring variants (M2S_SE_WS_CFG, A/B only; 0 = the default)
  int se_sp_waves = 8;  // se_gemm_sp: waves a workgroup (M2S_SE_SP_WAVES=4: one wave per SIMD; else 8)

  // ---- BiLSTM (acoustic_rnn.cpp) ----
  bool lstm_persistent = true;  // one-launch BiLSTM recurrence (env M2S_LSTM_PERSISTENT=0: a launch per step)
  bool lstm_mid = true;         // 4 < B <= 16: granule-exchange recurrence (env M2S_LSTM_MID=0: counter barrier)
  bool lstm_x3 = true;          // B > 4, non-fp32 engines: split-bf16 MFMA recurrence (env M2S_LSTM_X3=0: lstm_mid / f32)
  bool lstm_x3g = true;    // ... and for 5..16 sequences its granule hand-off form (env M2S_LSTM_X3G=0: lstm_x3)
  int lstm_small_b = 4;  // lstm_small's batch limit (M2S_LSTM_SMALL_B=8 selects the 8-sequence instantiation for B <= 8)
  int lstm_mid_ch = 0;   // lstm_mid's sequences per chunk (M2S_LSTM_MID_CH=4 / 8 / 16 for A/B runs); 0: 4 up to B = 8, 8 above

  // ---- vocoder (vocoder.cpp) ----
  bool mrf_fused = true;  // bf16: fused ResBlock1 kernel for C in {32, 64} (env M2S_MRF_FUSED=0 disables)
  bool mrf_halo = true;   // split: C = 64 MRF convs with once-staged input rows (env M2S_MRF_HALO=0: conv_gemm)
  // split: each (c1, c2) pair of the C = 64 stage in one launch, the tensor between the convs kept in LDS
  // (conv1d_halo_pair_kernel; env M2S_MRF_PAIR=0: one launch per conv; also off with M2S_MRF_HALO=0 / M2S_MRF_BATCH=0)
  bool mrf_pair = true;
  // ... and the last pair of every resblock chained in one launch with the MRF sum in registers, where the pass
  // fills the chip (env M2S_MRF_CHAIN=0: one launch per resblock, the sum read and written in memory)
  bool mrf_chain = true;
  // ... and the C = 128 stage on the same kernel (8 waves, one workgroup per CU) instead of conv_gemm's batches
  // (env M2S_MRF_PAIR128=1; packs that stage's weights a second time, in fragment order)
  bool mrf_pair128 = false;
  // fp8: the C = 64 / 32 MRF convs on e4m3 (conv1d_f8, 128 / C taps a K step; env M2S_F8_MRF64=1 / M2S_F8_MRF32=1).
  // Off: the fused bf16 ResBlock1 keeps a resblock's intermediates on chip and is faster at configs[4] (8 x 1000
  // frames, same box, gpurun_out/f8s2: fp8 step 74.8 ms with both fused, 79.7 with C = 64 on e4m3, 85.1 with both)
  bool f8_mrf64 = false;
  bool f8_mrf32 = false;
  bool mrf_batch = true;  // split: resblocks of a conv_gemm MRF stage batched per launch (env M2S_MRF_BATCH=0 disables)

  // ---- conv_gemm tiling and split K (both engines) ----
  ConvTune conv;

  // Reads every switch, each variable named once.  `seen` (tests): called with every name, in this order.
  template <class Seen>
  static Switches from_env(Seen seen);
  static Switches from_env() {
    return from_env([](const char*) {});
  }
};

// a flag: unset keeps the default; "0" turns it off, anything else (the empty string too) on
inline void env_flag(const char* name, bool& v) {
  if (const char* e = std::getenv(name)) v = std::strcmp(e, "0") != 0;
}
// an integer: unset keeps the default (and returns false), else atoi
inline bool env_int(const char* name, int& v) {
  const char* e = std::getenv(name);
  if (e) v = std::atoi(e);
  return e != nullptr;
}

template <class Seen>
Switches Switches::from_env(Seen seen) {
  Switches w;
  auto flag = [&](const char* name, bool& v) {
    seen(name);
    env_flag(name, v);
  };
  auto num = [&](const char* name, int& v) {
    seen(name);
    return env_int(name, v);
  };
  // atoi, 0 where unset: for the rules below that test the value, not the presence
  auto val = [&](const char* name) {
    int v = 0;
    num(name, v);
    return v;
  };
  // CNN routes (the last row: A/B and tests only)
  flag("M2S_IR_FUSED", w.ir_fused);
  flag("M2S_IR_WS", w.ir_ws);  // one variable, three values: "0" off, "handoff" on in the handed-off form, else on
  if (const char* e = std::getenv("M2S_IR_WS")) w.irws_handoff = std::strcmp(e, "handoff") == 0;
  flag("M2S_IR_WS_S2", w.ir_ws_s2);
  flag("M2S_IRWS_F32", w.irws_f32);
  flag("M2S_STEM_FUSED", w.stem_fused);
  flag("M2S_F8_EXPAND", w.f8_expand);
  flag("M2S_F8_S2", w.f8_s2);
  flag("M2S_F8_ER", w.f8_er);
  flag("M2S_ER8_X8", w.er8_x8);
  flag("M2S_F8_ER2", w.f8_er2);
  flag("M2S_SE_Y8", w.se_y8);
  flag("M2S_SE_FUSED", w.se_fused);
  flag("M2S_ER_FUSED", w.er_fused);
  flag("M2S_SE_WS", w.se_ws);
  flag("M2S_SE_SP", w.se_sp);
  flag("M2S_ER_MRG", w.er_mrg);
  flag("M2S_IR_S2BAND", w.ir_s2band);
  flag("M2S_ER_S2_FUSED", w.er_s2_fused);
  flag("M2S_SEWS_REV", w.sews_rev);
  // CNN launch shaping
  num("M2S_IRWS_MIN", w.irws_min);
  num("M2S_SEWS_MIN", w.sews_min_cus);
  num("M2S_IRWS_PARTS", w.irws_parts);  // > 0 forces, otherwise the rule
  if (int p = 0; num("M2S_STEM_PARTS", p)) w.stem_parts = std::max(1, p);
  w.sews_half = val("M2S_SEWS_HALF") == 1;
  num("M2S_SE_WS_CFG", w.se_ws_cfg);
  w.se_sp_waves = val("M2S_SE_SP_WAVES") == 4 ? 4 : 8;
  // BiLSTM
  flag("M2S_LSTM_PERSISTENT", w.lstm_persistent);
  flag("M2S_LSTM_MID", w.lstm_mid);
  flag("M2S_LSTM_X3", w.lstm_x3);
  flag("M2S_LSTM_X3G", w.lstm_x3g);
  w.lstm_small_b = val("M2S_LSTM_SMALL_B") == 8 ? 8 : 4;
  if (const int ch = val("M2S_LSTM_MID_CH"); ch == 4 || ch == 8 || ch == 16) w.lstm_mid_ch = ch;
  // vocoder
  flag("M2S_MRF_FUSED", w.mrf_fused);
  flag("M2S_MRF_BATCH", w.mrf_batch);
  flag("M2S_MRF_HALO", w.mrf_halo);
  flag("M2S_F8_MRF64", w.f8_mrf64);
  flag("M2S_F8_MRF32", w.f8_mrf32);
  flag("M2S_MRF_PAIR", w.mrf_pair);
  flag("M2S_MRF_CHAIN", w.mrf_chain);
  flag("M2S_MRF_PAIR128", w.mrf_pair128);
  // conv_gemm tiling and split K
  num("M2S_KSPLIT", w.conv.ksplit);  // > 0 forces the split count, otherwise automatic
  if (num("M2S_KSPLIT_MAX", w.conv.ksplit_max)) w.conv.ksplit_max = std::max(1, w.conv.ksplit_max);
  if (num("M2S_KSPLIT_MINST", w.conv.ksplit_minst)) w.conv.ksplit_minst = std::max(1, w.conv.ksplit_minst);
  w.conv.bn64 = val("M2S_CG_BN64") == 1;
  num("M2S_CG_STAGES", w.conv.stages);  // 3 and 4 have meaning
  return w;
}

}  // namespace m2s
