// The CNN's route table (cnn_route.hpp): the ladders of the EdgeResidual and InvertedResidual blocks, then the
// e4m3 hand-offs between the routes they chose.  Host code only: no launch, no HIP call.
#include "cnn_route.hpp"

#include "model.hpp"
#include "pack.hpp"

namespace m2s {
namespace {

// What every ladder reads beside its block: the engine (dispatch_act's activation type: sp_t for bf16x3, bf16_t for
// bf16 and fp8, float for fp32) and the pass
struct Pass {
  const Switches& sw;
  bool split, bf16, not_f32;
  int nc, cus;
  bool have_x8;
};

// x8: an e4m3 copy of the block's input can be had (er8w_fused's only operand source)
ErRoute er_ladder(const Block& b, const BlockRoute& r, const Pass& p, bool x8) {
  const Switches& sw = p.sw;
  const int nh = r.nh, nw = r.nw, co = chan_stride(b.cout);
  if (p.split) {
    if (sw.er_fused && b.er_sp && er_sp_supported(nh, nw, b.c1.cs_in, b.mid, co)) return ErRoute::ErSp;
    if (sw.er_fused && b.ers_sp && b.stride == 2 && ers2_sp_supported(nh, nw, b.c1.cs_in, b.mid, co)) return ErRoute::Ers2Sp;
  } else if (p.bf16) {
    if (sw.er_fused && sw.f8_er && b.er8 && er8_fused_supported(nh, nw, b.cin, b.mid, b.cout)) return ErRoute::Er8;
    if (sw.er_fused && b.er_frag && er_fused_supported(nh, nw, b.cin, b.mid, b.cout, b.c1.kp, b.c2.kp)) return ErRoute::Er;
    if (sw.er_fused && sw.f8_er && sw.f8_er2 && b.er8w && x8 && er8w_fused_supported(nh, nw, b.c1.cs_in, b.mid, b.cout))
      return ErRoute::Er8w;
    if (sw.er_fused && b.er_frag && er2_fused_supported(nh, nw, b.c1.cs_in, b.mid, b.cout, b.c1.kp, b.c2.kp)) return ErRoute::Er2;
    if (sw.er_fused && b.er_frag && b.stride == 2 && ers2_fused_supported(nh, nw, b.c1.cs_in, b.mid, co, b.c1.kp, b.c2.kp))
      return ErRoute::Ers2;
  }
  return ErRoute::Unfused;
}

void ir_ladders(const Block& b, BlockRoute& r, const Pass& p) {
  const Switches& sw = p.sw;
  const int oh = r.oh, ow = r.ow, nh = r.nh, nw = r.nw, cs = chan_stride(b.mid), co = chan_stride(b.cout);
  const bool SPL = p.split, FUSABLE = p.not_f32;
  const bool big = p.nc >= sw.irws_min;  // persistent ir_ws only where its one-image workgroups fill the chip
  // the SE-gated conv_pwl runs on se_ws: one persistent workgroup per tile (256 rows; 128 at 8 x 8) up to one per CU;
  // below a full round of tiles the split-K conv_gemm SE GEMM fills the chip instead
  const bool sews = SPL && sw.se_ws && se_ws_supported(nh * nw, cs, co) &&
                    ceil_div(p.nc * nh * nw, nh * nw == 64 ? 128 : 256) >= sw.sews_min_cus * p.cus;
  const bool gemm8 = b.f8_pwl && se_gemm_f8_supported(nh * nw, cs, co);  // fp8 engines: the e4m3 SE GEMM takes the block
  if (SPL && b.stride == 1 && sw.ir_fused && sw.ir_ws && big && ir_ws_supported(nh, nw, b.c1.cs_in, b.c1.kp, cs)) {
    r.front = IrFront::IrWs;
  } else if (FUSABLE && b.stride == 1 && sw.ir_fused && ir_fused_supported(nh, nw, b.c1.cs_in, cs, SPL)) {
    r.front = IrFront::Pwdw;
    r.f8 = gemm8;
  } else if (SPL && b.stride == 2 && sw.ir_fused && sw.ir_ws && sw.ir_ws_s2 && big &&
             ir_ws_s2_supported(oh, ow, b.c1.cs_in, b.c1.kp, cs, nh, nw, r.qt, r.ql)) {
    r.front = IrFront::IrWsS2;
  } else if (FUSABLE && b.stride == 2 && sw.ir_fused && ir_fused_s2_supported(oh, ow, b.c1.cs_in, cs, SPL) && nh * nw <= 64) {
    r.front = IrFront::PwdwS2;  // fp8 engines (blocks.5.0): e4m3 depthwise output, the expand on e4m3 as for stride 1
    r.f8 = sw.f8_s2 && gemm8;
  } else if (FUSABLE && b.stride == 2 && sw.ir_fused && sw.ir_s2band &&
             ir_s2band_supported(oh, ow, nh, nw, b.c1.cs_in, b.c1.kp, cs)) {
    r.front = IrFront::S2Band;  // fp8 engines (blocks.3.0): e4m3 depthwise output (the expand stays bf16)
    r.f8 = sw.f8_s2 && gemm8;
  } else {
    r.front = IrFront::Unfused;
  }
  const bool ws = r.front == IrFront::IrWs || r.front == IrFront::IrWsS2, pwdw = r.front == IrFront::Pwdw || r.front == IrFront::PwdwS2;
  r.mid_f32 = ws && sews && sw.irws_f32;
  // the expand on e4m3: ir_pwdw / ir_pwdw_s2 read x8 of the block input
  r.x8_in = pwdw && r.f8 && sw.f8_expand && b.f8_pw && p.have_x8;

  r.se = FUSABLE && sw.se_fused && se_excite_supported(b.rd, b.se2.kp, cs) ? IrSe::Excite : IrSe::Convs;

  if (r.f8 && sw.se_ws && se_ws_f8_supported(nh * nw, cs, co)) {
    r.pwl = IrPwl::SeWsF8;
  } else if (r.f8) {
    r.pwl = IrPwl::SeGemmF8;
  } else if (sews) {
    r.pwl = IrPwl::SeWs;
  } else if (SPL && sw.se_sp && se_gemm_sp_supported(nh * nw, cs, co)) {
    r.pwl = IrPwl::SeGemmSp;
  } else {
    r.pwl = IrPwl::Conv;
  }
}

const char* er_record(ErRoute e) {
  const char* const names[] = {"",
                               "er_sp_kernel",
                               "ers2_sp_kernel",
                               "er8_fused_kernel",
                               "er_fused_kernel",
                               "er8w_fused_kernel",
                               "er2_fused_kernel",
                               "ers2_fused_kernel"};
  return names[(int)e];
}
const char* front_record(IrFront f) {
  const char* const names[] = {"ir_ws_kernel", "ir_pwdw_kernel", "ir_ws_kernel", "ir_pwdw_s2_kernel", "ir_s2band_kernel", ""};
  return names[(int)f];
}

// Row stride in bytes of the e4m3 copy block k's last kernel can store: 0 none, -1 any (the e4m3 SE GEMMs take ld8)
int stores8(const Block& b, const BlockRoute& r, const Switches& sw) {
  if (b.type == 1) {
    if (r.er == ErRoute::Er8) return r.x8_in ? 32 : 0;  // er8_fused stores y8 only beside an x8 input
    if (r.er == ErRoute::Er8w) return 64;
    if (r.er == ErRoute::Ers2) return chan_stride(b.cout);  // (N, OH, OW, cs_out) bytes
    return 0;
  }
  return b.type == 2 && r.f8 && sw.se_y8 ? -1 : 0;
}

// ... and of the copy of its input block k's kernel reads (0: none).  er8_fused reads one where M2S_ER8_X8 lets the
// producer write it and converts in the kernel otherwise; er8w_fused and the e4m3 expand always read one.
int reads8(const Block& b, const BlockRoute& r, const Pass& p) {
  if (!p.have_x8) return 0;
  if (b.type == 1) return r.er == ErRoute::Er8 ? (p.sw.er8_x8 ? 32 : 0) : r.er == ErRoute::Er8w ? 64 : 0;
  return b.type == 2 && r.x8_in ? b.f8x_kp : 0;
}

}  // namespace

CnnRoute cnn_route(const std::vector<Block>& blocks, const Switches& sw, int dtype, int nc, int H, int W, int cus,
                   bool have_x8, bool tap_before_block2) {
  const Pass p{sw, dtype == M2S_DT_BF16X3, dtype == M2S_DT_BF16 || dtype == M2S_DT_FP8, dtype != M2S_DT_F32, nc, cus, have_x8};
  CnnRoute t;
  // stem + blocks.0 (two 3x3 ConvBnAct at stride 1: 32 -> 16, 16 -> 16 + skip) in one kernel
  const bool front = p.not_f32 && sw.stem_fused && !tap_before_block2 && blocks.size() >= 2 && blocks[0].type == 0 &&
                     blocks[0].stride == 1 && !blocks[0].skip && blocks[0].cout == 16 && blocks[0].c1.cs_in == 32 &&
                     blocks[0].c1.kp == 288 && blocks[1].type == 0 && blocks[1].stride == 1 && blocks[1].skip &&
                     blocks[1].cout == 16 && blocks[1].c1.cs_in == 16 && blocks[1].c1.kp == 160 && chan_stride(16) == 16;
  t.stem = front ? StemRoute::StemB0 : StemRoute::Stem;
  t.blocks.resize(blocks.size());

  // first pass: geometry and ladders
  int oh, ow, pad;
  same_pad(H, 3, 2, &oh, &pad);
  same_pad(W, 3, 2, &ow, &pad);
  for (size_t k = 0; k < blocks.size(); ++k) {
    const Block& b = blocks[k];
    BlockRoute& r = t.blocks[k];
    r.oh = oh;
    r.ow = ow;
    same_pad(oh, 3, b.stride, &r.nh, &r.qt);
    same_pad(ow, 3, b.stride, &r.nw, &r.ql);
    if (b.type == 1) r.er = er_ladder(b, r, p, have_x8);
    if (b.type == 2) ir_ladders(b, r, p);
    oh = r.nh;
    ow = r.nw;
  }

  // second pass: block k - 1 stores the copy block k reads, if its kernel can
  for (size_t k = 0; k < blocks.size(); ++k) {
    const Block& b = blocks[k];
    BlockRoute& r = t.blocks[k];
    auto handed = [&] {
      if (k == 0) return false;
      const int st = stores8(blocks[k - 1], t.blocks[k - 1], sw), rd = reads8(b, r, p);
      return rd != 0 && (st == rd || st == -1);
    };
    bool y8 = handed();
    if (r.er == ErRoute::Er8w && !y8) {  // no operand: the rungs below it
      r.er = er_ladder(b, r, p, false);
      y8 = handed();
    }
    if (b.type == 1) {
      r.x8_in = y8;
      r.record = er_record(r.er);
    } else if (b.type == 2) {
      r.convert8 = r.x8_in && !y8;
      r.record = front_record(r.front);
    }
    if (y8) {
      t.blocks[k - 1].y8_out = true;
      t.blocks[k - 1].ld8 = reads8(b, r, p);
    }
  }
  return t;
}

}  // namespace m2s
