// Which kernels one CNN pass runs: one record per backbone block, planned before the first launch.  cnn_route() is
// a pure function of the packed blocks, the switches, the engine dtype and the pass's shape (it calls the kernels'
// *_supported predicates and no HIP API: tests/cnn_route_dump.cpp prints its table without a device);
// acoustic_cnn.cpp executes the records.  DESIGN.md "The CNN route table" has the ladders as tables.
//
// Two passes.  The first walks the blocks in order and runs each block's ladder, first match wins, with an e4m3
// copy of the block's input taken as available wherever the X8 buffers exist.  The second settles the hand-offs from
// the routes both sides chose: block k stores an e4m3 copy of its output (y8_out) exactly when its kernel can store
// one of the row stride block k + 1's kernel reads, and that kernel reads one.  er8w_fused has no other source for
// its e4m3 operand, so a block on Er8w whose producer stores none runs its ladder again without that rung.
//
// What the executor still decides, because it needs what the table does not take:
//  - an unfused split stride-2 EdgeResidual block (blocks.2.0) runs launch_conv_gemm_er or two convs:
//    conv_gemm_er_supported asks plan_ksplit, which asks the device for its CU count;
//  - which of the two X8 buffers a copy goes to (they alternate with the block that wrote the last one);
//  - the X8 buffers' size (Acoustic::effnet_x8, part of the workspace size the C ABI reports): the table takes only
//    whether they exist.
#pragma once

#include <vector>

#include "switches.hpp"

namespace m2s {

struct Block;  // model.hpp

enum class StemRoute { StemB0, Stem };  // stem + blocks.0 in one kernel (blocks 0 and 1 then launch nothing), or the stem alone
enum class ErRoute { Unfused, ErSp, Ers2Sp, Er8, Er, Er8w, Er2, Ers2 };
enum class IrFront { IrWs, Pwdw, IrWsS2, PwdwS2, S2Band, Unfused };
enum class IrSe { Excite, Convs };
enum class IrPwl { SeWsF8, SeGemmF8, SeWs, SeGemmSp, Conv };

struct BlockRoute {
  int oh = 0, ow = 0, nh = 0, nw = 0, qt = 0, ql = 0;  // input map, output map and its TF-SAME top / left pads
  ErRoute er = ErRoute::Unfused;                       // EdgeResidual blocks
  IrFront front = IrFront::Unfused;                    // InvertedResidual blocks: expand + depthwise + SE mean,
  IrSe se = IrSe::Convs;                               // ... the SE gates,
  IrPwl pwl = IrPwl::Conv;                             // ... the gated conv_pwl
  bool f8 = false;        // fp8: e4m3 depthwise output into the e4m3 SE GEMM
  bool mid_f32 = false;   // ir_ws hands se_ws the expanded map as plain fp32 rows
  bool x8_in = false;     // the block's kernel reads an e4m3 copy of its input
  bool convert8 = false;  // ... which no producer wrote: launch_rows_e4m3 first (InvertedResidual only)
  bool y8_out = false;    // the block's last kernel also stores an e4m3 copy of its output
  int ld8 = 0;            // that copy's row stride in bytes, the consumer's (0 without y8_out)
  // prefix of the launch record of the block's EdgeResidual / front kernel; "" on the unfused legs and ConvBnAct
  // blocks, whose conv kernels run_conv chooses
  const char* record = "";
};

struct CnnRoute {
  StemRoute stem = StemRoute::Stem;
  std::vector<BlockRoute> blocks;  // one per backbone block, blocks 0 and 1 included under StemB0
};

// nc frames of H x W in an engine of `dtype` on a device of `cus` compute units.  have_x8: the pass has its e4m3
// hand-off buffers (effnet_x8(H, W) != 0).  tap_before_block2: a probe reads the stem's or blocks.0's output, which
// the fused front does not store.
CnnRoute cnn_route(const std::vector<Block>& blocks, const Switches& sw, int dtype, int nc, int H, int W, int cus,
                   bool have_x8, bool tap_before_block2);

}  // namespace m2s
