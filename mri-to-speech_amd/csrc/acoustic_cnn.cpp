// The acoustic model's CNN (tf_efficientnetv2_b2 backbone + GAP): the scratch of a pass, and the launches of the
// route table cnn_route() (cnn_route.hpp) plans for it.  Which kernel takes which block, shape and switch is decided
// there, once per pass size; the effnet_* functions here execute one record each: a switch on the route, each case
// the launcher call with its flops / bytes record.  The weights are packed by pack_acoustic.cpp (host code); the
// constructor here reads the switches, packs, uploads the arena and resolves device pointers.
#include <algorithm>

#include "plan_util.hpp"
#include "prof.hpp"

namespace m2s {

Acoustic::Acoustic(const StateDict& sd, int n_mels, int hidden, int dtype, int device)
    : dtype_(dtype), device_(device), n_mels_(n_mels), hidden_(hidden), sw_(Switches::from_env()) {
  pack_acoustic(sd, n_mels, hidden, dtype, arena_, p_);
  arena_.upload(device);
  for (auto& b : p_.blocks) {
    b.c1.resolve(arena_);
    if (b.type != 0) b.c2.resolve(arena_);
    if (b.type == 2) {
      b.se1.resolve(arena_);
      b.se2.resolve(arena_);
    }
  }
  p_.lstm_ih.resolve(arena_);
  M2S_HIP(hipHostMalloc(reinterpret_cast<void**>(&err_host_), sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent));
  *err_host_ = 0;
  M2S_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&err_dev_), err_host_, 0));
  M2S_HIP(hipMalloc(&gsync_, lstm_sync_bytes(true)));
  // zeroed here, not only by the first launch: where that launch is captured its memset is only recorded, and the
  // eager launches after it continue the count without one (lstm_route.hpp lstm_epoch_rule)
  M2S_HIP(hipMemset(gsync_, 0, lstm_sync_bytes(true)));
  M2S_HIP(hipDeviceSynchronize());
}

Acoustic::~Acoustic() {
  if (err_host_) (void)hipHostFree(err_host_);
  if (gsync_) (void)hipFree(gsync_);
}

unsigned Acoustic::take_async_error() { return __atomic_exchange_n(err_host_, 0u, __ATOMIC_ACQ_REL); }

void Acoustic::effnet_dims(int H, int W, size_t* io, size_t* mid, size_t* se) const {
  size_t mio = 0, mmid = 0, mse = 0;
  for_each_backbone_map(H, W, [&](const BlockDef& d, const BlockMap& m) {
    if (d.type == 1) mmid = std::max(mmid, (size_t)m.oh * m.ow * chan_stride(d.mid));
    if (d.type == 2) {
      mmid = std::max(mmid, (size_t)m.ih * m.iw * chan_stride(d.mid));
      mse = std::max(mse, (size_t)dw_pixel_blocks(m.oh, m.ow) * chan_stride(d.mid));
      if (d.stride == 2 && m.oh % 4 == 0) mse = std::max(mse, (size_t)ir_s2band_bands(m.oh) * chan_stride(d.mid));
    }
    // every map a block reads or writes (block 0 reads the stem's output)
    mio = std::max({mio, (size_t)m.ih * m.iw * chan_stride(d.cin), (size_t)m.oh * m.ow * chan_stride(d.cout)});
  });
  *io = mio;
  *mid = mmid;
  *se = mse;
}

size_t Acoustic::effnet_x8(int H, int W) const {
  if (dtype_ != M2S_DT_FP8 || (!sw_.f8_expand && !sw_.f8_er)) return 0;
  size_t mx = 0;
  for_each_backbone_map(H, W, [&](const BlockDef& d, const BlockMap& m) {
    const Block& b = p_.blocks[d.index];
    if (b.f8_pw && sw_.f8_expand) mx = std::max(mx, (size_t)m.ih * m.iw * b.f8x_kp);  // the block input's map
    if (b.er8 && sw_.f8_er) mx = std::max(mx, (size_t)m.oh * m.ow * 32);              // er8_fused x8 / y8 (N, H, W, 32)
    if (b.er8w && sw_.f8_er) mx = std::max(mx, (size_t)m.oh * m.ow * 64);             // er8w_fused x8 / y8 (N, H, W, 64)
  });
  return round_up((int)mx, 256);
}

// Frames per CNN pass: `chunk`, or, where one pass fewer of at most chunk + chunk / 16 frames covers N, that
// (8 x 1000 frames: 4 passes of 2000 instead of 4 x 1920 + a 320-frame tail, which fills the persistent
// kernels' one-workgroup-per-CU grids for under two of their rounds).  Every pass is exact (per-frame work), so
// the split never changes a result (test_effnet_chunking_is_exact).
int Acoustic::pass_frames(int N) const {
  if (N <= chunk) return N;
  const int n = ceil_div(N, chunk), even = ceil_div(N, n - 1);
  return even <= chunk + chunk / 16 ? even : chunk;
}

template <typename T>
Acoustic::EffBufs<T> Acoustic::effnet_bufs(Workspace& ws, int N, int H, int W) const {
  size_t io, mid, se;
  effnet_dims(H, W, &io, &mid, &se);
  const size_t nc = pass_frames(N), R = Elem<T>::R;  // split fp32: hi + lo planes
  EffBufs<T> b{};
  b.A = ws.take<T>(nc * io * R);
  b.B = ws.take<T>(nc * io * R);
  b.M = ws.take<T>(nc * mid * R);
  b.M2 = ws.take<T>(nc * mid * R);
  b.sums = ws.take<float>(nc * se);
  b.se_mean = ws.take<T>(nc * p_.max_mid_cs * R);
  b.se_hid = ws.take<T>(nc * SE_RD_MAX * R);
  b.scale = ws.take<T>(nc * p_.max_mid_cs * R);
  if (const size_t x8b = effnet_x8(H, W))
    for (uint8_t*& x : b.X8) x = ws.take<uint8_t>(nc * x8b);
  return b;
}

void Acoustic::effnet_ws(Workspace& ws, int N, int H, int W) const {
  dispatch_act(dtype_, [&](auto t) { effnet_bufs<typename decltype(t)::type>(ws, N, H, W); });
}

float* Acoustic::feats_buf(Workspace& ws, size_t rows) const { return ws.take<float>(rows * EFF_OUT); }

float* Acoustic::cnn_feats(const float* frames, long N, int H, int W, Workspace& ws, hipStream_t s) {
  float* feats = feats_buf(ws, (size_t)N);
  effnet(frames, (int)N, H, W, feats, -1, nullptr, nullptr, ws, s);
  return feats;
}

void Acoustic::effnet(const float* frames, int N, int H, int W, float* feats, int stop_after, float* probe,
                      int* probe_dims, Workspace& ws, hipStream_t s) {
  StageTag tag("cnn");
  dispatch_act(dtype_, [&](auto t) {
    effnet_t<typename decltype(t)::type>(frames, N, H, W, feats, stop_after, probe, probe_dims, ws, s);
  });
}

template <class Pass>  // a k x k conv of the pass's block: input oh x ow, output nh x nw
static ConvArgs conv2d_args(const Pass& p, const PConv& pc, const void* x, void* y) {
  ConvArgs a = conv_args(pc);
  a.x = x;
  a.y = y;
  const BlockRoute& r = *p.r;
  a.IH = r.oh;
  a.IW = r.ow;
  a.OH = r.nh;
  a.OW = r.nw;
  a.pad_t = r.qt;
  a.pad_l = r.ql;
  a.M = p.nc * r.nh * r.nw;
  return a;
}

template <typename T>
void Acoustic::effnet_cn(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  ConvArgs a = conv2d_args(p, b.c1, p.cur, p.nxt);
  a.act = ACT_SILU;
  a.res = b.skip ? p.cur : nullptr;
  run_conv<T>(a, b.c1, sw_.conv, p.s);
}

template <typename T>
void Acoustic::effnet_er(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const BlockRoute& r = *p.r;
  const int nc = p.nc, oh = r.oh, ow = r.ow, nh = r.nh, nw = r.nw, qt = r.qt, ql = r.ql;
  T *const cur = p.cur, *const nxt = p.nxt;
  hipStream_t s = p.s;
  const int co = chan_stride(b.cout);
  const double px = (double)nc * nh * nw, flops = 2.0 * px * b.mid * (9.0 * b.cin + b.cout);
  if constexpr (kSplit<T>) {
    switch (r.er) {
      case ErRoute::ErSp:
        launch_er_sp(cur, nc, nh, nw, b.c1.cs_in, b.mid, co, arena_.ptr(b.er_sp_w), b.c1.b, b.c2.b, nxt, flops,
                     4.0 * px * (b.c1.cs_in + co), s, sw_.er_mrg);
        return;
      case ErRoute::Ers2Sp:
        launch_ers2_sp(cur, nc, oh, ow, nh, nw, qt, ql, b.c1.cs_in, b.mid, co, arena_.ptr(b.er_wexp), b.c1.b,
                       arena_.ptr(b.er_wpwl), b.c2.b, nxt, flops, 4.0 * ((double)nc * oh * ow * b.c1.cs_in + px * co), s);
        return;
      default:
        break;
    }
  } else if constexpr (std::is_same<T, bf16_t>::value) {
    // fp8: the e4m3 copy of the input a producer wrote, and the one of the output the next block reads
    const uint8_t* const x8 = r.x8_in ? p.cur8 : nullptr;
    uint8_t* const y8 = p.next8 = r.y8_out ? p.other8() : nullptr;
    switch (r.er) {
      case ErRoute::Er8:  // without x8 the kernel converts its input itself (M2S_ER8_X8=0)
        launch_er8_fused(cur, nc, nh, nw, arena_.at<uint8_t>(b.er8_wexp), arena_.at<float>(b.er8_sexp), b.c1.b,
                         arena_.at<uint8_t>(b.er8_wpwl), arena_.at<float>(b.er8_spwl), b.c2.b, nxt, flops,
                         2.0 * px * (2.0 * b.cin) + (3.0 * 8 * 2048 + 2 * 2048), s, x8, y8);
        return;
      case ErRoute::Er:
        launch_er_fused(cur, nc, nh, nw, arena_.at<bf16_t>(b.er_wexp), b.c1.b, arena_.at<bf16_t>(b.er_wpwl), b.c2.b, nxt,
                        flops, 2.0 * px * (2.0 * b.cin) + 2.0 * (9.0 * 32 * 128 + 128 * 32), s);
        return;
      case ErRoute::Er8w:
        launch_er8w_fused(cur, x8, nc, nh, nw, arena_.at<uint8_t>(b.er8w_w), arena_.at<float>(b.er8w_sexp), b.c1.b,
                          arena_.at<float>(b.er8w_spwl), b.c2.b, nxt, y8, flops,
                          // e4m3 input + bf16 shortcut + bf16 output (+ its e4m3 copy) + the weights once
                          px * (b.cin + 2.0 * b.cin + 2.0 * b.cout + (y8 ? b.cout : 0.0)) + (9.0 * b.cin + b.cout) * b.mid, s);
        return;
      case ErRoute::Er2:
        launch_er2_fused(cur, nc, nh, nw, arena_.at<bf16_t>(b.er_wexp), b.c1.b, b.c2.b, nxt, flops,
                         2.0 * px * (2.0 * b.c1.cs_in) + 2.0 * er2_stage_elems(), s);
        return;
      case ErRoute::Ers2:  // the copy is (N, OH, OW, cs_out) bytes
        launch_ers2_fused(cur, nc, oh, ow, nh, nw, qt, ql, b.c1.cs_in, b.mid, co, arena_.at<bf16_t>(b.er_wexp), b.c1.b,
                          arena_.at<bf16_t>(b.er_wpwl), b.c2.b, nxt, flops,
                          2.0 * ((double)nc * oh * ow * b.c1.cs_in + px * co) + (y8 ? px * 32 : 0.0), s, y8);
        return;
      default:
        break;
    }
  }
  // ErRoute::Unfused: conv_exp and conv_pwl as two convs, the expanded map in M
  ConvArgs a = conv2d_args(p, b.c1, cur, p.b.M);
  a.act = ACT_SILU;
  ConvArgs q = pw_args(b.c2, p.b.M, nxt, nc * nh * nw, nh * nw);
  q.res = b.skip ? cur : nullptr;
  // conv_gemm_er_supported asks plan_ksplit and that the device, so this choice is not in the route table
  if (kSplit<T> && sw_.er_s2_fused && b.stride == 2 && conv_gemm_er_supported(a, q, sw_.conv)) {
    // split blocks.2.0: conv_pwl as conv_exp's epilogue GEMM, the expanded map stays in LDS (M is not touched);
    // compulsory bytes = the block's input and output maps and both convs' weights
    launch_conv_gemm_er(a, q, sw_.conv, s, flops,
                        4.0 * ((double)nc * oh * ow * b.cin + px * b.cout + (9.0 * b.cin + b.cout) * b.mid));
  } else {
    run_conv<T>(a, b.c1, sw_.conv, s);
    run_conv<T>(q, b.c2, sw_.conv, s);
  }
}

template <typename T>
void Acoustic::effnet_ir_front(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const BlockRoute& r = *p.r;
  const int nc = p.nc, oh = r.oh, ow = r.ow, nh = r.nh, nw = r.nw, qt = r.qt, ql = r.ql;
  T *const cur = p.cur, *const M = p.b.M, *const M2 = p.b.M2, *const se_mean = p.b.se_mean;
  float* const sums = p.b.sums;
  hipStream_t s = p.s;
  const int cs = chan_stride(b.mid);
  constexpr bool SPL = kSplit<T>;
  const bool f8 = r.f8;  // fp8 engine: e4m3 depthwise output -> the e4m3 SE GEMM
  const float *const dw_w = arena_.at<float>(b.dw_w), *const dw_b = arena_.at<float>(b.dw_b);
  // bf16 feeds the fused kernel bf16 depthwise taps (dword halves), split fp32 the fp32 taps
  const void* wdw = SPL ? dw_w : arena_.ptr(b.dw_w2);
  const double Po = (double)nh * nw, es = SPL ? 4.0 : 2.0;
  // the persistent front half on an ih x iw input map (stride 2: down to nh x nw, passed with its pads); where the
  // SE-gated conv_pwl runs on se_ws it hands it the expanded map as plain fp32 rows (mid_f32: one 16-byte store per
  // 4 channels, no split; se_ws gates the fp32 value before its one split)
  auto ir_ws = [&](int ih, int iw, int stride, int OH, int OW, int pad_t, int pad_l) {
    const double Pi = (double)ih * iw;  // (stride 1: the block's nh x nw map)
    launch_ir_ws(cur, nc, ih, iw, b.c1.cs_in, b.c1.kp, cs, b.c1.w, b.c1.b, dw_w, dw_b, M2, se_mean,
                 2.0 * nc * b.mid * (Pi * b.c1.cin + Po * 9),
                 // algorithmic bytes on the real channel counts (split fp32: 4 B an element): compulsory = the
                 // block input, the split expand weights, taps and biases, the SE means out; the depthwise output
                 // map is a spill (written here only for the SE-gated conv_pwl to read back: m2s.h spill_bytes)
                 4.0 * nc * Pi * b.c1.cin + 4.0 * b.mid * (b.c1.cin + 11.0) + 4.0 * nc * b.mid, s, ws_report(), stride,
                 OH, OW, pad_t, pad_l, 4.0 * nc * Po * b.mid, r.mid_f32, sw_.irws_parts, sw_.irws_handoff);
  };
  // fp8, the expand on e4m3: x8 of the block input, or null where the expand stays bf16
  if (r.convert8) {  // no e4m3 producer wrote this input: convert it
    p.cur8 = p.b.X8[0];
    launch_rows_e4m3(cur, (long)nc * oh * ow, b.c1.cs_in, p.cur8, b.f8x_kp, s);
  }
  const uint8_t* const x8 = r.x8_in ? p.cur8 : nullptr;
  const double Pi = (double)oh * ow;
  switch (r.front) {
    case IrFront::IrWs:
      ir_ws(nh, nw, 1, 0, 0, 0, 0);
      break;
    case IrFront::Pwdw:
      launch_ir_pwdw(cur, nc, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, wdw, dw_b, nh, nw, cs, M2, se_mean, SPL,
                     2.0 * nc * Po * b.mid * (b.c1.cin + 9), nc * Po * ((x8 ? 1.0 : es) * b.c1.cin + (f8 ? 1.0 : es) * b.mid),
                     s, f8, x8, x8 ? arena_.ptr(b.f8x_w) : nullptr, x8 ? arena_.at<float>(b.f8x_s) : nullptr, b.f8x_kp);
      break;
    case IrFront::IrWsS2:
      ir_ws(oh, ow, 2, nh, nw, qt, ql);
      break;
    case IrFront::PwdwS2:
      launch_ir_pwdw_s2(cur, nc, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, wdw, dw_b, oh, ow, nh, nw, qt, ql, cs, M2, se_mean,
                        SPL, 2.0 * nc * b.mid * (Pi * b.c1.cin + Po * 9),
                        nc * ((x8 ? 1.0 : es) * Pi * b.c1.cin + (f8 ? 1.0 : es) * Po * b.mid), s, f8, x8,
                        x8 ? arena_.ptr(b.f8x_w) : nullptr, x8 ? arena_.at<float>(b.f8x_s) : nullptr, b.f8x_kp);
      break;
    case IrFront::S2Band: {
      launch_ir_s2band(cur, nc, oh, ow, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, dw_w, dw_b, nh, nw, qt, ql, cs, M2, sums, SPL,
                       2.0 * nc * b.mid * (Pi * 1.125 * b.c1.cin + Po * 9),
                       nc * (es * Pi * b.c1.cs_in + (f8 ? 1.0 : es) * Po * cs), s, f8);
      ProfScope ps(tname<T>("se_mean_kernel"), 0.0, 4.0 * nc * cs * ir_s2band_bands(nh) + es * nc * cs, s);
      launch_se_mean<T>(sums, nc, ir_s2band_bands(nh), cs, 1.0f / (float)(nh * nw), se_mean, s);
      break;
    }
    case IrFront::Unfused: {
      ConvArgs e = pw_args(b.c1, cur, M, nc * oh * ow, oh * ow);
      e.act = ACT_SILU;
      run_conv<T>(e, b.c1, sw_.conv, s);
      {
        ProfScope ps(b.stride == 2 ? tname<T>("dwconv_kernel", ", 2") : tname<T>("dwconv_kernel", ", 1"), 2.0 * nc * nh * nw * b.mid * 9,
                     kStoreBytes<T> * (double)nc * (oh * ow + nh * nw) * b.mid, s);
        launch_dwconv<T>(M, nc, oh, ow, nh, nw, b.stride, qt, ql, b.mid, cs, dw_w, dw_b, M2, sums, s);
      }
      {
        ProfScope ps(tname<T>("se_mean_kernel"), 0.0, 4.0 * nc * cs * dw_pixel_blocks(nh, nw) + kStoreBytes<T> * (double)nc * cs, s);
        launch_se_mean<T>(sums, nc, dw_pixel_blocks(nh, nw), cs, 1.0f / (float)(nh * nw), se_mean, s);
      }
      break;
    }
  }
}

template <typename T>
void Acoustic::effnet_ir_se(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const int nc = p.nc, cs = chan_stride(b.mid);
  T *const se_mean = p.b.se_mean, *const se_hid = p.b.se_hid, *const scale = p.b.scale;
  hipStream_t s = p.s;
  switch (p.r->se) {
    case IrSe::Excite:
      launch_se_excite(se_mean, nc, b.mid, cs, b.se1.w, b.se1.kp, b.se1.b, b.rd, b.se2.w, b.se2.kp, b.se2.b, scale,
                       kSplit<T>, s);
      break;
    case IrSe::Convs: {
      ConvArgs r1 = pw_args(b.se1, se_mean, se_hid, nc, 1);  // conv_reduce + SiLU, all images of the chunk at once
      r1.act = ACT_SILU;
      run_conv<T>(r1, b.se1, sw_.conv, s);
      ConvArgs r2 = pw_args(b.se2, se_hid, scale, nc, 1);  // conv_expand + sigmoid -> per-(image, channel) gates
      r2.act = ACT_SIGMOID;
      run_conv<T>(r2, b.se2, sw_.conv, s);
      break;
    }
  }
}

template <typename T>
void Acoustic::effnet_ir_pwl(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const BlockRoute& r = *p.r;
  const int nc = p.nc, nh = r.nh, nw = r.nw, cs = chan_stride(b.mid), co = chan_stride(b.cout);
  T *const cur = p.cur, *const nxt = p.nxt, *const M2 = p.b.M2, *const scale = p.b.scale;
  hipStream_t s = p.s;
  // fp8: an e4m3 copy of the output for the next block's expand, into the buffer cur8 does not hold
  uint8_t* const next8 = p.next8 = r.y8_out ? p.other8() : nullptr;
  const int ld8 = r.ld8;
  const double rows = (double)nc * nh * nw;
  const void* const res = b.skip ? cur : nullptr;
  switch (r.pwl) {
    case IrPwl::SeWsF8:
      launch_se_ws_f8(M2, nc * nh * nw, nh * nw, cs, arena_.ptr(b.f8_w), b.f8_kp, b.f8_npad, arena_.at<float>(b.f8_s),
                      arena_.at<float>(b.f8_b), scale, res, nxt, co, s, 2.0 * rows * b.mid * b.cout,
                      rows * b.mid + 2.0 * rows * b.cout * (b.skip ? 2.0 : 1.0) + (double)b.cout * b.mid + 2.0 * nc * b.mid +
                          (next8 ? rows * b.cout : 0.0),
                      next8, ld8, ws_report(), sw_.sews_half);
      break;
    case IrPwl::SeGemmF8:
      launch_se_gemm_f8(M2, nc * nh * nw, nh * nw, cs, arena_.ptr(b.f8_w), b.f8_kp, b.f8_npad, arena_.at<float>(b.f8_s),
                        arena_.at<float>(b.f8_b), scale, res, nxt, co, s, 2.0 * rows * b.mid * b.cout,
                        rows * cs + 2.0 * rows * (double)co * (b.skip ? 2.0 : 1.0) + (double)b.f8_npad * b.f8_kp +
                            2.0 * nc * cs + (next8 ? rows * ld8 : 0.0),
                        next8, ld8);
      break;
    case IrPwl::SeWs:
      launch_se_ws(M2, nc * nh * nw, nh * nw, cs, b.c2.w, b.c2.n_pad, b.c2.b, scale, res, nxt, co, s,
                   2.0 * rows * b.mid * b.cout,
                   4.0 * rows * b.mid + 4.0 * rows * b.cout * (b.skip ? 2.0 : 1.0) + 4.0 * b.cout * b.mid + 4.0 * nc * b.mid,
                   ws_report(), r.mid_f32, sw_.sews_rev, sw_.sews_half, sw_.se_ws_cfg);
      break;
    case IrPwl::SeGemmSp:
      launch_se_gemm_sp(M2, nc * nh * nw, nh * nw, cs, b.c2.w, b.c2.n_pad, b.c2.b, scale, res, nxt, co, s,
                        2.0 * rows * b.mid * b.cout,
                        4.0 * rows * cs + 4.0 * rows * (double)co * (b.skip ? 2.0 : 1.0) + 4.0 * b.c2.n_pad * b.c2.kp +
                            4.0 * nc * cs,
                        sw_.se_sp_waves);
      break;
    case IrPwl::Conv: {
      ConvArgs q = pw_args(b.c2, M2, nxt, nc * nh * nw, nh * nw);
      q.in_xform = IN_SE_SCALE;
      q.in_scale = scale;
      q.res = res;
      run_conv<T>(q, b.c2, sw_.conv, s);
      break;
    }
  }
}

template <typename T>
void Acoustic::effnet_t(const float* frames, int N, int H, int W, float* feats, int stop_after, float* probe,
                        int* probe_dims, Workspace& ws, hipStream_t s) {
  M2S_CHECK(N > 0 && H >= 32 && W >= 32, "effnet: bad input size");
  const int nc_max = pass_frames(N);
  EffPass<T> p{};
  p.b = effnet_bufs<T>(ws, N, H, W);
  p.s = s;
  T* const A = p.b.A;
  T*& cur = p.cur;
  const float *const stem_w = arena_.at<float>(p_.stem_w), *const stem_b = arena_.at<float>(p_.stem_b);
  // the route table of a pass of nc frames: the full passes', and a shorter tail's
  auto plan = [&](int nc) {
    return cnn_route(p_.blocks, sw_, dtype_, nc, H, W, device_cus(), effnet_x8(H, W) != 0,
                     probe && stop_after >= 0 && stop_after < 2);
  };
  const CnnRoute full = plan(nc_max), tail = N % nc_max ? plan(N % nc_max) : CnnRoute{};
  for (int n0 = 0; n0 < N; n0 += nc_max) {
    const int nc = std::min(nc_max, N - n0);
    const CnnRoute& route = nc == nc_max ? full : tail;
    p.nc = nc;
    p.n0 = n0;
    int oh, ow, pt, pl;
    same_pad(H, 3, 2, &oh, &pt);
    same_pad(W, 3, 2, &ow, &pl);
    constexpr bool SPL = kSplit<T>;
    const bool front = route.stem == StemRoute::StemB0;
    cur = A;
    p.nxt = p.b.B;
    p.cur8 = nullptr;
    int cc = EFF_STEM;
    int bi = 0;
    if (front) {
      // stem + blocks.0 (two 3x3 ConvBnAct at stride 1: 32 -> 16, 16 -> 16 + skip) in one kernel
      const double px = (double)nc * oh * ow;
      launch_stem_b0(frames + (size_t)n0 * H * W, nc, H, W, oh, ow, pt, pl, stem_w, stem_b, p_.blocks[0].c1.w,
                     p_.blocks[0].c1.b, p_.blocks[0].c1.kp, p_.blocks[1].c1.w, p_.blocks[1].c1.b, p_.blocks[1].c1.kp, A, SPL,
                     2.0 * px * (EFF_STEM * 9 + 16 * 9 * 32 + 16 * 9 * 16), 4.0 * nc * H * W + (SPL ? 4.0 : 2.0) * px * 16, s,
                     sw_.stem_parts);
      cc = 16;
      bi = 2;
    } else {
      ProfScope ps(std::is_same<T, bf16_t>::value ? std::string("stem32_kernel") : tname<T>("stem_kernel"), 2.0 * nc * oh * ow * EFF_STEM * 27, 4.0 * nc * H * W + kStoreBytes<T> * (double)nc * oh * ow * 32, s);
      launch_stem<T>(frames + (size_t)n0 * H * W, nc, H, W, oh, ow, pt, pl, stem_w, stem_b, EFF_STEM,
                     chan_stride(EFF_STEM), A, s);
    }
    auto tap = [&](int done) {
      if (stop_after == done && probe) {
        launch_unpad<T>(cur, (long)nc * oh * ow, cc, chan_stride(cc), probe + (size_t)n0 * oh * ow * cc, s);
        if (probe_dims) {
          probe_dims[0] = oh;
          probe_dims[1] = ow;
          probe_dims[2] = cc;
        }
        return true;
      }
      return false;
    };
    if (tap(bi)) continue;  // bi = 0, or 2 after the fused front
    bool stopped = false;
    for (size_t k = front ? 2 : 0; k < p_.blocks.size(); ++k) {
      const Block& b = p_.blocks[k];
      p.r = &route.blocks[k];
      p.next8 = nullptr;  // the e4m3 copy of this block's output, if the block wrote one
      M2S_CHECK((!p.r->x8_in || p.r->convert8 || p.cur8) && (!(p.r->convert8 || p.r->y8_out) || p.b.X8[0]),
                "effnet: an e4m3 hand-off of the route table has no buffer");
      if (b.type == 0) {
        effnet_cn(p, k);
      } else if (b.type == 1) {
        effnet_er(p, k);
      } else {
        effnet_ir_front(p, k);
        effnet_ir_se(p, k);
        effnet_ir_pwl(p, k);
      }
      std::swap(cur, p.nxt);
      p.cur8 = p.next8;
      oh = p.r->nh;
      ow = p.r->nw;
      cc = b.cout;
      ++bi;
      if (tap(bi)) {
        stopped = true;
        break;
      }
    }
    if (stopped || !feats) continue;
    ProfScope ps(tname<T>("gap_kernel"), (double)nc * oh * ow * cc, kStoreBytes<T> * (double)nc * oh * ow * cc, s);
    launch_gap<T>(cur, nc, oh * ow, cc, chan_stride(cc), feats + (size_t)n0 * EFF_OUT, s);
  }
}

}  // namespace m2s
