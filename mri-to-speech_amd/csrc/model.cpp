// Execution plans of the acoustic model (CNN + BiLSTM + head) and the HiFi-GAN generator: which kernel runs for
// which block, shape and switch, the scratch layouts, and the ragged / windowed / chunk calls.  The weights are
// packed by pack_acoustic.cpp / pack_vocoder.cpp (host code); the constructors here read the switches, pack,
// upload the arena and resolve device pointers.
#include "model.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pack.hpp"
#include "prof.hpp"

namespace m2s {

void Arena::upload(int device) {
  M2S_HIP(hipSetDevice(device));
  M2S_HIP(hipMalloc(&dev_, host_.size() + 256));
  M2S_HIP(hipMemcpy(dev_, host_.data(), host_.size(), hipMemcpyHostToDevice));
  std::vector<uint8_t>().swap(host_);
}

Arena::~Arena() {
  if (dev_) (void)hipFree(dev_);
}

// The M2S_* switches: read once, when an engine is created; "0" turns a flag off, anything else on.
static void env_flag(const char* name, bool& v) {
  if (const char* e = std::getenv(name)) v = std::strcmp(e, "0") != 0;
}
static void env_int(const char* name, int& v) {
  if (const char* e = std::getenv(name)) v = std::atoi(e);
}

// ------------------------------------------------------------------------------------------
// Acoustic model
Acoustic::Acoustic(const StateDict& sd, int n_mels, int hidden, int dtype, int device)
    : dtype_(dtype), device_(device), n_mels_(n_mels), hidden_(hidden) {
  // (the last row: A/B and tests only)
  for (auto [name, v] : std::initializer_list<std::pair<const char*, bool*>>{
           {"M2S_IR_FUSED", &ir_fused_},   {"M2S_IR_WS", &ir_ws_},         {"M2S_IR_WS_S2", &ir_ws_s2_},
           {"M2S_IRWS_F32", &irws_f32_},   {"M2S_STEM_FUSED", &stem_fused_}, {"M2S_F8_EXPAND", &f8_expand_},
           {"M2S_F8_S2", &f8_s2_},         {"M2S_F8_ER", &f8_er_},         {"M2S_ER8_X8", &er8_x8_},
           {"M2S_F8_ER2", &f8_er2_},       {"M2S_SE_Y8", &se_y8_},         {"M2S_SE_FUSED", &se_fused_},
           {"M2S_ER_FUSED", &er_fused_},   {"M2S_SE_WS", &se_ws_},         {"M2S_LSTM_PERSISTENT", &lstm_persistent_},
           {"M2S_LSTM_MID", &lstm_mid_},   {"M2S_LSTM_X3", &lstm_x3_},     {"M2S_LSTM_X3G", &lstm_x3g_},
           {"M2S_SE_SP", &se_sp_},         {"M2S_ER_MRG", &er_mrg_},       {"M2S_IR_S2BAND", &ir_s2band_},
           {"M2S_ER_S2_FUSED", &er_s2_fused_}, {"M2S_SEWS_REV", &sews_rev_}})
    env_flag(name, *v);
  env_int("M2S_IRWS_MIN", irws_min_);
  env_int("M2S_SEWS_MIN", sews_min_cus_);
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
  M2S_HIP(hipMalloc(&gsync_, std::max(lstm_small_sync_bytes(), lstm_x3g_sync_bytes())));
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
  if (dtype_ != M2S_DT_FP8 || (!f8_expand_ && !f8_er_)) return 0;
  size_t mx = 0;
  for_each_backbone_map(H, W, [&](const BlockDef& d, const BlockMap& m) {
    const Block& b = p_.blocks[d.index];
    if (b.f8_pw && f8_expand_) mx = std::max(mx, (size_t)m.ih * m.iw * b.f8x_kp);  // the block input's map
    if (b.er8 && f8_er_) mx = std::max(mx, (size_t)m.oh * m.ow * 32);              // er8_fused x8 / y8 (N, H, W, 32)
    if (b.er8w && f8_er_) mx = std::max(mx, (size_t)m.oh * m.ow * 64);             // er8w_fused x8 / y8 (N, H, W, 64)
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

size_t Acoustic::workspace_bytes(int B, int T, int H, int W) const {
  return Workspace::bytes([&](Workspace& ws) {
    feats_buf(ws, (size_t)B * T);
    effnet_ws(ws, B * T, H, W);
    lstm_bufs(ws, B, T);
  });
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
  a.IH = p.oh;
  a.IW = p.ow;
  a.OH = p.nh;
  a.OW = p.nw;
  a.pad_t = p.qt;
  a.pad_l = p.ql;
  a.M = p.nc * p.nh * p.nw;
  return a;
}

template <typename T>
void Acoustic::effnet_cn(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  ConvArgs a = conv2d_args(p, b.c1, p.cur, p.nxt);
  a.act = ACT_SILU;
  a.res = b.skip ? p.cur : nullptr;
  run_conv<T>(a, b.c1, p.s);
}

template <typename T>
void Acoustic::effnet_er(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const int nc = p.nc, oh = p.oh, ow = p.ow, nh = p.nh, nw = p.nw, qt = p.qt, ql = p.ql;
  T *const cur = p.cur, *const nxt = p.nxt, *const M = p.b.M;
  uint8_t *const cur8 = p.cur8, *const *const X8 = p.b.X8, *&next8 = p.next8;
  hipStream_t s = p.s;
  const double px = (double)nc * nh * nw;
  // the next block is an e4m3 EdgeResidual (er8_fused): this block also stores its output as e4m3 bytes
  // (er8w_fused, blocks.2.1/.2, always takes its e4m3 operand from the producer; M2S_ER8_X8=0 switches only
  // er8_fused to its in-kernel conversion)
  uint8_t* const er8_next = X8[0] && f8_er_ && k + 1 < p_.blocks.size() &&
                                    ((er8_x8_ && p_.blocks[k + 1].er8) || (f8_er2_ && p_.blocks[k + 1].er8w))
                                ? (cur8 == X8[0] ? X8[1] : X8[0])
                                : nullptr;
  if (std::is_same<T, sp_t>::value && er_fused_ && b.er_sp &&
      er_sp_supported(nh, nw, b.c1.cs_in, b.mid, chan_stride(b.cout))) {
    launch_er_sp(cur, nc, nh, nw, b.c1.cs_in, b.mid, chan_stride(b.cout), arena_.ptr(b.er_sp_w), b.c1.b, b.c2.b, nxt,
                 2.0 * px * b.mid * (9.0 * b.cin + b.cout), 4.0 * px * (b.c1.cs_in + chan_stride(b.cout)), s, er_mrg_);
  } else if (std::is_same<T, sp_t>::value && er_fused_ && b.ers_sp && b.stride == 2 &&
             ers2_sp_supported(nh, nw, b.c1.cs_in, b.mid, chan_stride(b.cout))) {
    launch_ers2_sp(cur, nc, oh, ow, nh, nw, qt, ql, b.c1.cs_in, b.mid, chan_stride(b.cout), arena_.ptr(b.er_wexp),
                   b.c1.b, arena_.ptr(b.er_wpwl), b.c2.b, nxt, 2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                   4.0 * ((double)nc * oh * ow * b.c1.cs_in + px * chan_stride(b.cout)), s);
  } else if (std::is_same<T, bf16_t>::value && er_fused_ && f8_er_ && b.er8 &&
             er8_fused_supported(nh, nw, b.cin, b.mid, b.cout)) {
    uint8_t* y8 = cur8 && er8_next && er8_fused_supported(nh, nw, b.cout, b.mid, b.cout) ? er8_next : nullptr;
    launch_er8_fused(reinterpret_cast<const bf16_t*>(cur), nc, nh, nw, static_cast<const uint8_t*>(arena_.ptr(b.er8_wexp)),
                     static_cast<const float*>(arena_.ptr(b.er8_sexp)), b.c1.b,
                     static_cast<const uint8_t*>(arena_.ptr(b.er8_wpwl)), static_cast<const float*>(arena_.ptr(b.er8_spwl)),
                     b.c2.b, reinterpret_cast<bf16_t*>(nxt), 2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                     2.0 * px * (2.0 * b.cin) + (3.0 * 8 * 2048 + 2 * 2048), s, cur8, y8);
    next8 = y8;
  } else if (std::is_same<T, bf16_t>::value && er_fused_ && b.er_frag &&
             er_fused_supported(nh, nw, b.cin, b.mid, b.cout, b.c1.kp, b.c2.kp)) {
    launch_er_fused(reinterpret_cast<const bf16_t*>(cur), nc, nh, nw,
                    static_cast<const bf16_t*>(arena_.ptr(b.er_wexp)), b.c1.b,
                    static_cast<const bf16_t*>(arena_.ptr(b.er_wpwl)), b.c2.b, reinterpret_cast<bf16_t*>(nxt),
                    2.0 * px * b.mid * (9.0 * b.cin + b.cout), 2.0 * px * (2.0 * b.cin) + 2.0 * (9.0 * 32 * 128 + 128 * 32), s);
  } else if (std::is_same<T, bf16_t>::value && er_fused_ && f8_er_ && f8_er2_ && b.er8w && cur8 &&
             er8w_fused_supported(nh, nw, b.c1.cs_in, b.mid, b.cout)) {
    uint8_t* y8 = er8_next && p_.blocks[k + 1].er8w ? er8_next : nullptr;
    launch_er8w_fused(reinterpret_cast<const bf16_t*>(cur), cur8, nc, nh, nw, static_cast<const uint8_t*>(arena_.ptr(b.er8w_w)),
                      static_cast<const float*>(arena_.ptr(b.er8w_sexp)), b.c1.b,
                      static_cast<const float*>(arena_.ptr(b.er8w_spwl)), b.c2.b, reinterpret_cast<bf16_t*>(nxt), y8,
                      2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                      // e4m3 input + bf16 shortcut + bf16 output (+ its e4m3 copy) + the weights once
                      px * (b.cin + 2.0 * b.cin + 2.0 * b.cout + (y8 ? b.cout : 0.0)) + (9.0 * b.cin + b.cout) * b.mid, s);
    next8 = y8;
  } else if (std::is_same<T, bf16_t>::value && er_fused_ && b.er_frag &&
             er2_fused_supported(nh, nw, b.c1.cs_in, b.mid, b.cout, b.c1.kp, b.c2.kp)) {
    launch_er2_fused(reinterpret_cast<const bf16_t*>(cur), nc, nh, nw, static_cast<const bf16_t*>(arena_.ptr(b.er_wexp)),
                     b.c1.b, b.c2.b, reinterpret_cast<bf16_t*>(nxt), 2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                     2.0 * px * (2.0 * b.c1.cs_in) + 2.0 * er2_stage_elems(), s);
  } else if (std::is_same<T, bf16_t>::value && er_fused_ && b.er_frag && b.stride == 2 &&
             ers2_fused_supported(nh, nw, b.c1.cs_in, b.mid, chan_stride(b.cout), b.c1.kp, b.c2.kp)) {
    // fp8: an e4m3 copy of the output for an er8_fused next block (the copy is (N, OH, OW, cs_out) bytes)
    uint8_t* y8 = er8_next && ((chan_stride(b.cout) == 32 && p_.blocks[k + 1].er8 && er8_fused_supported(nh, nw, 32, 128, 32)) ||
                               (chan_stride(b.cout) == 64 && p_.blocks[k + 1].er8w && er8w_fused_supported(nh, nw, 64, 224, b.cout)))
                      ? er8_next
                      : nullptr;
    launch_ers2_fused(reinterpret_cast<const bf16_t*>(cur), nc, oh, ow, nh, nw, qt, ql, b.c1.cs_in, b.mid,
                      chan_stride(b.cout), static_cast<const bf16_t*>(arena_.ptr(b.er_wexp)), b.c1.b,
                      static_cast<const bf16_t*>(arena_.ptr(b.er_wpwl)), b.c2.b, reinterpret_cast<bf16_t*>(nxt),
                      2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                      2.0 * ((double)nc * oh * ow * b.c1.cs_in + px * chan_stride(b.cout)) + (y8 ? px * 32 : 0.0), s, y8);
    next8 = y8;
  } else {
    ConvArgs a = conv2d_args(p, b.c1, cur, M);
    a.act = ACT_SILU;
    ConvArgs q = conv_args(b.c2);
    q.x = M;
    q.y = nxt;
    q.M = nc * nh * nw;
    q.OH = nh * nw;
    q.res = b.skip ? cur : nullptr;
    if (std::is_same<T, sp_t>::value && er_s2_fused_ && b.stride == 2 && conv_gemm_er_supported(a, q)) {
      // split blocks.2.0: conv_pwl as conv_exp's epilogue GEMM, the expanded map stays in LDS (M is not touched);
      // compulsory bytes = the block's input and output maps and both convs' weights
      launch_conv_gemm_er(a, q, s, 2.0 * px * b.mid * (9.0 * b.cin + b.cout),
                          4.0 * ((double)nc * oh * ow * b.cin + px * b.cout + (9.0 * b.cin + b.cout) * b.mid));
      return;
    }
    run_conv<T>(a, b.c1, s);
    run_conv<T>(q, b.c2, s);
  }
}

template <typename T>
void Acoustic::effnet_ir_front(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const int nc = p.nc, oh = p.oh, ow = p.ow, nh = p.nh, nw = p.nw, qt = p.qt, ql = p.ql;
  T *const cur = p.cur, *const M = p.b.M, *const M2 = p.b.M2, *const se_mean = p.b.se_mean;
  float* const sums = p.b.sums;
  uint8_t *&cur8 = p.cur8, *const *const X8 = p.b.X8;
  hipStream_t s = p.s;
  const int cs = chan_stride(b.mid);
  constexpr bool SPL = std::is_same<T, sp_t>::value;
  const bool FUSABLE = (std::is_same<T, bf16_t>::value && (dtype_ == M2S_DT_BF16 || dtype_ == M2S_DT_FP8)) || SPL;
  p.f8 = p.mid_f32 = false;
  bool &f8 = p.f8, &mid_f32 = p.mid_f32;  // fp8 engine: e4m3 depthwise output -> the e4m3 SE GEMM
  // bf16 feeds the fused kernel bf16 depthwise taps (dword halves), split fp32 the fp32 taps
  const void* wdw = arena_.ptr(SPL ? b.dw_w : b.dw_w2);
  const bool big = nc >= irws_min_;  // persistent ir_ws only where its one-image workgroups fill the chip
  // the SE-gated conv_pwl runs on se_ws (effnet_ir_pwl): then ir_ws hands it the expanded map as plain fp32 rows
  // (one 16-byte store per 4 channels, no split; se_ws gates the fp32 value before its one split)
  const bool sews = p.sews = SPL && se_ws_ && se_ws_supported(nh * nw, cs, chan_stride(b.cout)) &&
                             // se_ws runs one persistent workgroup per tile (256 rows; 128 at 8 x 8) up to one per CU:
                             // below a full round of tiles the split-K conv_gemm SE GEMM fills the chip instead
                             ceil_div(nc * nh * nw, nh * nw == 64 ? 128 : 256) >= sews_min_cus_ * device_cus();
  if (SPL && b.stride == 1 && ir_fused_ && ir_ws_ && big && ir_ws_supported(nh, nw, b.c1.cs_in, b.c1.kp, cs)) {
    const double P = (double)nh * nw;
    launch_ir_ws(cur, nc, nh, nw, b.c1.cs_in, b.c1.kp, cs, b.c1.w, b.c1.b, static_cast<const float*>(arena_.ptr(b.dw_w)),
                 static_cast<const float*>(arena_.ptr(b.dw_b)), M2, se_mean, 2.0 * nc * P * b.mid * (b.c1.cin + 9),
                 // algorithmic bytes on the real channel counts (split fp32: 4 B an element): compulsory = the
                 // block input, the split expand weights, taps and biases, the SE means out; the depthwise output
                 // map is a spill (written here only for the SE-gated conv_pwl to read back: m2s.h spill_bytes)
                 4.0 * nc * P * b.c1.cin + 4.0 * b.mid * (b.c1.cin + 11.0) + 4.0 * nc * b.mid, s, ws_report(), 1, 0, 0,
                 0, 0, 4.0 * nc * P * b.mid, mid_f32 = sews && irws_f32_);
  } else if (FUSABLE && b.stride == 1 && ir_fused_ && ir_fused_supported(nh, nw, b.c1.cs_in, cs, SPL)) {
    const double P = (double)nh * nw, es = SPL ? 4.0 : 2.0;
    f8 = b.f8_pwl && se_gemm_f8_supported(nh * nw, cs, chan_stride(b.cout));
    const bool f8x = f8 && f8_expand_ && b.f8_pw && X8[0];  // the expand on e4m3 (x8 of the block input)
    if (f8x && !cur8) {  // no e4m3 producer wrote this input: convert it
      cur8 = X8[0];
      launch_rows_e4m3(cur, (long)nc * nh * nw, b.c1.cs_in, cur8, b.f8x_kp, s);
    }
    launch_ir_pwdw(cur, nc, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, wdw, static_cast<const float*>(arena_.ptr(b.dw_b)),
                   nh, nw, cs, M2, se_mean, SPL, 2.0 * nc * P * b.mid * (b.c1.cin + 9),
                   nc * P * ((f8x ? 1.0 : es) * b.c1.cin + (f8 ? 1.0 : es) * b.mid), s, f8, f8x ? cur8 : nullptr,
                   f8x ? arena_.ptr(b.f8x_w) : nullptr, f8x ? static_cast<const float*>(arena_.ptr(b.f8x_s)) : nullptr,
                   b.f8x_kp);
  } else if (SPL && b.stride == 2 && ir_fused_ && ir_ws_ && ir_ws_s2_ && big &&
             ir_ws_s2_supported(oh, ow, b.c1.cs_in, b.c1.kp, cs, nh, nw, qt, ql)) {
    const double Pi = (double)oh * ow, Po = (double)nh * nw;
    launch_ir_ws(cur, nc, oh, ow, b.c1.cs_in, b.c1.kp, cs, b.c1.w, b.c1.b, static_cast<const float*>(arena_.ptr(b.dw_w)),
                 static_cast<const float*>(arena_.ptr(b.dw_b)), M2, se_mean, 2.0 * nc * b.mid * (Pi * b.c1.cin + Po * 9),
                 4.0 * nc * Pi * b.c1.cin + 4.0 * b.mid * (b.c1.cin + 11.0) + 4.0 * nc * b.mid, s, ws_report(), 2, nh, nw,
                 qt, ql, 4.0 * nc * Po * b.mid, mid_f32 = sews && irws_f32_);
  } else if (FUSABLE && b.stride == 2 && ir_fused_ && ir_fused_s2_supported(oh, ow, b.c1.cs_in, cs, SPL) &&
             nh * nw <= 64) {
    const double Pi = (double)oh * ow, Po = (double)nh * nw, es = SPL ? 4.0 : 2.0;
    // fp8 engines (blocks.5.0): e4m3 depthwise output for the e4m3 SE GEMM, the expand on e4m3 as for stride 1
    f8 = f8_s2_ && b.f8_pwl && se_gemm_f8_supported(nh * nw, cs, chan_stride(b.cout));
    const bool f8x = f8 && f8_expand_ && b.f8_pw && X8[0];
    if (f8x && !cur8) {  // no e4m3 producer wrote this input: convert it
      cur8 = X8[0];
      launch_rows_e4m3(cur, (long)nc * oh * ow, b.c1.cs_in, cur8, b.f8x_kp, s);
    }
    launch_ir_pwdw_s2(cur, nc, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, wdw, static_cast<const float*>(arena_.ptr(b.dw_b)),
                      oh, ow, nh, nw, qt, ql, cs, M2, se_mean, SPL, 2.0 * nc * b.mid * (Pi * b.c1.cin + Po * 9),
                      nc * ((f8x ? 1.0 : es) * Pi * b.c1.cin + (f8 ? 1.0 : es) * Po * b.mid), s, f8,
                      f8x ? cur8 : nullptr, f8x ? arena_.ptr(b.f8x_w) : nullptr,
                      f8x ? static_cast<const float*>(arena_.ptr(b.f8x_s)) : nullptr, b.f8x_kp);
  } else if (FUSABLE && b.stride == 2 && ir_fused_ && ir_s2band_ &&
             ir_s2band_supported(oh, ow, nh, nw, b.c1.cs_in, b.c1.kp, cs)) {
    const double Pi = (double)oh * ow, Po = (double)nh * nw, es = SPL ? 4.0 : 2.0;
    // fp8 engines (blocks.3.0): e4m3 depthwise output for the e4m3 SE GEMM (the expand stays bf16)
    f8 = f8_s2_ && b.f8_pwl && se_gemm_f8_supported(nh * nw, cs, chan_stride(b.cout));
    launch_ir_s2band(cur, nc, oh, ow, b.c1.cs_in, b.c1.kp, b.c1.w, b.c1.b, static_cast<const float*>(arena_.ptr(b.dw_w)),
                     static_cast<const float*>(arena_.ptr(b.dw_b)), nh, nw, qt, ql, cs, M2, sums, SPL,
                     2.0 * nc * b.mid * (Pi * 1.125 * b.c1.cin + Po * 9),
                     nc * (es * Pi * b.c1.cs_in + (f8 ? 1.0 : es) * Po * cs), s, f8);
    ProfScope ps(tname<T>("se_mean_kernel"), 0.0, 4.0 * nc * cs * ir_s2band_bands(nh) + es * nc * cs, s);
    launch_se_mean<T>(sums, nc, ir_s2band_bands(nh), cs, 1.0f / (float)(nh * nw), se_mean, s);
  } else {
    ConvArgs e = conv_args(b.c1);
    e.x = cur;
    e.y = M;
    e.M = nc * oh * ow;
    e.OH = oh * ow;
    e.act = ACT_SILU;
    run_conv<T>(e, b.c1, s);
    {
      ProfScope ps(b.stride == 2 ? tname<T>("dwconv_kernel", ", 2") : tname<T>("dwconv_kernel", ", 1"), 2.0 * nc * nh * nw * b.mid * 9,
                   (sizeof(T) * Elem<T>::R) * (double)nc * (oh * ow + nh * nw) * b.mid, s);
      launch_dwconv<T>(M, nc, oh, ow, nh, nw, b.stride, qt, ql, b.mid, cs,
                       static_cast<const float*>(arena_.ptr(b.dw_w)), static_cast<const float*>(arena_.ptr(b.dw_b)),
                       M2, sums, s);
    }
    {
      ProfScope ps(tname<T>("se_mean_kernel"), 0.0, 4.0 * nc * cs * dw_pixel_blocks(nh, nw) + (sizeof(T) * Elem<T>::R) * (double)nc * cs, s);
      launch_se_mean<T>(sums, nc, dw_pixel_blocks(nh, nw), cs, 1.0f / (float)(nh * nw), se_mean, s);
    }
  }
}

template <typename T>
void Acoustic::effnet_ir_se(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const int nc = p.nc, cs = chan_stride(b.mid);
  T *const se_mean = p.b.se_mean, *const se_hid = p.b.se_hid, *const scale = p.b.scale;
  hipStream_t s = p.s;
  constexpr bool SPL = std::is_same<T, sp_t>::value;
  const bool FUSABLE = (std::is_same<T, bf16_t>::value && (dtype_ == M2S_DT_BF16 || dtype_ == M2S_DT_FP8)) || SPL;
  if (FUSABLE && se_fused_ && se_excite_supported(b.rd, b.se2.kp, cs)) {
    launch_se_excite(se_mean, nc, b.mid, cs, b.se1.w, b.se1.kp, b.se1.b, b.rd, b.se2.w, b.se2.kp, b.se2.b, scale,
                     SPL, s);
  } else {
    ConvArgs r1 = conv_args(b.se1);  // conv_reduce + SiLU, all images of the chunk at once
    r1.x = se_mean;
    r1.y = se_hid;
    r1.M = nc;
    r1.act = ACT_SILU;
    run_conv<T>(r1, b.se1, s);
    ConvArgs r2 = conv_args(b.se2);  // conv_expand + sigmoid -> per-(image, channel) gates
    r2.x = se_hid;
    r2.y = scale;
    r2.M = nc;
    r2.act = ACT_SIGMOID;
    run_conv<T>(r2, b.se2, s);
  }
}

template <typename T>
void Acoustic::effnet_ir_pwl(EffPass<T>& p, size_t k) {
  const Block& b = p_.blocks[k];
  const int nc = p.nc, nh = p.nh, nw = p.nw, cs = chan_stride(b.mid);
  T *const cur = p.cur, *const nxt = p.nxt, *const M2 = p.b.M2, *const scale = p.b.scale;
  uint8_t *const cur8 = p.cur8, *const *const X8 = p.b.X8, *&next8 = p.next8;
  hipStream_t s = p.s;
  constexpr bool SPL = std::is_same<T, sp_t>::value;
  const bool f8 = p.f8, sews = p.sews, mid_f32 = p.mid_f32;
  // the next block takes an e4m3 expand operand (fp8 engines: stride-1 IR blocks, and the stride-2 one on
  // ir_pwdw_s2, whose input map is this block's nh x nw output)
  const bool want8 = X8[0] && f8_expand_ && k + 1 < p_.blocks.size() && p_.blocks[k + 1].f8_pw &&
                     (p_.blocks[k + 1].stride == 1 ||
                      (f8_s2_ && ir_fused_s2_supported(nh, nw, p_.blocks[k + 1].c1.cs_in, chan_stride(p_.blocks[k + 1].mid), false)));
  // fp8: an e4m3 copy of the output for the next block's expand, into the buffer cur8 does not hold
  const int ld8 = want8 ? p_.blocks[k + 1].f8x_kp : 0;
  if (f8 && want8 && se_y8_) next8 = cur8 == X8[0] ? X8[1] : X8[0];
  if (f8 && se_ws_ && se_ws_f8_supported(nh * nw, cs, chan_stride(b.cout))) {
    const double rows = (double)nc * nh * nw;
    launch_se_ws_f8(M2, nc * nh * nw, nh * nw, cs, arena_.ptr(b.f8_w), b.f8_kp, b.f8_npad,
                    static_cast<const float*>(arena_.ptr(b.f8_s)), static_cast<const float*>(arena_.ptr(b.f8_b)),
                    scale, b.skip ? cur : nullptr, nxt, chan_stride(b.cout), s, 2.0 * rows * b.mid * b.cout,
                    rows * b.mid + 2.0 * rows * b.cout * (b.skip ? 2.0 : 1.0) + (double)b.cout * b.mid + 2.0 * nc * b.mid +
                        (next8 ? rows * b.cout : 0.0),
                    next8, ld8, ws_report());
  } else if (f8) {
    const double rows = (double)nc * nh * nw, co = chan_stride(b.cout);
    launch_se_gemm_f8(M2, nc * nh * nw, nh * nw, cs, arena_.ptr(b.f8_w), b.f8_kp, b.f8_npad,
                      static_cast<const float*>(arena_.ptr(b.f8_s)), static_cast<const float*>(arena_.ptr(b.f8_b)),
                      scale, b.skip ? cur : nullptr, nxt, chan_stride(b.cout), s, 2.0 * rows * b.mid * b.cout,
                      rows * cs + 2.0 * rows * co * (b.skip ? 2.0 : 1.0) + (double)b.f8_npad * b.f8_kp +
                          2.0 * nc * cs + (next8 ? rows * ld8 : 0.0),
                      next8, ld8);
  } else if (sews) {
    const double rows = (double)nc * nh * nw;
    launch_se_ws(M2, nc * nh * nw, nh * nw, cs, b.c2.w, b.c2.n_pad, b.c2.b, scale, b.skip ? cur : nullptr, nxt,
                 chan_stride(b.cout), s, 2.0 * rows * b.mid * b.cout,
                 4.0 * rows * b.mid + 4.0 * rows * b.cout * (b.skip ? 2.0 : 1.0) + 4.0 * b.cout * b.mid + 4.0 * nc * b.mid,
                 ws_report(), mid_f32, sews_rev_);
  } else if (SPL && se_sp_ && se_gemm_sp_supported(nh * nw, cs, chan_stride(b.cout))) {
    const double rows = (double)nc * nh * nw, co = chan_stride(b.cout);
    launch_se_gemm_sp(M2, nc * nh * nw, nh * nw, cs, b.c2.w, b.c2.n_pad, b.c2.b, scale, b.skip ? cur : nullptr, nxt,
                      chan_stride(b.cout), s, 2.0 * rows * b.mid * b.cout,
                      4.0 * rows * cs + 4.0 * rows * co * (b.skip ? 2.0 : 1.0) + 4.0 * b.c2.n_pad * b.c2.kp +
                          4.0 * nc * cs);
  } else {
    ConvArgs q = conv_args(b.c2);
    q.x = M2;
    q.y = nxt;
    q.M = nc * nh * nw;
    q.OH = nh * nw;
    q.in_xform = IN_SE_SCALE;
    q.in_scale = scale;
    q.res = b.skip ? cur : nullptr;
    run_conv<T>(q, b.c2, s);
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
  int &oh = p.oh, &ow = p.ow;
  T*& cur = p.cur;
  for (int n0 = 0; n0 < N; n0 += nc_max) {
    const int nc = std::min(nc_max, N - n0);
    p.nc = nc;
    p.n0 = n0;
    int pt, pl;
    same_pad(H, 3, 2, &oh, &pt);
    same_pad(W, 3, 2, &ow, &pl);
    // stem + blocks.0 (two 3x3 ConvBnAct at stride 1: 32 -> 16, 16 -> 16 + skip) in one kernel
    constexpr bool SPL = std::is_same<T, sp_t>::value;
    const bool front = ((std::is_same<T, bf16_t>::value && (dtype_ == M2S_DT_BF16 || dtype_ == M2S_DT_FP8)) || SPL) && stem_fused_ && !(probe && stop_after >= 0 && stop_after < 2) &&
                       p_.blocks.size() >= 2 && p_.blocks[0].type == 0 && p_.blocks[0].stride == 1 && !p_.blocks[0].skip &&
                       p_.blocks[0].cout == 16 && p_.blocks[0].c1.cs_in == 32 && p_.blocks[0].c1.kp == 288 &&
                       p_.blocks[1].type == 0 && p_.blocks[1].stride == 1 && p_.blocks[1].skip && p_.blocks[1].cout == 16 &&
                       p_.blocks[1].c1.cs_in == 16 && p_.blocks[1].c1.kp == 160 && chan_stride(16) == 16;
    cur = A;
    p.nxt = p.b.B;
    p.cur8 = nullptr;
    int cc = EFF_STEM;
    int bi = 0;
    if (front) {
      const double px = (double)nc * oh * ow;
      launch_stem_b0(frames + (size_t)n0 * H * W, nc, H, W, oh, ow, pt, pl, static_cast<const float*>(arena_.ptr(p_.stem_w)),
                     static_cast<const float*>(arena_.ptr(p_.stem_b)), p_.blocks[0].c1.w, p_.blocks[0].c1.b, p_.blocks[0].c1.kp,
                     p_.blocks[1].c1.w, p_.blocks[1].c1.b, p_.blocks[1].c1.kp, A, SPL,
                     2.0 * px * (EFF_STEM * 9 + 16 * 9 * 32 + 16 * 9 * 16), 4.0 * nc * H * W + (SPL ? 4.0 : 2.0) * px * 16, s);
      cc = 16;
      bi = 2;
    } else {
      ProfScope ps(std::is_same<T, bf16_t>::value ? std::string("stem32_kernel") : tname<T>("stem_kernel"), 2.0 * nc * oh * ow * EFF_STEM * 27, 4.0 * nc * H * W + (sizeof(T) * Elem<T>::R) * (double)nc * oh * ow * 32, s);
      launch_stem<T>(frames + (size_t)n0 * H * W, nc, H, W, oh, ow, pt, pl, static_cast<const float*>(arena_.ptr(p_.stem_w)),
                     static_cast<const float*>(arena_.ptr(p_.stem_b)), EFF_STEM, chan_stride(EFF_STEM), A, s);
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
      p.next8 = nullptr;  // the e4m3 copy of this block's output, if the block wrote one
      same_pad(oh, 3, b.stride, &p.nh, &p.qt);
      same_pad(ow, 3, b.stride, &p.nw, &p.ql);
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
      oh = p.nh;
      ow = p.nw;
      cc = b.cout;
      ++bi;
      if (tap(bi)) {
        stopped = true;
        break;
      }
    }
    if (stopped || !feats) continue;
    ProfScope ps(tname<T>("gap_kernel"), (double)nc * oh * ow * cc, (sizeof(T) * Elem<T>::R) * (double)nc * oh * ow * cc, s);
    launch_gap<T>(cur, nc, oh * ow, cc, chan_stride(cc), feats + (size_t)n0 * EFF_OUT, s);
  }
}

size_t Acoustic::lstm_sync_bytes() {
  return std::max({lstm_persistent_sync_bytes(), lstm_small_sync_bytes(), lstm_mid_sync_bytes(), lstm_x3_sync_bytes(),
                   lstm_x3g_sync_bytes()});
}

void Acoustic::lstm_recurrence(const float* pre, float* hs, float* cst, void* sync, int B, int T, double seq_steps,
                               double rows, hipStream_t s) {
  const int H = hidden_;
  const float* whh = static_cast<const float*>(arena_.ptr(p_.whh));
  // algorithmic bytes: W_hh of both directions once, gate pre-activations in, h out
  const double bytes = 4.0 * 2 * 4 * H * H + 4.0 * rows * (8.0 * H + 2.0 * H);
  const double f2 = 2.0 * 2 * 4.0 * H * H * seq_steps, f3 = 3.0 * 2 * 4.0 * H * H * seq_steps;
  if (lstm_persistent_ && lstm_small_supported(B, H)) {
    ProfScope ps("lstm_small_kernel", f2, bytes, s);
    launch_lstm_small(pre, whh, hs, B, T, H, gsync_, lstm_spin_max_, err_dev_, s, &gsync_epoch_);
  } else if (lstm_persistent_ && lstm_x3_ && lstm_x3g_ && dtype_ != M2S_DT_F32 && lstm_x3g_supported(B, H)) {
    // 5..16 sequences (configs[4]'s 8 clips a GPU): the granule hand-off (lstm_persistent.hip lstm_x3g_kernel)
    ProfScope ps("lstm_x3g_kernel", f3, bytes, s);
    launch_lstm_x3g(pre, whh, hs, B, T, H, gsync_, lstm_spin_max_, err_dev_, s, &gsync_epoch_);
  } else if (lstm_persistent_ && lstm_x3_ && dtype_ != M2S_DT_F32 && lstm_persistent_supported(H)) {
    // split engines above the small-batch kernel: 4.1 / 5.2 / 9.9 us per step at B = 8 / 16 / 64 against
    // lstm_mid's 7.2 / 11.9 and the f32 counter-barrier kernel's 24 (gpurun_out lstm2, lstm3_x3small)
    ProfScope ps("lstm_x3_kernel", f3, bytes, s);
    launch_lstm_x3(pre, whh, hs, B, T, H, sync, lstm_spin_max_, err_dev_, s);
  } else if (lstm_persistent_ && lstm_mid_ && lstm_mid_supported(B, H)) {
    ProfScope ps("lstm_mid_kernel", f2, bytes, s);
    launch_lstm_mid(pre, whh, hs, B, T, H, sync, lstm_spin_max_, err_dev_, s);
  } else if (lstm_persistent_ && lstm_persistent_supported(H)) {
    ProfScope ps("lstm_persistent_kernel", f2, bytes, s);
    launch_lstm_persistent(pre, whh, hs, B, T, H, sync, lstm_spin_max_, err_dev_, s);
  } else {
    for (int st = 0; st < T; ++st) {
      ProfScope ps("lstm_step_kernel", 2.0 * 2 * (rows / T) * 4.0 * H * H, 4.0 * 2 * 4 * H * H, s);
      launch_lstm_step(pre, whh, hs, cst, B, T, H, st, s);
    }
  }
}

Acoustic::LstmBufs Acoustic::lstm_bufs(Workspace& ws, int B, int T) const {
  const size_t BT = (size_t)B * T, H = (size_t)hidden_;
  LstmBufs b{};
  b.pre = ws.take<float>(BT * 8 * H);
  b.hs = ws.take<float>(2 * BT * H);
  b.cst = ws.take<float>((size_t)2 * B * H);
  b.sync = ws.take<char>(lstm_sync_bytes());
  return b;
}

void Acoustic::bilstm(const float* feats, int B, int T, float* y, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "bilstm: empty input");
  const int H = hidden_;
  const size_t BT = (size_t)B * T;
  const LstmBufs b = lstm_bufs(ws, B, T);
  float* const hs = b.hs;
  StageTag tag("bilstm");
  ConvArgs a = conv_args(p_.lstm_ih);
  a.x = feats;
  a.y = b.pre;
  a.M = (int)BT;
  // small passes (<= 64 frames): the four waves of a row tile split K (one 30-frame clip: 20 -> 12 us); larger passes
  // keep four row groups a workgroup sharing the weight tile (K split there: the 1920-frame step's projection
  // 0.13 ms slower).  The K summation order therefore differs between the two size classes (fp32 rounding only).
  // (keyed on the projection's row count M: a ragged call of N packed rows switches where a dense one of N does)
  a.kwave = BT <= 64 ? 1 : 0;
  run_conv<float>(a, p_.lstm_ih, s);
  lstm_recurrence(b.pre, hs, b.cst, b.sync, B, T, (double)B * (T - 1), (double)BT, s);
  if (mel_norm) {
    StageTag head("head");
    ProfScope ps("mel_head_kernel", 2.0 * BT * H * n_mels_, 4.0 * BT * (2 * H + n_mels_), s);
    launch_mel_head(hs, (int)BT, H, static_cast<const float*>(arena_.ptr(p_.head_wt)),
                    static_cast<const float*>(arena_.ptr(p_.head_b)), n_mels_, mel_norm, s);
  }
  if (y) launch_add2(hs, hs + BT * H, y, (long)(BT * H), s);
}

void Acoustic::forward(const float* frames, int B, int T, int H, int W, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "acoustic: empty input");
  float* feats = feats_buf(ws, (size_t)B * T);
  effnet(frames, B * T, H, W, feats, -1, nullptr, nullptr, ws, s);
  bilstm(feats, B, T, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Ragged batches (ragged.hip, DESIGN.md "Ragged batches")
RaggedDims ragged_dims(const int* lengths, int B, long rows) {
  M2S_CHECK(lengths && B >= 1, "ragged: at least one clip (lengths must not be empty)");
  RaggedDims d;
  d.B = B;
  d.Tmin = lengths[0];
  for (int b = 0; b < B; ++b) {
    M2S_CHECK(lengths[b] >= 1, "ragged: clip " + std::to_string(b) + " has length " + std::to_string(lengths[b]) +
                                   "; every length must be >= 1");
    d.N += lengths[b];
    d.Tmax = std::max(d.Tmax, lengths[b]);
    d.Tmin = std::min(d.Tmin, lengths[b]);
  }
  M2S_CHECK(d.N == rows, "ragged: sum(lengths) = " + std::to_string(d.N) + " but the packed input has " +
                             std::to_string(rows) + " rows");
  // the dense path counts its B x T rows in an int (the projection's M, the kernels' row indices)
  M2S_CHECK((double)B * d.Tmax <= 2147483647.0 && B <= 65535, "ragged: B x Tmax out of range");
  return d;
}

RaggedTable::~RaggedTable() {
  if (done_) (void)hipEventDestroy(done_);
  if (host_) (void)hipHostFree(host_);
}

void ragged_check_stream(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  M2S_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone)
    throw Error(M2S_E_STATE, "ragged calls cannot be captured into a graph (the clip table is staged per call)");
}

void RaggedTable::upload(const int* lengths, int B, int* dev, hipStream_t s) {
  std::vector<int> tab((size_t)2 * B);
  int off = 0;
  for (int b = 0; b < B; ++b) {
    tab[b] = off;
    tab[B + b] = lengths[b];
    off += lengths[b];
  }
  upload_ints(tab.data(), tab.size(), dev, s);
}

void RaggedTable::upload_ints(const int* src, size_t n, int* dev, hipStream_t s) {
  ragged_check_stream(s);
  if (!done_) M2S_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
  M2S_HIP(hipEventSynchronize(done_));  // the previous call's copy has read the staging buffer
  if (cap_ < n) {
    if (host_) M2S_HIP(hipHostFree(host_));
    host_ = nullptr;
    cap_ = 0;
    M2S_HIP(hipHostMalloc(reinterpret_cast<void**>(&host_), n * sizeof(int), hipHostMallocDefault));
    cap_ = n;
  }
  std::memcpy(host_, src, n * sizeof(int));
  M2S_HIP(hipMemcpyAsync(dev, host_, n * sizeof(int), hipMemcpyHostToDevice, s));
  M2S_HIP(hipEventRecord(done_, s));
}

size_t Acoustic::ragged_workspace_bytes(const int* lengths, int B, int H, int W) const {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  const RaggedDims d = ragged_dims(lengths, B, n);
  return Workspace::bytes([&](Workspace& ws) {
    feats_buf(ws, (size_t)d.N);
    effnet_ws(ws, (int)d.N, H, W);
    ragged_lstm_bufs(ws, d);
  });
}

Acoustic::RaggedLstmBufs Acoustic::ragged_lstm_bufs(Workspace& ws, const RaggedDims& d) const {
  RaggedLstmBufs b{};
  b.tab = ws.take<int>((size_t)2 * d.B);
  b.pre_packed = ws.take<float>((size_t)d.N * 8 * hidden_);
  b.d = lstm_bufs(ws, d.B, d.Tmax);
  return b;
}

void Acoustic::bilstm_ragged(const float* feats, const int* lengths, int B, long N, float* y, float* mel_norm,
                             Workspace& ws, hipStream_t s) {
  const RaggedDims d = ragged_dims(lengths, B, N);
  const int H = hidden_, T = d.Tmax;
  const RaggedLstmBufs rb = ragged_lstm_bufs(ws, d);
  int* const tab = rb.tab;
  float *const pre_packed = rb.pre_packed, *const pre = rb.d.pre, *const hs = rb.d.hs;
  rtab_.upload(lengths, B, tab, s);
  StageTag tag("bilstm");
  ConvArgs a = conv_args(p_.lstm_ih);
  a.x = feats;
  a.y = pre_packed;
  a.M = (int)N;
  a.kwave = N <= 64 ? 1 : 0;  // as bilstm: by the projection's row count
  run_conv<float>(a, p_.lstm_ih, s);
  {
    ProfScope ps("ragged_pre_scatter_kernel", 0.0, 2.0 * 4.0 * N * 8.0 * H, s);
    launch_ragged_pre_scatter(pre_packed, tab, B, T, 8 * H, pre, s);
  }
  // the dense kernels, Tmax steps for every clip: zero pre-activation rows keep the reverse direction's state at
  // exactly zero until the clip's last frame, and the forward direction's padded steps are never read
  lstm_recurrence(pre, hs, rb.d.cst, rb.d.sync, B, T, (double)(N - B), (double)N, s);
  StageTag head("head");
  ProfScope ps("ragged_head_gather_kernel", mel_norm ? 2.0 * N * H * n_mels_ : 0.0,
               4.0 * N * (2 * H + (mel_norm ? n_mels_ : 0) + (y ? H : 0)), s);
  launch_ragged_head_gather(hs, tab, B, T, H, static_cast<const float*>(arena_.ptr(p_.head_wt)),
                            static_cast<const float*>(arena_.ptr(p_.head_b)), n_mels_, y, mel_norm, s);
}

void Acoustic::forward_ragged(const float* frames, const int* lengths, int B, long N, int H, int W, float* mel_norm,
                              Workspace& ws, hipStream_t s) {
  ragged_dims(lengths, B, N);  // before the CNN launches
  ragged_check_stream(s);
  float* feats = feats_buf(ws, (size_t)N);
  effnet(frames, (int)N, H, W, feats, -1, nullptr, nullptr, ws, s);
  bilstm_ragged(feats, lengths, B, N, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Windowed inference (lstm_window.hip, DESIGN.md "Windowed acoustic inference")
WindowPlan window_plan(const int* lengths, const int* context, int B, long rows, int window, int merge) {
  M2S_CHECK(window >= 1 && window <= 16, "windowed: window = " + std::to_string(window) + " outside 1..16");
  M2S_CHECK(merge == M2S_WINDOW_LATEST || merge == M2S_WINDOW_MEAN, "windowed: unknown merge " + std::to_string(merge));
  M2S_CHECK(!(context && merge == M2S_WINDOW_MEAN), "windowed: a context needs the latest merge");
  const RaggedDims d = ragged_dims(lengths, B, rows);
  WindowPlan p;
  p.B = B;
  p.W = window;
  p.mean = merge == M2S_WINDOW_MEAN;
  p.N = d.N;
  p.max_len = d.Tmax;
  p.tab.resize((size_t)5 * B);
  long off = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lengths[b], ctx = context ? context[b] : 0;
    M2S_CHECK(ctx >= 0 && ctx <= window - 1 && ctx < len,
              "windowed: context[" + std::to_string(b) + "] = " + std::to_string(ctx) + " outside 0..min(window - 1, " +
                  "length - 1)");
    const int k = std::min(len, window);
    const int nwin = p.mean ? len - k + 1 : len - ctx;
    p.tab[b] = (int)off;
    p.tab[B + b] = len;
    p.tab[2 * B + b] = ctx;
    p.tab[3 * B + b] = (int)p.S;
    p.tab[4 * B + b] = (int)p.R;
    for (int j = 0; j < window; ++j)
      p.active[j] += p.mean ? (k > j ? 2.0 * nwin : 0.0) : (double)std::max(0, len - std::max(ctx, window - 1 - j));
    p.max_windows = std::max(p.max_windows, nwin);
    off += len;
    p.S += nwin;
    p.R += len - ctx;
  }
  return p;
}

Acoustic::WindowBufs Acoustic::window_bufs(Workspace& ws, const WindowPlan& p) const {
  const size_t H = (size_t)hidden_, S = (size_t)p.S, dirs = p.mean ? 2 : 1;
  WindowBufs b;
  b.tab = ws.take<int>((size_t)5 * p.B);
  b.win = ws.take<int2>(S);
  b.pre = ws.take<float>((size_t)p.N * 8 * H);
  if (p.W > 1) {  // the step operands (fp32 rows or split pairs: 4 bytes an element either way) and the cell state
    b.hop[0] = ws.take<float>(dirs * S * H);
    if (p.W > 2) b.hop[1] = ws.take<float>(dirs * S * H);
    b.c = ws.take<float>(dirs * S * H);
  }
  b.hm = ws.take<float>((size_t)(p.pairs ? 1 : 2) * p.R * H);  // pairs: the merged rows, one plane
  if (p.mean) b.hf = ws.take<float>((size_t)2 * p.W * S * H);
  return b;
}

size_t Acoustic::windowed_workspace_bytes(const int* lengths, const int* context, int B, int H, int W, int window,
                                          int merge) const {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  const WindowPlan p = window_plan(lengths, context, B, n, window, merge);
  return Workspace::bytes([&](Workspace& ws) {
    if (H != 0 || W != 0) {
      feats_buf(ws, (size_t)p.N);
      effnet_ws(ws, (int)p.N, H, W);
    }
    window_bufs(ws, p);
  });
}

// the clip table, the projection and the W step launches of a plan: what latest, mean and the pair outputs share
void Acoustic::window_steps(const float* feats, const WindowPlan& p, const WindowBufs& b, hipStream_t s) {
  const int H = hidden_, W = p.W, S = (int)p.S, dirs = p.mean ? 2 : 1, B = p.B;
  const long N = p.N;
  const bool split = dtype_ != M2S_DT_F32;
  rtab_.upload_ints(p.tab.data(), p.tab.size(), b.tab, s);
  // the projection, once per FRAME row; one K order for every row count (kwave stays 0: a row's bits must not
  // depend on how many rows the call holds, or a stream's chunking would show)
  ConvArgs a = conv_args(p_.lstm_ih);
  a.x = feats;
  a.y = b.pre;
  a.M = (int)N;
  a.kwave = 0;
  run_conv<float>(a, p_.lstm_ih, s);
  {
    ProfScope ps("lstm_window_table_kernel", 0.0, 4.0 * (5.0 * B + 2.0 * S), s);
    launch_lstm_window_table(b.tab, B, W, p.mean, p.max_windows, b.win, s);
  }
  const size_t plane = (size_t)S * H;
  {
    // step 0: three gates of one projected row per (window, unit); latest adds the reverse step of every window
    const double cells = p.active[0] + (p.mean ? 0.0 : (double)S);
    ProfScope ps("lstm_window_step0_kernel", 0.0, 4.0 * cells * H * (3.0 + 2.0), s);
    launch_lstm_window_step0(b.pre, b.win, S, !p.mean, split, b.hop[0], b.c, p.mean ? b.hf : (W == 1 ? b.hm : nullptr),
                             p.mean ? b.hf + (size_t)W * plane : b.hm + (size_t)p.R * H, s);
  }
  const float* wperm = static_cast<const float*>(arena_.ptr(p_.whh_win));
  for (int j = 1; j < W; ++j) {
    const void* hin = b.hop[(j - 1) & 1];
    void* hout = j + 1 < W ? b.hop[j & 1] : nullptr;
    float* hf = p.mean ? b.hf + (size_t)j * plane : (j == W - 1 ? b.hm : nullptr);
    // algorithmic work of the VALID window steps: W_hh of the launched directions once, and per cell update the
    // four gathered gates, h in and out, c in and out
    ProfScope ps(split ? "lstm_window_step_kernel<split>" : "lstm_window_step_kernel<f32>",
                 (split ? 3.0 : 2.0) * 4.0 * H * H * p.active[j], 4.0 * dirs * 4 * H * H + 4.0 * p.active[j] * H * 8.0, s);
    launch_lstm_window_step(b.pre, wperm, b.win, S, j, dirs, split, hin, hout, b.c, hf, (long)((size_t)W * plane), s);
  }
}

void Acoustic::bilstm_windowed(const float* feats, const int* lengths, const int* context, int B, long N, int window,
                               int merge, float* y, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  const WindowPlan p = window_plan(lengths, context, B, N, window, merge);
  ragged_check_stream(s);
  const int H = hidden_, W = p.W, S = (int)p.S;
  const WindowBufs b = window_bufs(ws, p);
  StageTag tag("bilstm");
  window_steps(feats, p, b, s);
  if (p.mean) {
    double contrib = 0.0;  // (window, step, direction) rows read: every valid one once
    for (int j = 0; j < W; ++j) contrib += p.active[j];
    ProfScope ps("lstm_window_mean_kernel", contrib * H, 4.0 * H * (contrib + 2.0 * p.N), s);
    launch_lstm_window_mean(b.hf, b.tab, B, W, S, p.N, p.max_len, b.hm, s);
  }
  if (mel_norm) {
    StageTag head("head");
    ProfScope ps("mel_head_kernel", 2.0 * p.R * H * n_mels_, 4.0 * p.R * (2 * H + n_mels_), s);
    launch_mel_head(b.hm, (int)p.R, H, static_cast<const float*>(arena_.ptr(p_.head_wt)),
                    static_cast<const float*>(arena_.ptr(p_.head_b)), n_mels_, mel_norm, s);
  }
  if (y) launch_add2(b.hm, b.hm + (size_t)p.R * H, y, (long)((size_t)p.R * H), s);
}

void Acoustic::forward_windowed(const float* frames, const int* lengths, const int* context, int B, long N, int H,
                                int W, int window, int merge, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  window_plan(lengths, context, B, N, window, merge);  // before the CNN launches
  ragged_check_stream(s);
  float* feats = feats_buf(ws, (size_t)N);
  effnet(frames, (int)N, H, W, feats, -1, nullptr, nullptr, ws, s);
  bilstm_windowed(feats, lengths, context, B, N, window, merge, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Pair outputs: every row of every training window (m2s.h "pair outputs")
WindowPlan pairs_plan(const int* lengths, int B, long rows, int window) {
  WindowPlan p = window_plan(lengths, nullptr, B, rows, window, M2S_WINDOW_MEAN);
  for (int b = 0; b < B; ++b)
    M2S_CHECK(lengths[b] >= window, "pairs: lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) +
                                        " is shorter than the window of " + std::to_string(window) +
                                        " (the reference skips such clips: leave them out)");
  M2S_CHECK((double)p.S * window <= 2147483647.0, "pairs: P x window out of range");
  p.pairs = true;
  p.R = p.S * window;
  return p;
}

size_t Acoustic::pairs_workspace_bytes(const int* lengths, int B, int H, int W, int window) const {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  const WindowPlan p = pairs_plan(lengths, B, n, window);
  return Workspace::bytes([&](Workspace& ws) {
    if (H != 0 || W != 0) {
      feats_buf(ws, (size_t)p.N);
      effnet_ws(ws, (int)p.N, H, W);
    }
    window_bufs(ws, p);
  });
}

void Acoustic::bilstm_pairs(const float* feats, const int* lengths, int B, long N, int window, float* y,
                            float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  const WindowPlan p = pairs_plan(lengths, B, N, window);
  ragged_check_stream(s);
  const int H = hidden_, W = p.W, S = (int)p.S;
  const WindowBufs b = window_bufs(ws, p);
  StageTag tag("bilstm");
  window_steps(feats, p, b, s);
  {
    // every (window, step, direction) row read once, every merged row written once (twice with y)
    ProfScope ps("lstm_window_pairs_kernel", (double)p.R * H, 4.0 * H * p.R * (y ? 4.0 : 3.0), s);
    launch_lstm_window_pairs(b.hf, W, S, b.hm, y, s);
  }
  if (mel_norm) {
    StageTag head("head");
    ProfScope ps("mel_head_kernel", 2.0 * p.R * H * n_mels_, 4.0 * p.R * (H + n_mels_), s);
    launch_mel_head(b.hm, (int)p.R, H, static_cast<const float*>(arena_.ptr(p_.head_wt)),
                    static_cast<const float*>(arena_.ptr(p_.head_b)), n_mels_, mel_norm, s, true);
  }
}

void Acoustic::forward_pairs(const float* frames, const int* lengths, int B, long N, int H, int W, int window,
                             float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  pairs_plan(lengths, B, N, window);  // before the CNN launches
  ragged_check_stream(s);
  float* feats = feats_buf(ws, (size_t)N);
  effnet(frames, (int)N, H, W, feats, -1, nullptr, nullptr, ws, s);
  bilstm_pairs(feats, lengths, B, N, window, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Vocoder
Vocoder::Vocoder(const StateDict& sd, const m2s_hifigan_h& h, int dtype, int device)
    : h_(h), dtype_(dtype), device_(device) {
  for (auto [name, v] : std::initializer_list<std::pair<const char*, bool*>>{
           {"M2S_MRF_FUSED", &mrf_fused_}, {"M2S_MRF_BATCH", &mrf_batch_}, {"M2S_MRF_HALO", &mrf_halo_},
           {"M2S_F8_MRF64", &f8_mrf64_},   {"M2S_F8_MRF32", &f8_mrf32_},   {"M2S_MRF_PAIR", &mrf_pair_},
           {"M2S_MRF_CHAIN", &mrf_chain_}, {"M2S_MRF_PAIR128", &mrf_pair128_}})
    env_flag(name, *v);
  pack_vocoder(sd, h, dtype, f8_mrf64_, f8_mrf32_, arena_, p_, mrf_pair_ && mrf_pair128_);
  arena_.upload(device);
  p_.pre.resolve(arena_);
  for (auto& u : p_.ups) u.resolve(arena_);
  for (auto& rb : p_.rbs) {
    for (auto& c : rb.c1) c.resolve(arena_);
    for (auto& c : rb.c2) c.resolve(arena_);
    for (size_t o : rb.f1_off) rb.f1.push_back(static_cast<const bf16_t*>(arena_.ptr(o)));
    for (size_t o : rb.f2_off) rb.f2.push_back(static_cast<const bf16_t*>(arena_.ptr(o)));
    for (size_t o : rb.h1_off) rb.h1.push_back(static_cast<const bf16_t*>(arena_.ptr(o)));
    for (size_t o : rb.h2_off) rb.h2.push_back(static_cast<const bf16_t*>(arena_.ptr(o)));
    for (auto* qv : {&rb.q1, &rb.q2})
      for (RB::F8& f : *qv) {
        f.wp = arena_.ptr(f.w);
        f.sp = static_cast<const float*>(arena_.ptr(f.s));
        f.bp = static_cast<const float*>(arena_.ptr(f.b));
      }
  }
}

size_t Vocoder::act_elems(int B, int T) const {
  size_t m = (size_t)B * T * chan_stride(h_.upsample_initial_channel);
  size_t L = T;
  for (int i = 0; i < h_.n_up; ++i) {
    L *= h_.upsample_rates[i];
    m = std::max(m, (size_t)B * L * chan_stride(h_.upsample_initial_channel >> (i + 1)));
  }
  return m;
}

void* Vocoder::mel_in(Workspace& ws, int B, int T) const {
  return ws.take<char>((size_t)B * T * chan_stride(h_.num_mels) * act_bytes(dtype_));
}

template <typename T>
Vocoder::GenBufs<T> Vocoder::gen_bufs(Workspace& ws, int B, int T_) const {
  const size_t n = act_elems(B, T_) * Elem<T>::R;
  GenBufs<T> g{};
  g.X = ws.take<T>(n);
  for (T*& h : g.Hb) h = ws.take<T>(n);
  g.T1 = ws.take<T>(n);
  g.S = ws.take<T>(n);
  if (dtype_ == M2S_DT_FP8) g.E8 = ws.take<T>(n);
  if (std::is_same<T, sp_t>::value)
    for (auto& bt : g.Bt)
      for (T*& q : bt) q = ws.take<T>(n);
  return g;
}

void Vocoder::gen_ws(Workspace& ws, int B, int T) const {
  dispatch_act(dtype_, [&](auto t) { gen_bufs<typename decltype(t)::type>(ws, B, T); });
}

size_t Vocoder::workspace_bytes(int B, int T) const {
  return Workspace::bytes([&](Workspace& ws) {
    mel_in(ws, B, T);
    gen_ws(ws, B, T);
  });
}

void Vocoder::forward(const float* mel, int layout, int B, int T, float* wav, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "vocoder: empty input");
  void* mn = mel_in(ws, B, T);
  dispatch_act(dtype_, [&](auto t) {
    using A = typename decltype(t)::type;
    launch_mel_to_nlc<A>(mel, B, h_.num_mels, T, layout, static_cast<A*>(mn), chan_stride(h_.num_mels), s);
    run_t<A>(mn, B, T, wav, ws, s);
  });
}

void Vocoder::forward_from_norm(const float* mel_norm, const float* mean, const float* std_, int B, int T,
                                float* mel_db, float* mel_log, void* ln_buf, float* wav, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "vocoder: empty input");
  const int nm = h_.num_mels, cs = chan_stride(nm);
  mel_in(ws, B, T);  // unused here (the input is ln_buf): the generator's buffers sit where forward() puts them
  StageTag tag("glue");
  dispatch_act(dtype_, [&](auto t) {
    using A = typename decltype(t)::type;
    {
      ProfScope ps(tname<A>("mel_glue_kernel"), 0.0, 4.0 * B * T * nm * 4, s);
      launch_mel_glue<A>(mel_norm, B * T, nm, mean, std_, mel_db, mel_log, static_cast<A*>(ln_buf), cs, s);
    }
    run_t<A>(ln_buf, B, T, wav, ws, s);
  });
}

// Ragged batches.  Workspace: clip table, padded ln-mel, padded wav, then the generator's buffers for (B, Tmax).
Vocoder::RaggedBufs Vocoder::ragged_bufs(Workspace& ws, int B, int Tmax, int tab_cols) const {
  RaggedBufs b{};
  b.tab = ws.take<int>((size_t)tab_cols * B);
  b.ln_buf = mel_in(ws, B, Tmax);
  b.wav_pad = ws.take<float>((size_t)B * Tmax * p_.hop);
  return b;
}

size_t Vocoder::ragged_workspace_bytes(const int* lengths, int B) const {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  const RaggedDims d = ragged_dims(lengths, B, n);
  return Workspace::bytes([&](Workspace& ws) {
    ragged_bufs(ws, B, d.Tmax);
    gen_ws(ws, B, d.Tmax);
  });
}

void Vocoder::ragged_run(const float* x, const float* mean, const float* std_, const int* lengths, int B, long N,
                         float* mel_db, float* mel_log, float* wav, Workspace& ws, hipStream_t s) {
  const RaggedDims d = ragged_dims(lengths, B, N);
  const int nm = h_.num_mels, cs = chan_stride(nm), T = d.Tmax;
  const RaggedBufs rb = ragged_bufs(ws, B, T);
  int* const tab = rb.tab;
  float* const wav_pad = rb.wav_pad;
  rtab_.upload(lengths, B, tab, s);
  // the masks write only where a clip is shorter than Tmax: with equal lengths the generator runs as the dense call
  const int* mask_tab = d.Tmin < T ? tab : nullptr;
  dispatch_act(dtype_, [&](auto t) {
    using A = typename decltype(t)::type;
    {
      StageTag tag("glue");
      ProfScope ps(tname<A>("ragged_glue_kernel"), 0.0, 4.0 * N * nm * (mean ? 4 : 2), s);
      launch_ragged_glue<A>(x, tab, B, T, nm, mean, std_, mel_db, mel_log, static_cast<A*>(rb.ln_buf), cs, s);
    }
    run_t<A>(rb.ln_buf, B, T, wav_pad, ws, s, mask_tab);
  });
  StageTag tag("voc_post");
  ProfScope ps("ragged_wav_pack_kernel", 0.0, 2.0 * 4.0 * N * p_.hop, s);
  launch_ragged_wav_pack(wav_pad, tab, B, T, p_.hop, wav, s);
}

void Vocoder::forward_ragged(const float* mel, const int* lengths, int B, long N, float* wav, Workspace& ws,
                             hipStream_t s) {
  ragged_run(mel, nullptr, nullptr, lengths, B, N, nullptr, nullptr, wav, ws, s);
}

void Vocoder::forward_from_norm_ragged(const float* mel_norm, const float* mean, const float* std_, const int* lengths,
                                       int B, long N, float* mel_db, float* mel_log, float* wav, Workspace& ws,
                                       hipStream_t s) {
  M2S_CHECK(mean && std_, "vocoder: null mel statistics");
  ragged_run(mel_norm, mean, std_, lengths, B, N, mel_db, mel_log, wav, ws, s);
}

// Streaming: the stateless chunk call (vocoder_chunk.hip, DESIGN.md "Streaming vocoder").
Vocoder::ChunkPlan Vocoder::chunk_plan(const int* lengths, const int* context, const int* hold, int B,
                                       long rows) const {
  ChunkPlan p;
  p.d = ragged_dims(lengths, B, rows);
  M2S_CHECK(context && hold, "chunk: context and hold must not be null");
  const int nl = h_.n_up, T = p.d.Tmax;
  // A cropped block's edge is a fake clip end: what it contaminates must lie in rows no emitted sample depends on.
  // That holds on the left when every clip brings the full history, on the right when every clip holds the full
  // look-ahead back; otherwise that side keeps its rows, and its ends are clip ends (tail masks as in ragged calls)
  bool left = chunk_cone_, right = chunk_cone_;
  int cmin = T;
  for (int b = 0; b < B; ++b) {
    const std::string c = "chunk: clip " + std::to_string(b);
    M2S_CHECK(context[b] >= 0 && hold[b] >= 0, c + ": context and hold must be >= 0");
    M2S_CHECK((long)context[b] + hold[b] < lengths[b],
              c + ": context " + std::to_string(context[b]) + " + hold " + std::to_string(hold[b]) +
                  " leaves no row of its " + std::to_string(lengths[b]) + " to emit");
    left = left && context[b] >= p_.back;
    right = right && hold[b] >= p_.ahead;
    cmin = std::min(cmin, context[b]);
  }
  p.mask = !right && p.d.Tmin < T;
  p.tab.assign((size_t)(5 + nl) * B, 0);
  int start = 0, rows_now = T;  // the block as it stands: rows start .. start + rows_now - 1 of every span
  for (int l = 0; l < nl; ++l) {
    int s0 = left ? cmin - p_.lvl_back[l] : 0, e0 = start + rows_now;
    if (right) {
      int need = 0;
      for (int b = 0; b < B; ++b) need = std::max(need, lengths[b] - hold[b] + p_.lvl_ahead[l]);
      e0 = std::min(e0, need);
    }
    s0 = std::max(s0, start);
    p.drop[l] = s0 - start;
    p.keep[l] = e0 - s0;
    p.crop = p.crop || p.drop[l] != 0 || p.keep[l] != rows_now;
    start = s0;
    rows_now = e0 - s0;
    for (int b = 0; b < B; ++b) p.tab[(size_t)(5 + l) * B + b] = lengths[b] - start;
  }
  p.t_final = rows_now;
  int off = 0;
  for (int b = 0; b < B; ++b) {
    const int n = lengths[b] - context[b] - hold[b];
    p.tab[b] = off;
    p.tab[(size_t)B + b] = lengths[b];
    p.tab[(size_t)2 * B + b] = context[b] - start;
    p.tab[(size_t)3 * B + b] = (int)p.out_rows;
    p.tab[(size_t)4 * B + b] = n;
    off += lengths[b];
    p.out_rows += n;
  }
  return p;
}


size_t Vocoder::chunk_workspace_bytes(const int* lengths, const int* context, const int* hold, int B) const {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  const ChunkPlan p = chunk_plan(lengths, context, hold, B, n);
  return Workspace::bytes([&](Workspace& ws) {
    ragged_bufs(ws, B, p.d.Tmax, 5 + h_.n_up);
    gen_ws(ws, B, p.d.Tmax);
  });
}

void Vocoder::forward_chunk(const float* mel, const int* lengths, const int* context, const int* hold, int B, long N,
                            float* wav, Workspace& ws, hipStream_t s) {
  const ChunkPlan p = chunk_plan(lengths, context, hold, B, N);
  const int nm = h_.num_mels, cs = chan_stride(nm), T = p.d.Tmax;
  const RaggedBufs cb = ragged_bufs(ws, B, T, 5 + h_.n_up);
  rtab_.upload_ints(p.tab.data(), p.tab.size(), cb.tab, s);
  Cone cone{};
  for (int l = 0; l < h_.n_up; ++l) {
    cone.drop[l] = p.drop[l];
    cone.keep[l] = p.keep[l];
    // launch_ragged_tail_mask reads clip b's length at tab[B + b]: column 5 + l through a table that starts at 4 + l
    cone.mask[l] = p.mask ? cb.tab + (size_t)(4 + l) * B : nullptr;
  }
  dispatch_act(dtype_, [&](auto t) {
    using A = typename decltype(t)::type;
    {
      StageTag tag("glue");
      ProfScope ps(tname<A>("ragged_glue_kernel"), 0.0, 4.0 * N * nm * 2, s);
      launch_ragged_glue<A>(mel, cb.tab, B, T, nm, nullptr, nullptr, nullptr, nullptr, static_cast<A*>(cb.ln_buf), cs,
                            s);
    }
    run_t<A>(cb.ln_buf, B, T, cb.wav_pad, ws, s, p.mask ? cb.tab : nullptr, p.crop ? &cone : nullptr);
  });
  StageTag tag("voc_post");
  ProfScope ps("chunk_wav_pack_kernel", 0.0, 2.0 * 4.0 * p.out_rows * p_.hop, s);
  const int* const emit = cb.tab + (size_t)2 * B;  // [src | dst | n]
  launch_chunk_wav_pack(cb.wav_pad, emit, emit + B, emit + (size_t)2 * B, B, p.t_final, p_.hop, wav, s);
}

constexpr int CONV_POST_TAPS = 7;  // conv_post: Conv1d(C, 1, 7) behind a right pad of 6 (launch_conv_post)

// Split-fp32 ResBlock1 stage with the resblocks batched (conv_gemm batch launches, grid.z = resblock):
// X holds a0 = lrelu(x) (the upsampler's epilogue applied it), so no conv re-applies LeakyReLU to its
// operand fragments per K step; each c2 recovers its residual x from lrelu(x) (slope 0.1 is
// invertible: x = a > 0 ? a : 10 a) and stores lrelu(xt + x) for the next pair's c1.  Per pair:
// one launch for the c1 of every resblock, one for the c2 (the last pair's c2 accumulates the MRF
// sum S = (x_0 + x_1 + ...) / num_kernels in resblock order, models.py:119-125, so it stays serial).
// C = 64 (M2S_MRF_PAIR): one launch per pair instead, c1 and c2 fused with the tensor between them in LDS
// (conv1d_halo_pair_kernel); the last pairs chained in one launch where the pass fills the chip.
template <typename T>
void Vocoder::mrf_stage_batched(int i, const T* X, T* S, T* const (*Bt)[3], int B, int L, bool act_out,
                                hipStream_t s) {
  const int nk = h_.n_kernels, np = (int)p_.rbs[i * nk].dil.size();
  int ord[CONV_BATCH];
  for (int j = 0; j < nk; ++j) ord[j] = j;
  std::sort(ord, ord + nk, [&](int x, int y) { return p_.rbs[i * nk + x].c1[0].kp > p_.rbs[i * nk + y].c1[0].kp; });
  auto a_in = [&](int j, int p) -> const T* { return p == 0 ? X : Bt[j][1 + ((p - 1) & 1)]; };  // lrelu(x) of pair p
  bool halo = mrf_halo_;  // input rows staged once per tile (conv1d_halo.hip) where the stage has the weights for it
  for (int j = 0; j < nk; ++j) halo = halo && !p_.rbs[i * nk + j].h1.empty();
  // each (c1, c2) pair in one launch (conv1d_halo_pair_kernel) where every pair of the stage is within its reach;
  // a stage with one that is not runs as a whole on the launches below
  const int C = p_.ups[i].cout;
  bool pair = halo && mrf_pair_ && std::is_same<T, sp_t>::value && (C == 64 || mrf_pair128_);
  for (int j = 0; j < nk && pair; ++j)
    for (int d : p_.rbs[i * nk + j].dil) pair = pair && conv1d_halo_pair_supported(C, chan_stride(C), p_.rbs[i * nk + j].k, d);
  for (int j = 0; j < nk; ++j)  // C = 128 has the fragments for the pair kernel only
    for (int d : p_.rbs[i * nk + j].dil) halo = halo && conv1d_halo_sp_supported(C, chan_stride(C), p_.rbs[i * nk + j].k, d);
  if (pair) {
    const double es = sizeof(T) * Elem<T>::R, act = es * B * L * C;
    auto make = [&](int j, int p, double* fl, double* by) {
      const RB& rb = p_.rbs[i * nk + j];
      HaloPair h{};
      h.x = a_in(j, p);
      h.w1 = rb.h1[p];
      h.w2 = rb.h2[p];
      h.b1 = conv_args(rb.c1[p]).bias;
      h.b2 = conv_args(rb.c2[p]).bias;
      h.k = rb.k;
      h.dil = rb.dil[p];
      *fl += 2.0 * (rb.c1[p].macs_per_row + rb.c2[p].macs_per_row) * B * L;
      *by += act + es * 2.0 * C * C * rb.k;  // x in, both weight sets; the caller adds what is stored
      return h;
    };
    for (int p = 0; p + 1 < np; ++p) {  // a_{p+1} = lrelu(x + xt) of every resblock, longest K first
      HaloPair hp[CONV_BATCH];
      double fl = 0.0, by = 0.0;
      for (int jj = 0; jj < nk; ++jj) {
        hp[jj] = make(ord[jj], p, &fl, &by);
        hp[jj].y = Bt[ord[jj]][1 + (p & 1)];
        hp[jj].act = 1;
        by += act;
      }
      launch_conv1d_halo_pair(hp, nk, C, B, L, false, 1.f, s, fl, by);
    }
    // the last pairs in resblock order: xs = sum_j resblock_j(x); S = xs / num_kernels, lrelu'd for an upsampler
    HaloPair hp[CONV_BATCH];
    double fl = 0.0, by = 0.0;
    const bool chain = mrf_chain_ && conv1d_halo_pair_fills(C, B, L);
    for (int j = 0; j < nk; ++j) {
      double f = 0.0, b = 0.0;
      hp[j] = make(j, np - 1, &f, &b);
      hp[j].y = S;
      hp[j].accum = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
      hp[j].act = act_out && j == nk - 1;
      if (!chain) launch_conv1d_halo_pair(&hp[j], 1, C, B, L, false, (float)nk, s, f, b + act * (hp[j].accum ? 2 : 1));
      fl += f;
      by += b;
    }
    if (chain) launch_conv1d_halo_pair(hp, nk, C, B, L, true, (float)nk, s, fl, by + act);
    return;
  }
  auto launch_batch = [&](ConvArgs* cs, int n, double fl, double by) {
    if (halo)
      launch_conv1d_halo_sp(cs, n, s, fl, by);
    else
      launch_conv_gemm_batch(cs, n, s, fl, by);
  };
  for (int p = 0; p < np; ++p) {
    ConvArgs cs[CONV_BATCH];
    double fl = 0.0, by = 0.0, f, b;
    for (int jj = 0; jj < nk; ++jj) {
      const int j = ord[jj];
      const RB& rb = p_.rbs[i * nk + j];
      ConvArgs c = conv_args(rb.c1[p]);
      if (halo) c.w = rb.h1[p];
      c.x = a_in(j, p);
      c.y = Bt[j][0];
      c.L_in = c.L_out = L;
      c.M = B * L;
      c.act = ACT_LRELU;
      c.act_slope = 0.1f;
      conv_cost<T>(c, rb.c1[p], &f, &b);
      fl += f;
      by += b;
      cs[jj] = c;
    }
    launch_batch(cs, nk, fl, by);
    fl = by = 0.0;
    for (int jj = 0; jj < nk; ++jj) {
      const int j = p + 1 < np ? ord[jj] : jj;
      const RB& rb = p_.rbs[i * nk + j];
      ConvArgs c = conv_args(rb.c2[p]);
      if (halo) c.w = rb.h2[p];
      c.x = Bt[j][0];
      c.res = a_in(j, p);
      c.res_unslope = 10.f;
      c.L_in = c.L_out = L;
      c.M = B * L;
      if (p + 1 < np) {  // a_{p+1} = lrelu(xt + x)
        c.y = Bt[j][1 + (p & 1)];
        c.act = ACT_LRELU;
        c.act_slope = 0.1f;
        c.act_after_res = 1;
        conv_cost<T>(c, rb.c2[p], &f, &b);
        fl += f;
        by += b;
        cs[jj] = c;
      } else {  // xs = sum_j resblock_j(x); x = xs / num_kernels
        c.y = S;
        c.accum = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
        c.accum_div = (float)nk;
        if (act_out && j == nk - 1) {  // S = lrelu(xs / num_kernels) for the next upsampler
          c.act = ACT_LRELU;
          c.act_slope = 0.1f;
          c.act_after_res = 1;
        }
        if (halo) {
          conv_cost<T>(c, rb.c2[p], &f, &b);
          launch_conv1d_halo_sp(&c, 1, s, f, b);
        } else {
          run_conv<T>(c, rb.c2[p], s);
        }
      }
    }
    if (p + 1 < np) launch_batch(cs, nk, fl, by);
  }
}

template <typename T>
void Vocoder::run_t(const void* mel_nlc, int B, int Tn, float* wav, Workspace& ws, hipStream_t s, const int* tab,
                    const Cone* cone) {
  constexpr bool SPL = std::is_same<T, sp_t>::value;
  int Tc = Tn;              // rows per clip of the block as it stands (a cone shortens it between stages)
  const int* mtab = tab;    // ... and the clip table its tail masks read
  // ragged calls: zero the `halo` rows of S that the next consumer reads past the end of a short clip (they hold
  // biases and resblock outputs of the padding; lrelu(0) = 0, so masking before the activation is equivalent)
  auto mask_tail = [&](T* S, int L, int halo, int cs) {
    if (!mtab || halo <= 0) return;
    const size_t row_bytes = sizeof(T) * Elem<T>::R * (size_t)cs;
    ProfScope ps("ragged_tail_mask_kernel", 0.0, (double)B * halo * row_bytes, s);
    launch_ragged_tail_mask(S, mtab, B, L, L / Tc, halo, row_bytes, s);
  };
  const GenBufs<T> g = gen_bufs<T>(ws, B, Tn);
  T *const X = g.X, *const *const Hb = g.Hb, *const T1 = g.T1, *const S = g.S, *const E8 = g.E8;
  T* const(*Bt)[3] = g.Bt;
  int L = Tn;
  const int nk = h_.n_kernels;
  // chunk calls: level l of the cone, on S as conv_pre (l = 0) or the MRF of stage l - 1 left it.  The kept rows go
  // to Hb[0], which nothing holds between an MRF stage and the next upsampler
  T* Sin = S;
  auto crop = [&](int l) {
    Sin = S;
    if (!cone) return;
    mtab = cone->mask[l];
    if (cone->drop[l] == 0 && cone->keep[l] == Tc) return;
    const long scale = L / Tc, keep = cone->keep[l] * scale;
    const size_t row_bytes = sizeof(T) * Elem<T>::R * (size_t)p_.ups[l].cs_in;
    StageTag tag("glue");
    ProfScope ps("crop_rows_kernel", 0.0, 2.0 * B * keep * row_bytes, s);
    launch_crop_rows(S, B, L, cone->drop[l] * scale, keep, row_bytes, Hb[0], s);
    Sin = Hb[0];
    Tc = cone->keep[l];
    L = (int)keep;
  };
  auto is_batched = [&](int i) {  // stage i's MRF runs as batched split launches (mrf_stage_batched)
    const PConv& up = p_.ups[i];
    const bool fused = (std::is_same<T, bf16_t>::value || SPL) && mrf_fused_ && !p_.rbs[i * nk].f1.empty();
    bool b = SPL && mrf_batch_ && !fused && h_.resblock == 1 && nk <= CONV_BATCH && up.cout >= 32 && up.cout % 32 == 0;
    for (int j = 0; j < nk; ++j) b = b && p_.rbs[i * nk + j].dil.size() == p_.rbs[i * nk].dil.size();
    return b;
  };
  // split: the upsampler's input S may already hold lrelu(x) (slope 0.1, models.py:116-117), written so
  // by its producer's epilogue (conv_pre, or a batched stage's final MRF accumulation), so the
  // upsampler does not re-apply LeakyReLU to its operand fragments every K step
  bool s_act = SPL;
  {
    StageTag tag("voc_pre");
    ConvArgs a = conv_args(p_.pre);
    a.x = mel_nlc;
    a.y = S;
    a.L_in = L;
    a.L_out = L;
    a.M = B * L;
    if (s_act) {
      a.act = ACT_LRELU;
      a.act_slope = 0.1f;
    }
    run_conv<T>(a, p_.pre, s);
  }
  for (int i = 0; i < h_.n_up; ++i) {
    const PConv& up = p_.ups[i];
    const bool batched = is_batched(i);
    crop(i);
    StageTag tag("ups_c" + std::to_string(up.cout));
    // a transposed conv of rate u and padding p reads floor((u - 1 + p) / u) input rows ahead of its output
    mask_tail(Sin, L, (up.ct_u - 1 + up.ct_pad) / up.ct_u, up.cs_in);
    ConvArgs a = conv_args(up);
    a.x = Sin;
    a.y = X;
    a.L_in = L;
    a.L_out = L * up.ct_u;
    a.M = B * L;  // rows per phase
    if (!s_act) {
      a.in_xform = IN_LRELU;
      a.in_slope = 0.1f;
    }
    if (batched) {  // X = lrelu(upsampled x): the MRF convs read it as is (mrf_stage_batched)
      a.act = ACT_LRELU;
      a.act_slope = 0.1f;
    }
    run_conv<T>(a, up, s);
    L *= up.ct_u;
    StageTag mrf("mrf_c" + std::to_string(up.cout));  // the stage's MRF (ResBlocks + sum), models.py:119-125
    if (batched) {
      // the last accumulation stores lrelu(S) when the next consumer is an upsampler (conv_post
      // takes F.leaky_relu's default slope 0.01 on the raw S)
      s_act = i + 1 < h_.n_up;
      mrf_stage_batched<T>(i, X, S, Bt, B, L, s_act, s);
      continue;
    }
    s_act = false;
    // every resblock of the stage must carry e4m3 weights (q8 is decided per resblock: k <= 31)
    bool stage_f8 = std::is_same<T, bf16_t>::value;
    for (int j = 0; j < nk && stage_f8; ++j) {
      const RB& rb = p_.rbs[i * nk + j];
      stage_f8 = rb.q1.size() == rb.dil.size() && rb.q2.size() == rb.dil.size() && !rb.dil.empty();
    }
    if (stage_f8) {
      // fp8 stage (C = 128 / 256): e4m3 operands.  X8 = e4m3(lrelu(x)) once; per pair, c1 stores only
      // e4m3(lrelu(xt)) (its sole consumer is c2), c2 adds the bf16 residual and stores x (bf16, the next
      // residual) and e4m3(lrelu(x)) (the next c1's operand); the last c2 accumulates the MRF sum in S.
      const int C = up.cout;
      const long nel = (long)B * L * C;
      uint8_t* X8 = reinterpret_cast<uint8_t*>(T1);  // T1 (2 bytes / element) holds X8 and T8
      uint8_t* T8 = X8 + nel;
      uint8_t* H8[2] = {reinterpret_cast<uint8_t*>(E8), reinterpret_cast<uint8_t*>(E8) + nel};
      {
        ProfScope ps("lrelu_e4m3_kernel", 0.0, 3.0 * nel, s);
        launch_lrelu_e4m3(reinterpret_cast<const bf16_t*>(X), X8, nel, 0.1f, s);
      }
      const double rows = (double)B * L;
      for (int j = 0; j < nk; ++j) {
        const RB& rb = p_.rbs[i * nk + j];
        const int np = (int)rb.dil.size();
        const bf16_t* cur = reinterpret_cast<const bf16_t*>(X);
        const uint8_t* cur8 = X8;
        for (int p = 0; p < np; ++p) {
          const double fl = 2.0 * rows * C * C * rb.k, wb = (double)C * C * rb.k;
          launch_conv1d_f8(cur8, B, L, C, rb.k, rb.dil[p], rb.q1[p].wp, rb.q1[p].sp, rb.q1[p].bp, nullptr, nullptr, T8,
                           0.1f, 0, 1.f, s, fl, 2.0 * nel + wb);
          if (p == np - 1) {
            const int accum = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
            launch_conv1d_f8(T8, B, L, C, rb.k, 1, rb.q2[p].wp, rb.q2[p].sp, rb.q2[p].bp, cur, S, nullptr, 0.f, accum,
                             (float)nk, s, fl, nel * (1.0 + 2.0 + 2.0 + (accum ? 2.0 : 0.0)) + wb);
          } else {
            bf16_t* xo = reinterpret_cast<bf16_t*>(Hb[p & 1]);
            launch_conv1d_f8(T8, B, L, C, rb.k, 1, rb.q2[p].wp, rb.q2[p].sp, rb.q2[p].bp, cur, xo, H8[p & 1], 0.1f, 0,
                             1.f, s, fl, nel * (1.0 + 2.0 + 2.0 + 1.0) + wb);
            cur = xo;
            cur8 = H8[p & 1];
          }
        }
      }
      continue;
    }
    for (int j = 0; j < nk; ++j) {
      const RB& rb = p_.rbs[i * nk + j];
      const T* hcur = X;
      const int np = (int)rb.dil.size();
      const int accum = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
      if ((std::is_same<T, bf16_t>::value || SPL) && mrf_fused_ && !rb.f1.empty()) {
        // one launch for the whole resblock + MRF sum (mrf_fused.hip)
        const bf16_t* w1[8];
        const bf16_t* w2[8];
        const float* b1[8];
        const float* b2[8];
        double macs = 0.0;
        for (int p = 0; p < np; ++p) {
          w1[p] = rb.f1[p];
          w2[p] = rb.f2[p];
          b1[p] = rb.c1[p].b;
          b2[p] = rb.c2[p].b;
          macs += rb.c1[p].macs_per_row + rb.c2[p].macs_per_row;
        }
        const int C = rb.c1[0].cout;
        const double rows = (double)B * L;
        const double bytes = (SPL ? 2.0 : 1.0) * (2.0 * rows * C * (2 + (accum ? 1 : 0)) + 2.0 * np * 2 * C * C * rb.k);
        launch_rb1_fused(reinterpret_cast<const bf16_t*>(X), reinterpret_cast<bf16_t*>(S), B, L, C, rb.k, np,
                         rb.dil.data(), w1, b1, w2, b2, rb.c1[0].kp, accum, (float)nk, SPL, 2.0 * macs * rows, bytes,
                         s);
        continue;
      }
      for (int p = 0; p < np; ++p) {
        const bool last = p == np - 1;
        T* out = last ? S : Hb[p & 1];
        ConvArgs c = conv_args(rb.c1[p]);
        c.x = hcur;
        c.L_in = L;
        c.L_out = L;
        c.M = B * L;
        c.in_xform = IN_LRELU;
        c.in_slope = 0.1f;
        if (h_.resblock == 1) {  // xt = c2(lrelu(c1(lrelu(x)))) ; x = xt + x
          c.y = T1;
          c.act = ACT_LRELU;
          c.act_slope = 0.1f;
          run_conv<T>(c, rb.c1[p], s);
          c = conv_args(rb.c2[p]);
          c.x = T1;
          c.L_in = L;
          c.L_out = L;
          c.M = B * L;
        }
        c.y = out;
        c.res = hcur;
        if (last) {  // xs = sum_j resblock_j(x); x = xs / num_kernels (models.py:119-125)
          c.accum = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
          c.accum_div = (float)nk;
        }
        run_conv<T>(c, h_.resblock == 1 ? rb.c2[p] : rb.c1[p], s);
        hcur = out;
      }
    }
  }
  StageTag tag("voc_post");
  mask_tail(S, L, CONV_POST_TAPS - 1, chan_stride(p_.post_c));
  ProfScope ps(tname<T>(p_.post_c <= 64 ? "conv_post_tile_kernel" : "conv_post_kernel"), 2.0 * B * L * p_.post_c * 7, (sizeof(T) * Elem<T>::R) * (double)B * L * p_.post_c + 4.0 * B * L, s);
  launch_conv_post<T>(S, B, L, p_.post_c, chan_stride(p_.post_c), static_cast<const float*>(arena_.ptr(p_.post_w)), p_.post_b,
                      wav, s);
}

// ------------------------------------------------------------------------------------------
// Pipeline scratch (capi.cpp: the size queries and m2s_pipeline_forward(_ragged))
PipelineBufs pipeline_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, int B, int T, int H, int W) {
  const size_t rows = (size_t)B * T;
  PipelineBufs b{};
  b.mn = ws.take<float>(rows * a.n_mels());
  b.ln_t = ws.take<char>(rows * chan_stride(a.n_mels()) * 4);
  b.rest_bytes = std::max(a.workspace_bytes(B, T, H, W), v.workspace_bytes(B, T));
  b.rest = ws.take<char>(b.rest_bytes);
  return b;
}

PipelineBufs pipeline_ragged_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, const int* lengths, int B, int H,
                                  int W) {
  PipelineBufs b{};
  b.rest_bytes = std::max(a.ragged_workspace_bytes(lengths, B, H, W), v.ragged_workspace_bytes(lengths, B));
  size_t rows = 0;
  for (int i = 0; i < B; ++i) rows += (size_t)lengths[i];
  b.mn = ws.take<float>(rows * a.n_mels());
  b.rest = ws.take<char>(b.rest_bytes);
  return b;
}

}  // namespace m2s
