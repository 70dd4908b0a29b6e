// Execution plan of the HiFi-GAN generator: the stage loop that executes the route table (voc_route.hpp: which
// kernel runs for which stage, dtype and switch, planned once in the constructor), the scratch layouts, and the
// ragged and chunk calls.  The weights are packed by pack_vocoder.cpp (host code); the constructor
// here reads the switches, packs, uploads the arena and resolves device pointers.
#include <algorithm>

#include "plan_util.hpp"
#include "prof.hpp"

namespace m2s {

Vocoder::Vocoder(const StateDict& sd, const m2s_hifigan_h& h, int dtype, int device)
    : h_(h), dtype_(dtype), device_(device), sw_(Switches::from_env()), wants_(voc_pack_wants(h, dtype, sw_)),
      route_(voc_route(h, dtype, sw_, wants_)) {
  pack_vocoder(sd, h, dtype, wants_, arena_, p_);
  arena_.upload(device);
  p_.pre.resolve(arena_);
  for (auto& u : p_.ups) u.resolve(arena_);
  for (auto& rb : p_.rbs) rb.resolve(arena_);
  // a route whose kernel reads a copy the packer did not stage is refused here, once, not found at a launch
  for (size_t q = 0; q < p_.rbs.size(); ++q) {
    const StageRoute& r = route_.stages[q / h.n_kernels];
    const RB& rb = p_.rbs[q];
    const size_t np = rb.dil.size();
    const bool fused = r.mrf == MrfRoute::PerResblock && r.rb[q % h.n_kernels] == RbRoute::Fused;
    const bool halo = r.mrf == MrfRoute::Pair || r.mrf == MrfRoute::HaloBatched, f8 = r.mrf == MrfRoute::F8;
    M2S_CHECK((!fused || rb.f2.size() == np) && (!halo || rb.h2.size() == np) && (!f8 || (dtype == M2S_DT_FP8 && rb.q2.size() == np)),
              "vocoder: stage " + std::to_string(q / h.n_kernels) + " is routed to a kernel whose weights were not packed");
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
  if (kSplit<T>)
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

bool Vocoder::tap_info(int tap, int T, int* L, int* C) const {
  M2S_CHECK(tap >= 0 && tap <= 2 * h_.n_up, "vocoder probe: tap must be 0 .. 2 * n_up");
  *L = T;
  *C = h_.upsample_initial_channel;
  if (tap == 0) return route_.pre_act_out;
  const int i = (tap - 1) / 2;
  for (int q = 0; q <= i; ++q) *L *= h_.upsample_rates[q];
  *C = h_.upsample_initial_channel >> (i + 1);
  const StageRoute& r = route_.stages[i];
  return tap % 2 ? r.ups_act_out : r.mrf_act_out;
}

void Vocoder::probe(const float* mel, int layout, int B, int T, int tap, float* out, int* L, int* C, int* act,
                    Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "vocoder: empty input");
  int l = 0, c = 0;
  tap_info(tap, T, &l, &c);  // refuses a tap out of range
  void* mn = mel_in(ws, B, T);
  Probe pr{tap, out, 0, 0, false};
  dispatch_act(dtype_, [&](auto t) {
    using A = typename decltype(t)::type;
    launch_mel_to_nlc<A>(mel, B, h_.num_mels, T, layout, static_cast<A*>(mn), chan_stride(h_.num_mels), s);
    run_t<A>(mn, B, T, nullptr, ws, s, nullptr, nullptr, &pr);
  });
  if (L) *L = pr.L;
  if (C) *C = pr.C;
  if (act) *act = pr.act ? 1 : 0;
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
  const RaggedDims d = ragged_dims(lengths, B, sum_lengths(lengths, B));
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
  const ChunkPlan p = chunk_plan(lengths, context, hold, B, sum_lengths(lengths, B));
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

// a 1-D conv of the generator on B clips of L rows (an upsampler's caller sets its longer L_out)
static ConvArgs conv1d_args(const PConv& pc, const void* x, void* y, int B, int L) {
  ConvArgs c = conv_args(pc);
  c.x = x;
  c.y = y;
  c.L_in = c.L_out = L;
  c.M = B * L;
  return c;
}
// the generator's LeakyReLU (slope 0.1, models.py:116-117) as the conv's epilogue
static void lrelu_out(ConvArgs& c) {
  c.act = ACT_LRELU;
  c.act_slope = 0.1f;
}
// ConvArgs::accum of resblock j's last conv: xs = sum_j resblock_j(x), the last one divides by num_kernels
static int mrf_accum(int j, int nk) { return j == 0 ? 0 : (j == nk - 1 ? 2 : 1); }

// Split-fp32 ResBlock1 stage with the resblocks batched (conv_gemm batch launches, grid.z = resblock):
// X holds a0 = lrelu(x) (the upsampler's epilogue applied it), so no conv re-applies LeakyReLU to its
// operand fragments per K step; each c2 recovers its residual x from lrelu(x) (slope 0.1 is
// invertible: x = a > 0 ? a : 10 a) and stores lrelu(xt + x) for the next pair's c1.  Per pair:
// one launch for the c1 of every resblock, one for the c2 (the last pair's c2 accumulates the MRF
// sum S = (x_0 + x_1 + ...) / num_kernels in resblock order, models.py:119-125, so it stays serial); HaloBatched:
// on conv1d_halo_sp, the input rows staged once per tile.  Pair: one launch per pair instead, c1 and c2 fused with the tensor between them in LDS
// (conv1d_halo_pair_kernel); the last pairs chained in one launch where the pass fills the chip.
template <typename T>
void Vocoder::mrf_stage_batched(int i, const GenBufs<T>& g, int B, int L, hipStream_t s) {
  const StageRoute& r = route_.stages[i];
  const T* const X = g.X;
  T* const S = g.S;
  T* const(*Bt)[3] = g.Bt;
  const bool pair = r.mrf == MrfRoute::Pair, halo = r.mrf == MrfRoute::HaloBatched, act_out = r.mrf_act_out;
  const int nk = h_.n_kernels, np = (int)p_.rbs[i * nk].dil.size();
  int ord[CONV_BATCH];
  for (int j = 0; j < nk; ++j) ord[j] = j;
  std::sort(ord, ord + nk, [&](int x, int y) { return p_.rbs[i * nk + x].c1[0].kp > p_.rbs[i * nk + y].c1[0].kp; });
  auto a_in = [&](int j, int p) -> const T* { return p == 0 ? X : Bt[j][1 + ((p - 1) & 1)]; };  // lrelu(x) of pair p
  const int C = p_.ups[i].cout;
  if (pair) {
    const double es = kStoreBytes<T>, act = es * B * L * C;
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
    const bool chain = r.chain_wanted && conv1d_halo_pair_fills(C, B, L);
    for (int j = 0; j < nk; ++j) {
      double f = 0.0, b = 0.0;
      hp[j] = make(j, np - 1, &f, &b);
      hp[j].y = S;
      hp[j].accum = mrf_accum(j, nk);
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
      launch_conv_gemm_batch(cs, n, sw_.conv, s, fl, by);
  };
  for (int p = 0; p < np; ++p) {
    ConvArgs cs[CONV_BATCH];
    double fl = 0.0, by = 0.0, f, b;
    for (int jj = 0; jj < nk; ++jj) {
      const int j = ord[jj];
      const RB& rb = p_.rbs[i * nk + j];
      ConvArgs c = conv1d_args(rb.c1[p], a_in(j, p), Bt[j][0], B, L);
      if (halo) c.w = rb.h1[p];
      lrelu_out(c);
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
      ConvArgs c = conv1d_args(rb.c2[p], Bt[j][0], p + 1 < np ? Bt[j][1 + (p & 1)] : S, B, L);
      if (halo) c.w = rb.h2[p];
      c.res = a_in(j, p);
      c.res_unslope = 10.f;
      if (p + 1 < np) {  // a_{p+1} = lrelu(xt + x)
        lrelu_out(c);
        c.act_after_res = 1;
        conv_cost<T>(c, rb.c2[p], &f, &b);
        fl += f;
        by += b;
        cs[jj] = c;
      } else {  // xs = sum_j resblock_j(x); x = xs / num_kernels
        c.accum = mrf_accum(j, nk);
        c.accum_div = (float)nk;
        if (act_out && j == nk - 1) {  // S = lrelu(xs / num_kernels) for the next upsampler
          lrelu_out(c);
          c.act_after_res = 1;
        }
        if (halo) {
          conv_cost<T>(c, rb.c2[p], &f, &b);
          launch_conv1d_halo_sp(&c, 1, s, f, b);
        } else {
          run_conv<T>(c, rb.c2[p], sw_.conv, s);
        }
      }
    }
    if (p + 1 < np) launch_batch(cs, nk, fl, by);
  }
}

// fp8 stage (C = 128 / 256; C = 64 / 32 by switch): e4m3 operands.  X8 = e4m3(lrelu(x)) once; per pair, c1 stores only
// e4m3(lrelu(xt)) (its sole consumer is c2), c2 adds the bf16 residual and stores x (bf16, the next
// residual) and e4m3(lrelu(x)) (the next c1's operand); the last c2 accumulates the MRF sum in S.
template <typename T>
void Vocoder::mrf_stage_f8(int i, const GenBufs<T>& g, int B, int L, hipStream_t s) {
  const T* const X = g.X;
  T *const *const Hb = g.Hb, *const T1 = g.T1, *const S = g.S, *const E8 = g.E8;
  const int nk = h_.n_kernels, C = p_.ups[i].cout;
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
        const int accum = mrf_accum(j, nk);
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
}

// Resblock by resblock: the fused ResBlock1 kernel (one launch for the resblock and its share of the MRF sum,
// mrf_fused.hip) or run_conv pairs, as the route says for each
template <typename T>
void Vocoder::mrf_stage_resblocks(int i, const GenBufs<T>& g, int B, int L, hipStream_t s) {
  constexpr bool SPL = kSplit<T>;
  const StageRoute& r = route_.stages[i];
  T *const X = g.X, *const *const Hb = g.Hb, *const T1 = g.T1, *const S = g.S;
  const int nk = h_.n_kernels;
  for (int j = 0; j < nk; ++j) {
    const RB& rb = p_.rbs[i * nk + j];
    const T* hcur = X;
    const int np = (int)rb.dil.size();
    const int accum = mrf_accum(j, nk);
    if (r.rb[j] == RbRoute::Fused) {
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
      ConvArgs c = conv1d_args(rb.c1[p], hcur, out, B, L);
      c.in_xform = IN_LRELU;
      c.in_slope = 0.1f;
      if (h_.resblock == 1) {  // xt = c2(lrelu(c1(lrelu(x)))) ; x = xt + x
        c.y = T1;
        lrelu_out(c);
        run_conv<T>(c, rb.c1[p], sw_.conv, s);
        c = conv1d_args(rb.c2[p], T1, out, B, L);
      }
      c.res = hcur;
      if (last) {  // xs = sum_j resblock_j(x); x = xs / num_kernels (models.py:119-125)
        c.accum = accum;
        c.accum_div = (float)nk;
      }
      run_conv<T>(c, h_.resblock == 1 ? rb.c2[p] : rb.c1[p], sw_.conv, s);
      hcur = out;
    }
  }
}

template <typename T>
void Vocoder::run_t(const void* mel_nlc, int B, int Tn, float* wav, Workspace& ws, hipStream_t s, const int* tab,
                    const Cone* cone, Probe* probe) {
  int Tc = Tn;              // rows per clip of the block as it stands (a cone shortens it between stages)
  const int* mtab = tab;    // ... and the clip table its tail masks read
  // ragged calls: zero the `halo` rows of S that the next consumer reads past the end of a short clip (they hold
  // biases and resblock outputs of the padding; lrelu(0) = 0, so masking before the activation is equivalent)
  auto mask_tail = [&](T* S, int L, int halo, int cs) {
    if (!mtab || halo <= 0) return;
    const size_t row_bytes = kStoreBytes<T> * (size_t)cs;
    ProfScope ps("ragged_tail_mask_kernel", 0.0, (double)B * halo * row_bytes, s);
    launch_ragged_tail_mask(S, mtab, B, L, L / Tc, halo, row_bytes, s);
  };
  const GenBufs<T> g = gen_bufs<T>(ws, B, Tn);
  T *const *const Hb = g.Hb, *const S = g.S;
  int L = Tn;
  // probe calls: the run ends behind the tapped tensor, copied out as stored (fp32, rows x C), lrelu'd or not as the
  // route's hand-off flag says
  auto tapped = [&](int tap, const T* buf, int C, bool act) {
    if (!probe || probe->tap != tap) return false;
    StageTag tag("probe");
    launch_unpad<T>(buf, (long)B * L, C, chan_stride(C), probe->out, s);
    probe->L = L;
    probe->C = C;
    probe->act = act;
    return true;
  };
  // chunk calls: level l of the cone, on S as conv_pre (l = 0) or the MRF of stage l - 1 left it.  The kept rows go
  // to Hb[0], which nothing holds between an MRF stage and the next upsampler
  T* Sin = S;
  auto crop = [&](int l) {
    Sin = S;
    if (!cone) return;
    mtab = cone->mask[l];
    if (cone->drop[l] == 0 && cone->keep[l] == Tc) return;
    const long scale = L / Tc, keep = cone->keep[l] * scale;
    const size_t row_bytes = kStoreBytes<T> * (size_t)p_.ups[l].cs_in;
    StageTag tag("glue");
    ProfScope ps("crop_rows_kernel", 0.0, 2.0 * B * keep * row_bytes, s);
    launch_crop_rows(S, B, L, cone->drop[l] * scale, keep, row_bytes, Hb[0], s);
    Sin = Hb[0];
    Tc = cone->keep[l];
    L = (int)keep;
  };
  {
    StageTag tag("voc_pre");
    ConvArgs a = conv1d_args(p_.pre, mel_nlc, S, B, L);
    if (route_.pre_act_out) lrelu_out(a);
    run_conv<T>(a, p_.pre, sw_.conv, s);
  }
  if (tapped(0, S, p_.pre.cout, route_.pre_act_out)) return;
  for (int i = 0; i < h_.n_up; ++i) {
    const PConv& up = p_.ups[i];
    const StageRoute& r = route_.stages[i];
    crop(i);
    StageTag tag("ups_c" + std::to_string(up.cout));
    // a transposed conv of rate u and padding p reads floor((u - 1 + p) / u) input rows ahead of its output
    mask_tail(Sin, L, (up.ct_u - 1 + up.ct_pad) / up.ct_u, up.cs_in);
    ConvArgs a = conv1d_args(up, Sin, g.X, B, L);  // M: rows per phase
    a.L_out = L * up.ct_u;
    if (!r.in_act) {  // else the producer's epilogue stored lrelu(x) (slope 0.1, models.py:116-117; voc_route.hpp)
      a.in_xform = IN_LRELU;
      a.in_slope = 0.1f;
    }
    if (r.ups_act_out) lrelu_out(a);  // X = lrelu(upsampled x): a batched stage's convs read it as is
    run_conv<T>(a, up, sw_.conv, s);
    L *= up.ct_u;
    if (tapped(2 * i + 1, g.X, up.cout, r.ups_act_out)) return;
    StageTag mrf("mrf_c" + std::to_string(up.cout));  // the stage's MRF (ResBlocks + sum), models.py:119-125
    switch (r.mrf) {
      case MrfRoute::Pair:
      case MrfRoute::HaloBatched:
      case MrfRoute::GemmBatched: mrf_stage_batched<T>(i, g, B, L, s); break;
      case MrfRoute::F8: mrf_stage_f8<T>(i, g, B, L, s); break;
      case MrfRoute::PerResblock: mrf_stage_resblocks<T>(i, g, B, L, s); break;
    }
    if (tapped(2 * i + 2, S, up.cout, r.mrf_act_out)) return;
  }
  StageTag tag("voc_post");
  mask_tail(S, L, CONV_POST_TAPS - 1, chan_stride(p_.post_c));
  ProfScope ps(tname<T>(p_.post_c <= 64 ? "conv_post_tile_kernel" : "conv_post_kernel"), 2.0 * B * L * p_.post_c * 7, kStoreBytes<T> * (double)B * L * p_.post_c + 4.0 * B * L, s);
  launch_conv_post<T>(S, B, L, p_.post_c, chan_stride(p_.post_c), arena_.at<float>(p_.post_w), p_.post_b, wav, s);
}

}  // namespace m2s
