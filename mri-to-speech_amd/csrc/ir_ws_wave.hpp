// The per-wave form of ir_ws's stride-1 front half on 16-wide maps of at most 16 rows and on 8 x 8 maps (included by
// ir_ws.hip, which has the kernel entry and the launcher): a wave runs expand -> bn1 + SiLU -> depthwise 3x3 -> bn2 + SiLU -> store ->
// squeeze for all pixels of 16 expanded channels of one image by itself, the expanded activation never leaving its
// MFMA accumulators.
//
// The expand MFMA takes A = weights (16 channels x 32 k) and B = 16 positions x 32 k, so lane (g = lane >> 4, r16 =
// lane & 15) of the accumulator of position subtile T holds channels 4g .. 4g + 3 of position 16 T + r16.  On a
// 16-wide map a subtile is one image row: the vertical neighbours of a value are the same lane of the accumulators
// of rows T - 1 and T + 1, the horizontal ones sit one lane away inside the 16-lane DPP row (row_shr:1 / row_shl:1,
// bound_ctrl supplying the zero padding at the left and right edge).  No LDS tile, no second role, no counters, no
// waits that can time out, and the squeeze is an in-lane sum over the rows plus one 16-lane reduction: no atomics,
// the same bits whichever workgroup or wave runs the unit.
//
// Workgroup: 8 waves (two per SIMD, up to 256 registers each), one per CU, owning whole images dealt as in the
// handed-off form (n_full whole images, the tail images in `parts` ranges, here ranges of 16-channel groups).  The
// image's x rows go to LDS once by LDS-DMA in ir_ws's swizzled [pos][hi plane | lo plane] layout (256 positions x
// 512 B = 128 KB, single-buffered: one barrier pair and one DMA wait per image), behind 8 KB of tap slots (one per
// wave); the units (image, 16-channel group) of the image are then dealt round-robin to the waves, which run them
// with no barrier in between.
//
// Arithmetic: the three MFMA terms in ir_ws's order (al bh, ah bl, ah bh) and k-step order, the depthwise as
// b + sum_t w[t] u in tap order with rows outside the image contributing nothing, the squeeze as an in-lane sum
// over the rows and a 16-lane reduction.  Same split fp32 arithmetic as the handed-off form; the compiler contracts
// the tap chains its own way and the squeeze sums in another order, so the two agree to a few 17-bit roundings
// (tests/test_gpu_ir_ws_wave.py), not bit for bit.
//
// The above describes the 16-wide form, ir_ws_wave16; the 8 x 8 form, ir_ws_wave8 (two image rows a subtile, x
// double-buffered), follows it below and shares the unit dealing, the weight fragments and the taps.
#pragma once

// (no namespace of its own: ir_ws.hip includes it inside m2s's unnamed one, after hx_of and the LDS-DMA helpers)

// Ablations (diagnostic builds only, wrong results; tools/build_irws_variants.sh + ab_kern.py): bit 0 no stores of
// the expanded map, bit 1 no depthwise (the second SiLU on the expand's output), bit 2 x rows loaded for a
// workgroup's first image only
#ifndef IRWS_WAVE_ABL
#define IRWS_WAVE_ABL 0
#endif
constexpr int WV_NW = 8;   // waves a workgroup
constexpr int WV_GC = 16;  // expanded channels a unit
constexpr int WV_PF = 5;   // operand ring slots of the expand (k-steps of B fragments in registers)

__device__ __forceinline__ float dpp_left(float v) {  // the value of lane - 1 of the 16-lane row (0 at lane 0)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_right(float v) {  // lane + 1 (0 at lane 15)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xF, 0xF, true));
}
// Work units of a workgroup, dealt round-robin (launch_ir_ws): images 0 .. n_full - 1 whole, then the tail images
// cut into `parts` ranges of 16-channel groups each
struct WvUnit {
  int img, glo, ghi;  // image and group range [glo, ghi)
};
__device__ __forceinline__ WvUnit wv_unit_of(int u, int n_full, int parts, int NG) {
  if (u < n_full) return WvUnit{u, 0, NG};
  const int q = u - n_full, pt = q % parts;
  return WvUnit{n_full + q / parts, pt * NG / parts, (pt + 1) * NG / parts};
}
template <int ROR>
__device__ __forceinline__ float dpp_ror_add(float v) {  // v + the value ROR lanes round the 16-lane row
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + ROR, 0xF, 0xF, false));
}

// The weights of a 16-channel group as MFMA A fragments: lane (g, r16) holds row 16 cg + r16 of W_hi / W_lo, k
// elements 32 ks + 8 g .. + 7 (16 rows x 64 B a load: L2)
template <int KS>
struct WvAFrag {
  bf16x8 h[KS], l[KS];
};
// (lane offsets of the global accesses are rebuilt where they are used, behind an asm barrier: hoisted out of the
// loops they were kept in registers the units need, and spilled)
__device__ __forceinline__ int wv_lane_now(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}
template <int KS>
__device__ __forceinline__ WvAFrag<KS> wv_load_a(const bf16_t* __restrict__ wpw, int cg, int ln) {
  constexpr int CS = KS * 32;
  WvAFrag<KS> a;
  const bf16_t* wr = wpw + ((size_t)(cg * WV_GC + (ln & 15)) * CS * 2 + (ln >> 4) * 8);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    a.h[ks] = *reinterpret_cast<const bf16x8*>(wr + ks * 32);
    a.l[ks] = *reinterpret_cast<const bf16x8*>(wr + CS + ks * 32);
  }
  return a;
}
struct WvTaps {
  float4 w[9], bp, bd;  // the lane's 4 channels: depthwise taps, expand bias, depthwise bias
};
// A unit's taps and biases reach the wave's own 1 KB LDS slot by one LDS-DMA (lane l < 44: row l >> 2 of
// [9 taps | expand bias | depthwise bias], channels 4 (l & 3) ..): a register prefetch of the 11 vectors beside
// the next unit's weights spilled (256 registers, 396 B of scratch)
__device__ __forceinline__ void wv_issue_taps(const float* __restrict__ wdw, const float* __restrict__ bpw,
                                              const float* __restrict__ bdw, const char* zpage, int cs_mid, int cg, int ln,
                                              char* tslot) {
  const int t = ln >> 2, c = cg * WV_GC + 4 * (ln & 3);
  const void* src = t < 9 ? static_cast<const void*>(wdw + (t * cs_mid + c))
                          : t == 9 ? static_cast<const void*>(bpw + c) : t == 10 ? static_cast<const void*>(bdw + c) : zpage;
  dma16_asm(src, lds_lo32_u(tslot));
}
__device__ __forceinline__ WvTaps wv_read_taps(const char* tslot, int g) {
  WvTaps t;
#pragma unroll
  for (int k = 0; k < 9; ++k) t.w[k] = *reinterpret_cast<const float4*>(tslot + k * 64 + g * 16);
  t.bp = *reinterpret_cast<const float4*>(tslot + 9 * 64 + g * 16);
  t.bd = *reinterpret_cast<const float4*>(tslot + 10 * 64 + g * 16);
  return t;
}

// FULL (a 16-row map) and F32 (plain fp32 rows out, else the interleaved split layout) are compile-time, so a unit is
// straight-line code in which the compiler counts its loads and stores exactly (below); one copy of the whole image
// loop per pair, chosen once per launch (with the four unit loops side by side in one image loop the compiler fell
// back to vmcnt(0) at the head of the last one)
template <int KS, bool FULL, bool F32>
__device__ __forceinline__ void ir_ws_wave16(const bf16_t* __restrict__ x, int N, int H, int cs_mid,
                                             const bf16_t* __restrict__ wpw, const float* __restrict__ bpw,
                                             const float* __restrict__ wdw, const float* __restrict__ bdw,
                                             bf16_t* __restrict__ y, bf16_t* __restrict__ se_mean, int n_full, int parts) {
  constexpr int W = 16, HMAX = 16;
  constexpr int CS = KS * 32;  // input channel stride = expand K
  constexpr int CPP = (CS * 2 + 255) / 256 * 16;
  constexpr int CPR = 2 * CPP;  // 16-byte chunks per LDS x row
  constexpr int XP = CPR * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* xs = smem + WV_NW * 1024;  // behind the waves' tap slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int NG = cs_mid / WV_GC, P = H * W;
  const int n_units = n_full + (N - n_full) * parts;
  const char* zpage = zero_page();
  const int hxl = hx_of(r16);

  using AFrag = WvAFrag<KS>;
  using Taps = WvTaps;
  char* const tslot = smem + wave * 1024;
  auto lane_now = [&]() { return wv_lane_now(lane); };
  auto load_a = [&](int cg) { return wv_load_a<KS>(wpw, cg, lane_now()); };
  auto issue_taps = [&](int cg) { wv_issue_taps(wdw, bpw, bdw, zpage, cs_mid, cg, lane_now(), tslot); };
  auto read_taps = [&]() { return wv_read_taps(tslot, g); };

  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const WvUnit un = wv_unit_of(u, n_full, parts, NG);
    const int img = un.img, ghi = un.ghi;
    int cg = un.glo + wave;
    AFrag a;
    if (cg < ghi) {  // the first unit's taps and weights land with the x rows
      issue_taps(cg);
      a = load_a(cg);
    }
    __syncthreads();               // every wave is done with the last image's x rows
    if (!(IRWS_WAVE_ABL & 4) || u == (int)blockIdx.x) {
      const int ninstr = P * CPR / 64;
      const bf16_t* xi = x + (size_t)img * P * CS * 2;
      for (int j = wave; j < ninstr; j += WV_NW) {
        const int id = j * 64 + lane, r = id / CPR, p = id - r * CPR;
        const int L = (p & ~15) | ((p & 15) ^ hx_of(r));
        const int plane = L / CPP, k8 = L - plane * CPP;
        const void* src = k8 * 8 < CS ? static_cast<const void*>(xi + (size_t)r * CS * 2 + plane * CS + k8 * 8) : zpage;
        dma16_asm(src, lds_lo32_u(xs + j * 1024));
      }
    }
    // vmcnt(0), spelled as the builtin: the compiler then knows the first unit's weights have landed here.  With the
    // asm form it held them pending at the unit loop's entry and, merging that with the back edge, drained the
    // stores in front of every unit's first MFMA with its own vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    __syncthreads();

    auto unit = [&]() {
      const int c4 = cg * WV_GC + 4 * g;  // the lane's 4 channels
      // ---- expand: the (row, k-step) operand reads run WV_PF - 1 steps ahead of their 3 MFMAs, through a ring of
      // WV_PF register slots
      f32x4 acc[HMAX];
      {
        constexpr int NI = HMAX * KS;
        bf16x8 bh[WV_PF], bl[WV_PF];
        auto load_b = [&](int i) {
          const int T = i / KS, ks = i % KS;
          const char* xr = xs + (T * 16 + r16) * XP;
          const int Lh = ks * 4 + g, Ll = CPP + ks * 4 + g;
          const int ph = ((Lh & ~15) | ((Lh & 15) ^ hxl)) << 4, pl = ((Ll & ~15) | ((Ll & 15) ^ hxl)) << 4;
          bh[i % WV_PF] = *reinterpret_cast<const bf16x8*>(xr + ph);
          bl[i % WV_PF] = *reinterpret_cast<const bf16x8*>(xr + pl);
        };
#pragma unroll
        for (int i = 0; i < WV_PF - 1; ++i)
          if (FULL || i / KS < H) load_b(i);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int T = i / KS, ks = i % KS, ip = i + WV_PF - 1;
          if (FULL || T < H) {
            if (ip < NI && (FULL || ip / KS < H)) load_b(ip);
            // keep the reads ahead of the MFMAs (left alone the scheduler sinks each to its use)
            __builtin_amdgcn_sched_barrier(0);
            f32x4 c = ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[T];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l[ks], bh[i % WV_PF], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h[ks], bl[i % WV_PF], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h[ks], bh[i % WV_PF], c, 0, 0, 0);
            acc[T] = c;
          }
        }
      }
      // This unit's taps: their DMA was issued before the weights the MFMAs above waited for, and vmcnt retires in
      // issue order, so they have landed
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" ::: "memory");
      const Taps tp = read_taps();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are in registers: the slot is free
      // The next unit's taps and weights, issued here: before this unit's stores.  The next unit's wait for them
      // then lets every store of this unit stay in flight; a load issued after the stores could only be waited for
      // together with all of them (the wave then stood out the write latency every unit: 642 us a launch, 404
      // without the stores).  The last unit of an image loads its own again (no branch).
      const int cgn = cg + WV_NW < ghi ? cg + WV_NW : cg;
      issue_taps(cgn);
      const AFrag an = load_a(cgn);
      __builtin_amdgcn_sched_barrier(0);

      // ---- depthwise: source row s feeds output rows s + 1 (taps 0-2), s (3-5) and s - 1 (6-8), so an output
      // row collects its taps in order 0 .. 8 and a row's two DPP moves serve all three
      const uint32_t ps = 4u * (uint32_t)cs_mid;  // bytes per position
      const int lny = lane_now();
      const uint32_t ylane = (uint32_t)(lny & 15) * ps + (F32 ? 4u * (uint32_t)(cg * WV_GC + 4 * (lny >> 4))
                                                              : 128u * (uint32_t)(cg >> 1) + 8u * (uint32_t)((cg & 1) * 4 + (lny >> 4)));
      char* const yimg = reinterpret_cast<char*>(y) + (uint32_t)(img * P) * ps;  // launch_ir_ws: < 2^32
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
      const float bbv[4] = {tp.bp.x, tp.bp.y, tp.bp.z, tp.bp.w}, bdv[4] = {tp.bd.x, tp.bd.y, tp.bd.z, tp.bd.w};
      float w[9][4];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        w[t][0] = tp.w[t].x; w[t][1] = tp.w[t].y; w[t][2] = tp.w[t].z; w[t][3] = tp.w[t].w;
      }
      float prv[4] = {0.f, 0.f, 0.f, 0.f}, cur[4] = {bdv[0], bdv[1], bdv[2], bdv[3]}, nxt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s <= HMAX; ++s) {
        if ((IRWS_WAVE_ABL & 2) && s < HMAX && (FULL || s < H)) {
#pragma unroll
          for (int j = 0; j < 4; ++j) nxt[j] = silu(acc[s][j] + bbv[j]) + w[4][j];
        } else if (s < HMAX && (FULL || s < H)) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float uc = silu(acc[s][j] + bbv[j]);
            const float ul = dpp_left(uc), ur = dpp_right(uc);
            nxt[j] = bdv[j];
            nxt[j] += w[0][j] * ul;
            nxt[j] += w[1][j] * uc;
            nxt[j] += w[2][j] * ur;
            cur[j] += w[3][j] * ul;
            cur[j] += w[4][j] * uc;
            cur[j] += w[5][j] * ur;
            if (s > 0) {
              prv[j] += w[6][j] * ul;
              prv[j] += w[7][j] * uc;
              prv[j] += w[8][j] * ur;
            }
          }
        }
        if (s >= 1 && (FULL || s - 1 < H)) {  // output row s - 1 is complete
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = silu(prv[j]);
            sum[j] += o[j];
          }
          char* dst = yimg + ((uint32_t)(s - 1) * 16u * ps + ylane);
          if (IRWS_WAVE_ABL & 1) {
          } else if (F32) {  // plain fp32 rows
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
          } else {  // the SE GEMM's interleaved operand: [hi 32 | lo 32] per 32-channel group
            uint2 hi, lo;
            split4(o, hi, lo);
            *reinterpret_cast<uint2*>(dst) = hi;
            *reinterpret_cast<uint2*>(dst + 64) = lo;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          prv[j] = cur[j];
          cur[j] = nxt[j];
        }
        // row by row: over the whole straight-line depthwise the scheduler ran the rows' chains side by side, into scratch
        __builtin_amdgcn_sched_barrier(0);
      }

      // ---- squeeze: the lane's rows are summed; add the 16 columns, lane r16 = j stores channel c4 + j
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[j] = dpp_ror_add<1>(dpp_ror_add<2>(dpp_ror_add<4>(dpp_ror_add<8>(sum[j]))));
      if (r16 < 4) {
        const float v = r16 == 0 ? sum[0] : r16 == 1 ? sum[1] : r16 == 2 ? sum[2] : sum[3];
        act_st<sp_t>(reinterpret_cast<sp_t*>(se_mean), img, cs_mid, c4 + r16, v / (float)P);
      }
      a = an;
    };
    for (; cg < ghi; cg += WV_NW) unit();
  }
}

template <int KS>
__device__ __forceinline__ void ir_ws_wave16(const bf16_t* __restrict__ x, int N, int H, int cs_mid,
                                             const bf16_t* __restrict__ wpw, const float* __restrict__ bpw,
                                             const float* __restrict__ wdw, const float* __restrict__ bdw,
                                             bf16_t* __restrict__ y, bf16_t* __restrict__ se_mean, int fm32, int n_full,
                                             int parts) {
  const bool full = H == 16;
  if (full && fm32) ir_ws_wave16<KS, true, true>(x, N, H, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
  else if (full) ir_ws_wave16<KS, true, false>(x, N, H, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
  else if (fm32) ir_ws_wave16<KS, false, true>(x, N, H, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
  else ir_ws_wave16<KS, false, false>(x, N, H, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
}

// ---- 8 x 8 maps --------------------------------------------------------------------------------------------------
// A position subtile of 16 is two image rows: lane (g, r16) of accumulator T holds channels 4g .. 4g + 3 of row
// 2 T + (r16 >> 3), column r16 & 7, and an image is 4 accumulators.  Horizontal taps are the same row_shr:1 /
// row_shl:1 moves, but lanes 7 and 8 of a DPP row are different image rows, so column 0 selects zero instead of lane
// - 1 and column 7 instead of lane + 1 (a select on the moved value, not a zeroed weight: a neighbour's Inf / NaN
// stays out).  Vertical taps: with v[T] = row_ror:8(u[T]) (the two halves swapped), the row above a lane of half h is
// U[T] = h ? v[T] : v[T - 1] and the row below is h ? v[T + 1] : v[T] = U[T + 1]; v[-1] and v[4] are outside the
// image (zero).  So step s builds U[s] once and uses it as output row pair s - 1's taps 6-8 and s's taps 0-2.
//
// x is double-buffered (2 x 64 positions x 1024 B at KS 7): the next work unit's image is DMA'd right after the
// image's one barrier, ahead of every load and store of the image's units (vmcnt retires in issue order, so nothing
// a unit waits for is ever behind it), and is waited for with the vmcnt(0) before the next barrier.
__device__ __forceinline__ float dpp_swap8(float v) {  // the value 8 lanes round the 16-lane row: the other image row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
}

// Channel groups a unit (diagnostic builds set 2: one wave runs two groups against each x fragment, which halves the
// operand reads; the taps then go through two slot sets, by unit parity)
#ifndef IRWS_WAVE8_G
#define IRWS_WAVE8_G 1
#endif
constexpr int WV8_G = IRWS_WAVE8_G;
constexpr int WV8_TS = WV8_G == 1 ? 1 : 2 * WV8_G;  // 1 KB tap slots a wave

template <int KS, bool F32>
__device__ __forceinline__ void ir_ws_wave8(const bf16_t* __restrict__ x, int N, int cs_mid, const bf16_t* __restrict__ wpw,
                                            const float* __restrict__ bpw, const float* __restrict__ wdw,
                                            const float* __restrict__ bdw, bf16_t* __restrict__ y,
                                            bf16_t* __restrict__ se_mean, int n_full, int parts) {
  constexpr int NT = 4, P = 64;  // accumulators (row pairs) and positions of an image
  constexpr int CS = KS * 32;    // input channel stride = expand K
  constexpr int CPP = (CS * 2 + 255) / 256 * 16;
  constexpr int CPR = 2 * CPP;  // 16-byte chunks per LDS x row
  constexpr int XP = CPR * 16;
  constexpr int XB = P * XP;    // bytes of an image's x rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const xs0 = smem + WV_NW * WV8_TS * 1024;  // two image buffers behind the waves' tap slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int NG = cs_mid / WV_GC;
  const int n_units = n_full + (N - n_full) * parts;
  const char* zpage = zero_page();
  const int hxl = hx_of(r16);

  using AFrag = WvAFrag<KS>;
  constexpr int G = WV8_G;
  auto tslot = [&](int q, int par) { return smem + (wave * WV8_TS + (G == 1 ? 0 : par * G + q)) * 1024; };
  auto lane_now = [&]() { return wv_lane_now(lane); };
  auto load_a = [&](int cg) { return wv_load_a<KS>(wpw, cg, lane_now()); };
  auto issue_taps = [&](int cg, char* slot) { wv_issue_taps(wdw, bpw, bdw, zpage, cs_mid, cg, lane_now(), slot); };
  auto issue_x = [&](int img, char* dst) {
    constexpr int ninstr = P * CPR / 64;
    const bf16_t* xi = x + (size_t)img * P * CS * 2;
    for (int j = wave; j < ninstr; j += WV_NW) {
      const int id = j * 64 + lane, r = id / CPR, p = id - r * CPR;
      const int L = (p & ~15) | ((p & 15) ^ hx_of(r));
      const int plane = L / CPP, k8 = L - plane * CPP;
      const void* src = k8 * 8 < CS ? static_cast<const void*>(xi + (size_t)r * CS * 2 + plane * CS + k8 * 8) : zpage;
      dma16_asm(src, lds_lo32_u(dst + j * 1024));
    }
  };

  int u = blockIdx.x, buf = 0, par = 0;
  if (u < n_units) issue_x(wv_unit_of(u, n_full, parts, NG).img, xs0);
  for (; u < n_units; u += gridDim.x, buf ^= 1) {
    const WvUnit un = wv_unit_of(u, n_full, parts, NG);
    const int img = un.img, ghi = un.ghi;
    int cg = un.glo + G * wave;
    // group q of the unit at c (an odd range's last unit runs its one group twice)
    auto gq = [&](int c, int q) { return c + q < ghi ? c + q : ghi - 1; };
    AFrag a[G];
    if (cg < ghi) {  // the first unit's taps and weights land with the x rows
#pragma unroll
      for (int q = 0; q < G; ++q) {
        issue_taps(gq(cg, q), tslot(q, par));
        a[q] = load_a(gq(cg, q));
      }
    }
    // vmcnt(0) as the builtin (ir_ws_wave16): this image's x rows (issued an image ago), the first unit's taps and
    // weights.  The one barrier of an image: every wave's share of the x rows has landed, and every wave is done with
    // the last image's buffer, which the next image's rows may now overwrite
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    __syncthreads();
    const int u_next = u + (int)gridDim.x;
    if (u_next < n_units && !(IRWS_WAVE_ABL & 4)) issue_x(wv_unit_of(u_next, n_full, parts, NG).img, xs0 + (buf ^ 1) * XB);
    const char* const xs = xs0 + ((IRWS_WAVE_ABL & 4) ? 0 : buf * XB);

    auto unit = [&]() {
      // ---- expand: as ir_ws_wave16, 4 subtiles
      f32x4 acc[G][NT];
      {
        constexpr int NI = NT * KS;
        bf16x8 bh[WV_PF], bl[WV_PF];
        auto load_b = [&](int i) {
          const int T = i / KS, ks = i % KS;
          const char* xr = xs + (T * 16 + r16) * XP;
          const int Lh = ks * 4 + g, Ll = CPP + ks * 4 + g;
          const int ph = ((Lh & ~15) | ((Lh & 15) ^ hxl)) << 4, pl = ((Ll & ~15) | ((Ll & 15) ^ hxl)) << 4;
          bh[i % WV_PF] = *reinterpret_cast<const bf16x8*>(xr + ph);
          bl[i % WV_PF] = *reinterpret_cast<const bf16x8*>(xr + pl);
        };
#pragma unroll
        for (int i = 0; i < WV_PF - 1; ++i) load_b(i);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int T = i / KS, ks = i % KS, ip = i + WV_PF - 1;
          if (ip < NI) load_b(ip);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < G; ++q) {
            f32x4 c = ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[q][T];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q].l[ks], bh[i % WV_PF], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q].h[ks], bl[i % WV_PF], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q].h[ks], bh[i % WV_PF], c, 0, 0, 0);
            acc[q][T] = c;
          }
        }
      }
      // this unit's taps have landed (issued before the weights the MFMAs waited for); the next unit's taps and
      // weights go out before this unit's stores (ir_ws_wave16)
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" ::: "memory");
      WvTaps tp0;
      if (G == 1) {  // one slot: read before the next unit's taps overwrite it
        tp0 = wv_read_taps(tslot(0, 0), g);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      const int cgn = cg + G * WV_NW < ghi ? cg + G * WV_NW : cg;
      AFrag an[G];
#pragma unroll
      for (int q = 0; q < G; ++q) {
        issue_taps(gq(cgn, q), tslot(q, par ^ 1));
        an[q] = load_a(gq(cgn, q));
      }
      __builtin_amdgcn_sched_barrier(0);

      // ---- depthwise of one group
      auto depthwise = [&](const f32x4 (&acc)[NT], const WvTaps& tp, int cg) {
      const int c4 = cg * WV_GC + 4 * g;  // the lane's 4 channels
      const uint32_t ps = 4u * (uint32_t)cs_mid;  // bytes per position
      const int lny = lane_now();
      const uint32_t ylane = (uint32_t)(lny & 15) * ps + (F32 ? 4u * (uint32_t)(cg * WV_GC + 4 * (lny >> 4))
                                                              : 128u * (uint32_t)(cg >> 1) + 8u * (uint32_t)((cg & 1) * 4 + (lny >> 4)));
      char* const yimg = reinterpret_cast<char*>(y) + (uint32_t)(img * P) * ps;  // launch_ir_ws: < 2^32
      const bool col0 = (lny & 7) == 0, col7 = (lny & 7) == 7, half = (lny & 8) != 0;
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
      const float bbv[4] = {tp.bp.x, tp.bp.y, tp.bp.z, tp.bp.w}, bdv[4] = {tp.bd.x, tp.bd.y, tp.bd.z, tp.bd.w};
      float w[9][4];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        w[t][0] = tp.w[t].x; w[t][1] = tp.w[t].y; w[t][2] = tp.w[t].z; w[t][3] = tp.w[t].w;
      }
      float cur[4] = {0.f, 0.f, 0.f, 0.f}, vprev[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s <= NT; ++s) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (IRWS_WAVE_ABL & 2) {
            if (s >= 1) o[j] = silu(acc[s - 1][j] + bbv[j]) + w[4][j];
            continue;
          }
          float uc = 0.f, ul = 0.f, ur = 0.f, v = 0.f;
          if (s < NT) {
            uc = silu(acc[s][j] + bbv[j]);
            const float ml = dpp_left(uc), mr = dpp_right(uc);
            ul = col0 ? 0.f : ml;
            ur = col7 ? 0.f : mr;
            v = dpp_swap8(uc);
          }
          // U[s]: the image row above row pair s's lanes = the row below row pair s - 1's
          const float up = half ? v : vprev[j];
          // (the moves stand outside the selects: inside a conditional arm they would run under a partial exec mask,
          // where a DPP move reads zero from the disabled lanes)
          const float mul = dpp_left(up), mur = dpp_right(up);
          const float upl = col0 ? 0.f : mul, upr = col7 ? 0.f : mur;
          vprev[j] = v;
          if (s >= 1) {
            float c = cur[j];
            c += w[6][j] * upl;
            c += w[7][j] * up;
            c += w[8][j] * upr;
            o[j] = c;
          }
          if (s < NT) {
            float n = bdv[j];
            n += w[0][j] * upl;
            n += w[1][j] * up;
            n += w[2][j] * upr;
            n += w[3][j] * ul;
            n += w[4][j] * uc;
            n += w[5][j] * ur;
            cur[j] = n;
          }
        }
        if (s >= 1) {  // output row pair s - 1 is complete
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = silu(o[j]);
            sum[j] += o[j];
          }
          char* dst = yimg + ((uint32_t)(s - 1) * 16u * ps + ylane);
          if (IRWS_WAVE_ABL & 1) {
          } else if (F32) {  // plain fp32 rows
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
          } else {  // the SE GEMM's interleaved operand: [hi 32 | lo 32] per 32-channel group
            uint2 hi, lo;
            split4(o, hi, lo);
            *reinterpret_cast<uint2*>(dst) = hi;
            *reinterpret_cast<uint2*>(dst + 64) = lo;
          }
        }
        __builtin_amdgcn_sched_barrier(0);  // row pair by row pair (ir_ws_wave16)
      }

      // ---- squeeze: the lane's row pairs are summed; add the 16 lanes (2 rows x 8 columns), lane r16 = j stores
      // channel c4 + j
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[j] = dpp_ror_add<1>(dpp_ror_add<2>(dpp_ror_add<4>(dpp_ror_add<8>(sum[j]))));
      if (r16 < 4) {
        const float v = r16 == 0 ? sum[0] : r16 == 1 ? sum[1] : r16 == 2 ? sum[2] : sum[3];
        act_st<sp_t>(reinterpret_cast<sp_t*>(se_mean), img, cs_mid, c4 + r16, v / (float)P);
      }
      };
#pragma unroll
      for (int q = 0; q < G; ++q) {
        if (G == 1) {
          depthwise(acc[q], tp0, cg);
        } else {
          const WvTaps tp = wv_read_taps(tslot(q, par), g);
          depthwise(acc[q], tp, gq(cg, q));
        }
        a[q] = an[q];
      }
      if (G > 1) par ^= 1;
    };
    for (; cg < ghi; cg += G * WV_NW) unit();
  }
}

template <int KS>
__device__ __forceinline__ void ir_ws_wave8(const bf16_t* __restrict__ x, int N, int cs_mid, const bf16_t* __restrict__ wpw,
                                            const float* __restrict__ bpw, const float* __restrict__ wdw,
                                            const float* __restrict__ bdw, bf16_t* __restrict__ y,
                                            bf16_t* __restrict__ se_mean, int fm32, int n_full, int parts) {
  if (fm32) ir_ws_wave8<KS, true>(x, N, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
  else ir_ws_wave8<KS, false>(x, N, cs_mid, wpw, bpw, wdw, bdw, y, se_mean, n_full, parts);
}
