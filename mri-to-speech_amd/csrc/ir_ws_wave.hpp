// The per-wave form of ir_ws's stride-1 front half on 16-wide maps of at most 16 rows (included by ir_ws.hip, which
// has the kernel entry and the launcher): a wave runs expand -> bn1 + SiLU -> depthwise 3x3 -> bn2 + SiLU -> store ->
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
template <int ROR>
__device__ __forceinline__ float dpp_ror_add(float v) {  // v + the value ROR lanes round the 16-lane row
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + ROR, 0xF, 0xF, false));
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

  struct AFrag {
    bf16x8 h[KS], l[KS];
  };
  // lane (g, r16): row 16 cg + r16 of W_hi / W_lo, k elements 32 ks + 8 g .. + 7 (16 rows x 64 B a load: L2)
  // (lane offsets of the global accesses are rebuilt where they are used, behind an asm barrier: hoisted out of the
  // loops they were kept in registers the units need, and spilled)
  auto lane_now = [&]() {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    return ln;
  };
  auto load_a = [&](int cg) {
    AFrag a;
    const int ln = lane_now();
    const bf16_t* wr = wpw + ((size_t)(cg * WV_GC + (ln & 15)) * CS * 2 + (ln >> 4) * 8);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      a.h[ks] = *reinterpret_cast<const bf16x8*>(wr + ks * 32);
      a.l[ks] = *reinterpret_cast<const bf16x8*>(wr + CS + ks * 32);
    }
    return a;
  };

  struct Taps {
    float4 w[9], bp, bd;  // the lane's 4 channels: depthwise taps, expand bias, depthwise bias
  };
  // A unit's taps and biases reach the wave's own 1 KB LDS slot by one LDS-DMA (lane l < 44: row l >> 2 of
  // [9 taps | expand bias | depthwise bias], channels 4 (l & 3) ..): a register prefetch of the 11 vectors beside
  // the next unit's weights spilled (256 registers, 396 B of scratch)
  char* const tslot = smem + wave * 1024;
  auto issue_taps = [&](int cg) {
    const int ln = lane_now(), t = ln >> 2, c = cg * WV_GC + 4 * (ln & 3);
    const void* src = t < 9 ? static_cast<const void*>(wdw + (t * cs_mid + c))
                            : t == 9 ? static_cast<const void*>(bpw + c) : t == 10 ? static_cast<const void*>(bdw + c) : zpage;
    dma16_asm(src, lds_lo32_u(tslot));
  };
  auto read_taps = [&]() {
    Taps t;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.w[k] = *reinterpret_cast<const float4*>(tslot + k * 64 + g * 16);
    t.bp = *reinterpret_cast<const float4*>(tslot + 9 * 64 + g * 16);
    t.bd = *reinterpret_cast<const float4*>(tslot + 10 * 64 + g * 16);
    return t;
  };

  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    int img = u, glo = 0, ghi = NG;  // image and group range [glo, ghi)
    if (u >= n_full) {
      const int q = u - n_full, pt = q % parts;
      img = n_full + q / parts;
      glo = pt * NG / parts;
      ghi = (pt + 1) * NG / parts;
    }
    int cg = glo + wave;
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
