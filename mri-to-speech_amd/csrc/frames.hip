// Device frame front end: decoded uint8 frames at the scanner's size -> the fp32 frames the acoustic model
// consumes, BGR -> grey, resize and normalisation in one kernel.  Serves both frame conventions of the reference:
//   inference  scripts/run_mri_video_inference.py:34-54 (_preprocess_frame): grey, cv2.INTER_LINEAR, per-frame
//              z-score, min-max to [0, 1]
//   training   mri2speech_code/preprocess_rtmri_data.py:99-113: grey, cv2.INTER_AREA, / 255
//
// The resize is OpenCV's 8-bit two-tap path (resize.cpp: the INTER_LINEAR branch, which INTER_AREA also takes
// where no axis shrinks), restated in DESIGN.md §22.  Per axis with source size s and destination size d:
// inv = (double)d / s, scale = 1.0 / inv, and for destination index i
//   LINEAR  f = (float)((i + 0.5) * scale - 0.5); i0 = floor(f); f -= i0
//   AREA    i0 = floor(i * scale); f = (float)((i + 1) - (i0 + 1) * inv); f = f <= 0 ? 0 : f - floor(f)
//   w1 = rint(f * 2048), w0 = rint((1 - f) * 2048) in float, taps clamp(i0) and clamp(i0 + 1) with the weights kept
//   R[y][x] = S[y][x0] * a0 + S[y][x1] * a1;  out = (((b0 * (R[y0][x] >> 4)) >> 16) + ((b1 * (R[y1][x] >> 4)) >> 16) + 2) >> 2
// Only IEEE basic operations with contraction off, so the coefficients are the host's bit for bit.  Shrinking takes
// other OpenCV paths (true area averaging, the exact-2x case) and is refused.
//
// One 1024-thread workgroup per frame, no workspace, one HBM traversal: the grey source frame is staged in LDS once
// (16-byte loads where the frame's base allows them, dwords or bytes otherwise; a frame base of i*h*w*ch bytes is
// unaligned in general), pass 1 resizes out of LDS into a byte image in LDS and reduces sum, sum of squares, min and
// max in integers (exact), pass 2 turns the byte image into fp32 with 16-byte stores where the output base allows
// them.  A resized pixel has one of 256 levels, so the normalisation is evaluated once per level into a table and
// pass 2 looks it up.  Dynamic LDS is source + resized bytes (<= 64 KB each) plus, while it fits in 128 KB, the two
// per-axis coefficient tables; a frame pair at both limits computes its coefficients per pixel instead.  The
// reduction scratch and the level table reuse the source bytes, which are dead after pass 1.  ZSCORE_MINMAX is
// preprocess_kernel's arithmetic on the resized integers; UNIT is (float)g / 255.0f.  Store-bound: h*w*ch bytes in,
// 4*out_h*out_w bytes out per frame.
//
// Masked variant (frames_masked_kernel): grid (frame, mask variant), the same body with the staging
// helpers' MASKED branch compiled in.  Every byte of every channel becomes (uint8)clip((float)byte * mask[y][x], 0,
// 255) on its way into LDS (scripts/mask_rtmri_video.py:96-98: one IEEE multiply, truncation), before bgr_grey.  The
// mask row is read from global memory (float4 where its base m*h*w*4 allows, dwords otherwise) and never staged, so
// the LDS layout and limits are the unmasked kernel's; frames and masks are re-read per variant out of L2.
#include "kernels.hpp"
#include "prof.hpp"

namespace m2s {
namespace {

constexpr int FR_THREADS = 1024;
constexpr int FR_WAVES = FR_THREADS / 64;
constexpr int FR_LDS_MAX = 128 * 1024;
constexpr int FR_MAX_PIX = 65536;
// reduction scratch + the 256-level output table, aliased onto the source bytes after pass 1
constexpr int FR_SCRATCH = 2048;
constexpr int FR_LUT_OFF = 512;

// dynamic LDS: [resized bytes][source bytes | reduction scratch][y table][x table]
struct FrLayout {
  int dst, src, total;
  bool tab;
  __host__ __device__ FrLayout(int hw, int how, int Ho, int Wo) {
    dst = (how + 15) & ~15;
    const int sb = (hw + 15) & ~15;
    src = sb > FR_SCRATCH ? sb : FR_SCRATCH;
    const int t = 8 * (Ho + Wo);
    tab = dst + src + t <= FR_LDS_MAX;
    total = dst + src + (tab ? t : 0);
  }
};

struct Coef {
  int t0, t1, w0, w1;  // clamped taps, 11-bit fixed-point weights
};

__device__ __forceinline__ Coef coef_at(int i, int s, double inv, double scale, int interp) {
#pragma clang fp contract(off)
  float f;
  int i0;
  if (interp == 0) {
    f = (float)(((double)i + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    i0 = (int)fl;
    f = f - fl;
  } else {
    i0 = (int)floor((double)i * scale);
    f = (float)((double)(i + 1) - (double)(i0 + 1) * inv);
    f = f <= 0.f ? 0.f : f - floorf(f);
  }
  Coef c;
  c.w1 = (int)rintf(f * 2048.f);
  c.w0 = (int)rintf((1.f - f) * 2048.f);
  c.t0 = min(max(i0, 0), s - 1);
  c.t1 = min(max(i0 + 1, 0), s - 1);
  return c;
}

__device__ __forceinline__ uint2 coef_pack(const Coef& c) {
  return make_uint2((uint32_t)c.t0 | ((uint32_t)c.t1 << 16), (uint32_t)c.w0 | ((uint32_t)c.w1 << 16));
}
__device__ __forceinline__ Coef coef_unpack(uint2 e) {
  Coef c;
  c.t0 = e.x & 0xffff;
  c.t1 = e.x >> 16;
  c.w0 = e.y & 0xffff;
  c.w1 = e.y >> 16;
  return c;
}

__device__ __forceinline__ int bgr_grey(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + (1 << 13)) >> 14; }

// the reference's mask application to one byte: float multiply, clip to [0, 255], truncate
__device__ __forceinline__ int mask_byte(int b, float m) { return (int)fminf(fmaxf((float)b * m, 0.f), 255.f); }

// the masks of pixels p .. p + 3 (p % 4 == 0): one 16-byte load where the mask's base allows it
__device__ __forceinline__ float4 mask4(const float* __restrict__ mk, int p, bool mvec) {
  if (mvec) return *reinterpret_cast<const float4*>(mk + p);
  return make_float4(mk[p], mk[p + 1], mk[p + 2], mk[p + 3]);
}

template <bool MASKED>
__device__ __forceinline__ uint8_t stage_pixel(const uint8_t* __restrict__ f, int ch, int p, const float* __restrict__ mk) {
  if constexpr (MASKED) {
    const float m = mk[p];
    return ch == 1 ? (uint8_t)mask_byte(f[p], m)
                   : (uint8_t)bgr_grey(mask_byte(f[3 * p], m), mask_byte(f[3 * p + 1], m), mask_byte(f[3 * p + 2], m));
  } else {
    return ch == 1 ? f[p] : (uint8_t)bgr_grey(f[3 * p], f[3 * p + 1], f[3 * p + 2]);
  }
}

// NW dwords of grey pixels per step: NW source dwords (grey) or 3 NW (BGR) -> NW dwords of LDS; bytes for the rest.
// MASKED: every source byte goes through mask_byte with its pixel's mask first (mk = this variant's mask).
template <int NW, bool MASKED>
__device__ __forceinline__ void stage_frame(const uint8_t* __restrict__ f, int hw, int ch, uint8_t* src, int tid,
                                            const float* __restrict__ mk, bool mvec) {
  const int nv = hw / (4 * NW);
  const uint32_t* f32 = reinterpret_cast<const uint32_t*>(f);
  uint32_t* s32 = reinterpret_cast<uint32_t*>(src);
  if (ch == 1) {
    for (int k = tid; k < nv; k += FR_THREADS) {
      uint32_t v[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) v[j] = f32[k * NW + j];
      if constexpr (MASKED) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const float4 m = mask4(mk, 4 * (k * NW + j), mvec);
          v[j] = (uint32_t)mask_byte(v[j] & 255, m.x) | ((uint32_t)mask_byte((v[j] >> 8) & 255, m.y) << 8) |
                 ((uint32_t)mask_byte((v[j] >> 16) & 255, m.z) << 16) | ((uint32_t)mask_byte(v[j] >> 24, m.w) << 24);
        }
      }
#pragma unroll
      for (int j = 0; j < NW; ++j) s32[k * NW + j] = v[j];
    }
  } else {
    for (int k = tid; k < nv; k += FR_THREADS) {
      uint32_t v[3 * NW];
#pragma unroll
      for (int j = 0; j < 3 * NW; ++j) v[j] = f32[k * 3 * NW + j];
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        uint32_t o = 0;
        float mq[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (MASKED) {
          const float4 m = mask4(mk, 4 * (k * NW + j), mvec);
          mq[0] = m.x, mq[1] = m.y, mq[2] = m.z, mq[3] = m.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = 3 * (4 * j + q);  // byte offset of the pixel's B within v
          int B = (v[b >> 2] >> (8 * (b & 3))) & 255;
          int G = (v[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 255;
          int R = (v[(b + 2) >> 2] >> (8 * ((b + 2) & 3))) & 255;
          if constexpr (MASKED) B = mask_byte(B, mq[q]), G = mask_byte(G, mq[q]), R = mask_byte(R, mq[q]);
          o |= (uint32_t)bgr_grey(B, G, R) << (8 * q);
        }
        s32[k * NW + j] = o;
      }
    }
  }
  for (int p = nv * 4 * NW + tid; p < hw; p += FR_THREADS) src[p] = stage_pixel<MASKED>(f, ch, p, mk);
}

// One frame through staging, resize and normalisation: f the frame's bytes, o its output, mk its mask (MASKED only).
template <bool MASKED>
__device__ __forceinline__ void frames_body(const uint8_t* __restrict__ f, const float* __restrict__ mk, int h, int w, int ch,
                                            int Ho, int Wo, int interp, int norm_mode, float* __restrict__ o) {
  extern __shared__ __attribute__((aligned(16))) uint8_t fr_lds[];
  const int hw = h * w, how = Ho * Wo;
  const FrLayout L(hw, how, Ho, Wo);
  uint8_t* dst = fr_lds;
  uint8_t* src = fr_lds + L.dst;
  uint2* ty = reinterpret_cast<uint2*>(fr_lds + L.dst + L.src);
  uint2* tx = ty + Ho;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  double inv_y, scale_y, inv_x, scale_x;
  {
#pragma clang fp contract(off)
    inv_y = (double)Ho / (double)h;
    scale_y = 1.0 / inv_y;
    inv_x = (double)Wo / (double)w;
    scale_x = 1.0 / inv_x;
  }

  const bool mvec = MASKED && ((uintptr_t)mk & 15) == 0;  // a mask base is dword-aligned, 16-byte aligned only sometimes
  if (((uintptr_t)f & 15) == 0)
    stage_frame<4, MASKED>(f, hw, ch, src, tid, mk, mvec);
  else if (((uintptr_t)f & 3) == 0)
    stage_frame<1, MASKED>(f, hw, ch, src, tid, mk, mvec);
  else
    for (int p = tid; p < hw; p += FR_THREADS) src[p] = stage_pixel<MASKED>(f, ch, p, mk);
  if (L.tab)
    for (int i = tid; i < Ho + Wo; i += FR_THREADS)
      ty[i] = coef_pack(i < Ho ? coef_at(i, h, inv_y, scale_y, interp) : coef_at(i - Ho, w, inv_x, scale_x, interp));
  __syncthreads();

  // pass 1: resize out of LDS, four pixels (one dword of the byte image) a step
  unsigned sum32 = 0, sq32 = 0;  // a thread sees at most 64 pixels: 64 * 255^2 < 2^32
  int mn = 255, mx = 0;
  const int units = (how + 3) >> 2;
  for (int k = tid; k < units; k += FR_THREADS) {
    int p = 4 * k;
    int y = p / Wo, x = p - y * Wo;
    uint32_t pack = 0;
    Coef cy = L.tab ? coef_unpack(ty[y]) : coef_at(y, h, inv_y, scale_y, interp);  // k < units: y < Ho
    const uint8_t* r0 = src + cy.t0 * w;
    const uint8_t* r1 = src + cy.t1 * w;
#pragma unroll
    for (int j = 0; j < 4; ++j, ++p) {
      if (p < how) {
        const Coef cx = L.tab ? coef_unpack(tx[x]) : coef_at(x, w, inv_x, scale_x, interp);
        const int R0 = r0[cx.t0] * cx.w0 + r0[cx.t1] * cx.w1;
        const int R1 = r1[cx.t0] * cx.w0 + r1[cx.t1] * cx.w1;
        const int g = (((cy.w0 * (R0 >> 4)) >> 16) + ((cy.w1 * (R1 >> 4)) >> 16) + 2) >> 2;
        pack |= (uint32_t)g << (8 * j);
        sum32 += g;
        sq32 += (unsigned)(g * g);
        mn = min(mn, g);
        mx = max(mx, g);
        if (++x == Wo) {  // the step crosses into the next row
          x = 0;
          ++y;
          if (p + 1 < how) {
            cy = L.tab ? coef_unpack(ty[y]) : coef_at(y, h, inv_y, scale_y, interp);
            r0 = src + cy.t0 * w;
            r1 = src + cy.t1 * w;
          }
        }
      }
    }
    reinterpret_cast<uint32_t*>(dst)[k] = pack;
  }

  static_assert(FR_MAX_PIX / 4 <= 16 * FR_THREADS, "pixels per thread");
  float mean = 0.f, sd = 0.f, zlo = 0.f, zhi = 0.f;
  float* lut = reinterpret_cast<float*>(src + FR_LUT_OFF);
  if (norm_mode == 0) {
    unsigned long long sum = sum32, sq = sq32;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      sum += __shfl_xor(sum, m);
      sq += __shfl_xor(sq, m);
      mn = min(mn, __shfl_xor(mn, m));
      mx = max(mx, __shfl_xor(mx, m));
    }
    __syncthreads();  // every wave is done with the source bytes: the scratch may overwrite them
    unsigned long long* s_sum = reinterpret_cast<unsigned long long*>(src);
    unsigned long long* s_sq = s_sum + FR_WAVES;
    int* s_min = reinterpret_cast<int*>(s_sq + FR_WAVES);
    int* s_max = s_min + FR_WAVES;
    float* s_par = reinterpret_cast<float*>(s_max + FR_WAVES);
    static_assert(FR_WAVES * 24 + 16 <= FR_LUT_OFF && FR_LUT_OFF + 256 * 4 <= FR_SCRATCH, "reduction scratch");
    if (lane == 0) {
      s_sum[wave] = sum;
      s_sq[wave] = sq;
      s_min[wave] = mn;
      s_max[wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {  // preprocess_kernel's parameters, on the resized frame
      unsigned long long S = 0, Q = 0;
      int lo = 255, hi = 0;
      for (int v = 0; v < FR_WAVES; ++v) {
        S += s_sum[v];
        Q += s_sq[v];
        lo = min(lo, s_min[v]);
        hi = max(hi, s_max[v]);
      }
      const double n = (double)how;
      const float mean_ = (float)((double)S / n);
      const double var = ((double)Q - (double)S * (double)S / n) / n;
      const float sd_ = (float)sqrt(var > 0.0 ? var : 0.0);
      float zlo_, zhi_;
      {
#pragma clang fp contract(off)
        zlo_ = sd_ > 0.f ? ((float)lo - mean_) / sd_ : (float)lo - mean_;
        zhi_ = sd_ > 0.f ? ((float)hi - mean_) / sd_ : (float)hi - mean_;
      }
      s_par[0] = mean_;
      s_par[1] = sd_;
      s_par[2] = zlo_;
      s_par[3] = zhi_;
    }
    __syncthreads();
    mean = s_par[0], sd = s_par[1], zlo = s_par[2], zhi = s_par[3];
  } else {
    __syncthreads();  // the byte image is complete, the source bytes are dead
  }

  // a resized pixel has one of 256 levels: the output of each, once, in the reference's float32 operation order
  const bool flat = !(zhi > zlo);
  if (tid < 256) {
#pragma clang fp contract(off)
    const float g = (float)tid;
    float v;
    if (norm_mode != 0) {
      v = g / 255.0f;
    } else {
      const float z = sd > 0.f ? (g - mean) / sd : g - mean;
      v = flat ? 0.f : (z - zlo) / (zhi - zlo);
    }
    lut[tid] = v;
  }
  __syncthreads();

  // pass 2: byte image -> fp32
  auto norm = [&](int gi) { return lut[gi]; };
  if (((uintptr_t)o & 15) == 0) {
    for (int k = tid; k < how / 4; k += FR_THREADS) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(dst)[k];
      reinterpret_cast<float4*>(o)[k] = make_float4(norm(v & 255), norm((v >> 8) & 255), norm((v >> 16) & 255), norm(v >> 24));
    }
    for (int p = (how & ~3) + tid; p < how; p += FR_THREADS) o[p] = norm(dst[p]);
  } else {
    for (int p = tid; p < how; p += FR_THREADS) o[p] = norm(dst[p]);
  }
}

// 8 waves a SIMD (64 VGPRs): two workgroups share a CU where their LDS fits (84 x 84 -> 256 x 256 takes 77 KB)
__global__ void __launch_bounds__(FR_THREADS, 8) frames_kernel(const uint8_t* __restrict__ frames, int h, int w, int ch, int Ho,
                                                            int Wo, int interp, int norm_mode, float* __restrict__ out) {
  const int hw = h * w, how = Ho * Wo;
  frames_body<false>(frames + (size_t)blockIdx.x * hw * ch, nullptr, h, w, ch, Ho, Wo, interp, norm_mode,
                     out + (size_t)blockIdx.x * how);
}

// grid (frame, mask variant): out (n_masks, N, Ho, Wo)
__global__ void __launch_bounds__(FR_THREADS, 8) frames_masked_kernel(const uint8_t* __restrict__ frames, int h, int w, int ch,
                                                                   const float* __restrict__ masks, int Ho, int Wo,
                                                                   int interp, int norm_mode, float* __restrict__ out) {
  const int hw = h * w, how = Ho * Wo;
  frames_body<true>(frames + (size_t)blockIdx.x * hw * ch, masks + (size_t)blockIdx.y * hw, h, w, ch, Ho, Wo, interp,
                    norm_mode, out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * how);
}

}  // namespace

namespace {
void check_frames(int N, int h, int w, int channels, int out_h, int out_w, int interp, int norm) {
  M2S_CHECK(N >= 0 && h > 0 && w > 0 && out_h > 0 && out_w > 0, "frames: bad shape");
  M2S_CHECK(channels == 1 || channels == 3, "frames: channels must be 1 (grey) or 3 (BGR)");
  M2S_CHECK(h <= out_h && w <= out_w, "frames: a shrinking resize is not supported (OpenCV takes other paths there)");
  M2S_CHECK((long)h * w <= FR_MAX_PIX && (long)out_h * out_w <= FR_MAX_PIX, "frames: more than 65536 pixels a frame");
  M2S_CHECK(interp == 0 || interp == 1, "frames: unknown m2s_frame_interp");
  M2S_CHECK(norm == 0 || norm == 1, "frames: unknown m2s_frame_norm");
}
}  // namespace

void launch_frames(const uint8_t* frames, int N, int h, int w, int channels, int out_h, int out_w, int interp, int norm,
                   float* out, hipStream_t s) {
  check_frames(N, h, w, channels, out_h, out_w, interp, norm);
  if (N == 0) return;
  M2S_CHECK(frames && out, "frames: null argument");
  const FrLayout L(h * w, out_h * out_w, out_h, out_w);
  allow_lds(reinterpret_cast<const void*>(&frames_kernel));
  StageTag tag("frames");
  const double bytes = (double)N * ((double)h * w * channels + 4.0 * out_h * out_w);
  ProfScope ps("frames_kernel", 0.0, bytes, s);
  hipLaunchKernelGGL(frames_kernel, dim3(N), dim3(FR_THREADS), L.total, s, frames, h, w, channels, out_h, out_w, interp, norm,
                     out);
  M2S_HIP(hipGetLastError());
}

void launch_frames_masked(const uint8_t* frames, int N, int h, int w, int channels, const float* masks, int n_masks,
                          int out_h, int out_w, int interp, int norm, float* out, hipStream_t s) {
  check_frames(N, h, w, channels, out_h, out_w, interp, norm);
  M2S_CHECK(n_masks >= 1 && n_masks <= 65535, "frames: n_masks outside 1..65535");
  if (N == 0) return;
  M2S_CHECK(frames && masks && out, "frames: null argument");
  const FrLayout L(h * w, out_h * out_w, out_h, out_w);
  allow_lds(reinterpret_cast<const void*>(&frames_masked_kernel));
  StageTag tag("frames");
  const double bytes = (double)N * n_masks * ((double)h * w * (channels + 4.0) + 4.0 * out_h * out_w);
  ProfScope ps("frames_masked_kernel", 0.0, bytes, s);
  hipLaunchKernelGGL(frames_masked_kernel, dim3(N, n_masks), dim3(FR_THREADS), L.total, s, frames, h, w, channels, masks, out_h,
                     out_w, interp, norm, out);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
