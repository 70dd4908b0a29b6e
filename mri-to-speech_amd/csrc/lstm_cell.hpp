// Device pieces the BiLSTM recurrence kernels share (lstm_persistent.hip: persistent, x3, x3g, small, mid;
// lstm_window.hip: the window step): the gate activations, the W_hh -> resident A-fragment loads, the split MFMA
// chain, the K-slice partial store and sum, the cell update, the hand-off encodings of h and the timeout exit.
// Device-only: included by .hip files, every definition has internal linkage.  A piece that one kernel alone uses
// lives in that kernel (DESIGN.md §29 lists them).
#pragma once

#include "lstm_route.hpp"
#include "m2s_common.hpp"

namespace m2s {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

// The rcp-based sigmoid (v_exp + v_rcp, 1 ulp each) and tanh(x) = 2 sigmoid(2x) - 1 (absolute error ~1e-7): the
// cell update is on every step's critical path, and libm's expf + IEEE divide and tanhf cost 7.51 against 7.18 us
// per recurrent step at 8 x 1000.
__device__ __forceinline__ float lstm_sig(float x) { return sigmoidf_(x); }
__device__ __forceinline__ float lstm_tanh(float x) { return 2.f * sigmoidf_(2.f * x) - 1.f; }

// the frame a direction visits at a step: forward t = step, reverse t = T - 1 - step
__device__ __forceinline__ int lstm_time(int dir, int step, int T) { return dir == 0 ? step : T - 1 - step; }

// N consecutive k of a W_hh row -> fp32 A fragments / dot-product operands, resident for the launch.  (The caller
// forms the row pointer: a helper for it changed the scalar address code of every kernel)
template <int N>
__device__ __forceinline__ void lstm_wfrag_f32(const float* wr, float (&wa)[N]) {
#pragma unroll
  for (int s = 0; s < N; s += 4) {
    const float4 v = *reinterpret_cast<const float4*>(wr + s);
    wa[s] = v.x;
    wa[s + 1] = v.y;
    wa[s + 2] = v.z;
    wa[s + 3] = v.w;
  }
}

// KS k-steps of 16 of a W_hh row, split -> resident hi / lo bf16 A fragments (wr: the row at this lane's first k,
// slice + 8 (lane / 32); k-step s covers k = 16 s + 0..7 from there)
template <int KS>
__device__ __forceinline__ void lstm_wfrag_split(const float* wr, bf16x8 (&whi)[KS], bf16x8 (&wlo)[KS]) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const float4 a = *reinterpret_cast<const float4*>(wr + 16 * s);
    const float4 b = *reinterpret_cast<const float4*>(wr + 16 * s + 4);
    const float v0[4] = {a.x, a.y, a.z, a.w}, v1[4] = {b.x, b.y, b.z, b.w};
    uint2 h0, l0, h1, l1;
    split4(v0, h0, l0);
    split4(v1, h1, l1);
    whi[s] = __builtin_bit_cast(bf16x8, make_uint4(h0.x, h0.y, h1.x, h1.y));
    wlo[s] = __builtin_bit_cast(bf16x8, make_uint4(l0.x, l0.y, l1.x, l1.y));
  }
}

// W_hi h_lo + W_lo h_hi + W_hi h_hi over a wave's K slice, fp32 accumulation (v_mfma_f32_32x32x16_bf16): three
// terms per k-step, small ones first; the two row tiles' chains interleave
template <int KS>
__device__ __forceinline__ void lstm_mfma_x3(const bf16x8 (&whi)[2][KS], const bf16x8 (&wlo)[2][KS],
                                             const uint4 (&bh)[KS], const uint4 (&bl)[KS], f32x16 (&acc)[2]) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[m][s], __builtin_bit_cast(bf16x8, bh[s]), acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi[m][s], __builtin_bit_cast(bf16x8, bl[s]), acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi[m][s], __builtin_bit_cast(bf16x8, bh[s]), acc[m], 0, 0, 0);
    }
}

// one 32 x 32 accumulator tile -> its 32 rows of the K-slice partial image: acc[i] holds row 8 (i / 4) + 4 hh + i % 4
// (hh = lane / 32), column l32 = lane % 32
__device__ __forceinline__ void lstm_store_partial(float (*rows)[33], const f32x16& acc, int hh, int l32) {
#pragma unroll
  for (int i = 0; i < 16; ++i) rows[8 * (i / 4) + 4 * hh + (i % 4)][l32] = acc[i];
}

// the eight K-slice partials of (gate row r, sequence b), summed in a fixed order
template <class Red>
__device__ __forceinline__ float lstm_sum8(const Red& red, int r, int b) {
  return ((red[0][r][b] + red[1][r][b]) + (red[2][r][b] + red[3][r][b])) +
         ((red[4][r][b] + red[5][r][b]) + (red[6][r][b] + red[7][r][b]));
}

// i, f, g, o (pre-activation pre[q] + recurrent sum gs[q]) -> c' = f c + i g in place, returns h' = o tanh(c').
// has_prev = false is step 0 (c = 0: the forget term is dropped, not multiplied).
// c' is two rounded products and a rounded sum, never an fma: that is what every kernel computed when each had its
// own copy of this (the two products packed into one v_pk_mul_f32), by the vectoriser's choice; written down here
// so that a change of code layout cannot fuse it in one kernel and change that kernel's result bits.
__device__ __forceinline__ float lstm_cell(const float (&pre)[4], const float (&gs)[4], bool has_prev, float& c) {
  const float gi = lstm_sig(pre[0] + gs[0]);
  const float gf = lstm_sig(pre[1] + gs[1]);
  const float gg = lstm_tanh(pre[2] + gs[2]);
  const float go = lstm_sig(pre[3] + gs[3]);
  float cn;
  {
#pragma clang fp contract(off)
    cn = has_prev ? gf * c + gi * gg : gi * gg;
  }
  c = cn;
  return go * lstm_tanh(cn);
}

// h as a bf16 pair hi + lo (the split of sp_t, 17 bits)
__device__ __forceinline__ void lstm_split_h(float h, bf16_t& hi, bf16_t& lo) {
  hi = f2bf(h);
  lo = f2bf(h - bf2f(hi));
}

// a data-tagged 8-byte granule {tag | fp32 h} (lstm_small, lstm_mid; lstm_x3g packs its hi / lo pair itself)
__device__ __forceinline__ unsigned long long lstm_granule(unsigned tag, float h) {
  return ((unsigned long long)tag << 32) | __float_as_uint(h);
}

// A hand-off wait timed out (abort_flag set, the workgroup past its barrier): flag the host and write NaN over the
// workgroup's U units of sequences [0, nb) at this and every later step, so the grid drains and nothing stale is
// read as a result.  The caller returns.
template <int U, int THREADS>
__device__ __forceinline__ void lstm_poison(float* hsd, unsigned* err_host, int dir, int ug, int step, int T, int nb) {
  const int tid = threadIdx.x;
  if (tid == 0 && err_host) __hip_atomic_store(err_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (int st = step; st < T; ++st) {
    const int tt = lstm_time(dir, st, T);
    for (int p = tid; p < U * nb; p += THREADS)
      hsd[((size_t)(p / U) * T + tt) * LSTM_H + ug * U + p % U] = __builtin_nanf("");
  }
}

}  // namespace
}  // namespace m2s
