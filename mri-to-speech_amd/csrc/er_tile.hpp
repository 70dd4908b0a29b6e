// What the fused EdgeResidual kernels (er_fused, er2_fused, er_sp_fused, ers2_fused, er8_fused, er8w_fused) share
// besides lds_dma.hpp: the tile decode and the planar bf16 halo loader.  Device-only, internal linkage.
#pragma once

#include "lds_dma.hpp"

namespace m2s {
namespace {

// Tile index -> image n and the tile's first output row / column; tiles are TH x TW output pixels, image-major,
// then row-major (tpi = tiles_x * tiles_y tiles per image).
struct TilePos {
  int n, y0, x0;
};
template <int TH, int TW>
__device__ __forceinline__ TilePos tile_pos(int tile, int tpi, int tiles_x) {
  const int n = tile / tpi, tr = tile - n * tpi, ty = tr / tiles_x;
  return {n, ty * TH, (tr - ty * tiles_x) * TW};
}

// One wave's HP pieces of the haloed bf16 input of a stride-1 3x3 tile at t: (TH + 2) x 18 pixels around it, as planes
// of 8 channels [plane][pixel][16 B], each plane in 64-pixel DMA pieces of 1 KB; pixels outside the image (and the
// last piece's slots past the halo) come from the zero page.  xi: the image, ROW channels per pixel.  Piece
// wave * HP + j is plane piece / HPB, pixel block piece % HPB.  (er_sp_fused.hip keeps its own copy, with hi and lo
// plane groups: folded into this one it gained SGPR spills.)
template <int TH, int ROW, int HP>
__device__ __forceinline__ void halo_planes_dma(const bf16_t* xi, int H, int W, TilePos t, int wave, int lane,
                                                const void* zpage, char* buf) {
  constexpr int HW = 18, HPIX = (TH + 2) * HW, HPB = (HPIX + 63) / 64, HPLANE = HPB * 1024;
  const int ty0 = t.y0 - 1, tx0 = t.x0 - 1;
#pragma unroll
  for (int j = 0; j < HP; ++j) {
    const int piece = wave * HP + j, c = piece / HPB, pb = piece - c * HPB;
    const int p = pb * 64 + lane, hy = p / HW, hx = p - hy * HW;
    const int iy = ty0 + hy, ix = tx0 + hx;
    const void* src = zpage;
    if (p < HPIX && iy >= 0 && iy < H && ix >= 0 && ix < W) src = xi + ((size_t)iy * W + ix) * ROW + c * 8;
    dma16(src, buf + c * HPLANE + pb * 1024);
  }
}

}  // namespace
}  // namespace m2s
