// ffx_splat_shared.h — what the K2 translation units (ffx_splat.hip, ffx_depth.hip) share: the tile and list sizes, the cut-off of a splat
// and its value at one texel.  Device code only.
#pragma once
#include "ffx_common.h"

#define SPLAT_BLOCK 256
#define TILE_W 32
#define TILE_H 8
#define CAND_MAX 512   // candidates staged per chunk in the fused forward kernel
#define NEIGH_MAX 2048 // neighbour list capacity of the gradient kernel
// exp(-q^2) is exactly 0 in binary32 for q^2 > 103.98; 10.3^2 = 106.1 leaves a margin, so culling
// on q > FFX_QCUT never drops a non-zero term.
#define FFX_QCUT 10.3f

// value of one splat at texel (fj, fi); rasterization.py:29-35
__device__ __forceinline__ float splat_val(float fj, float fi, float p0s, float p1s, float sigma, float inv_sigma, float &d, float &yd, float &xd) {
  yd = fj - p0s;
  xd = fi - p1s;
  d = yd * yd + xd * xd;
  if (d * inv_sigma > FFX_QCUT) return 0.f;
  float q = d / sigma;
  return expf(-(q * q));
}
// dv/d(p0*size0) = v*4*d*yd/sigma^2 (and xd for the other axis)
__device__ __forceinline__ float splat_gcoef(float v, float d, float sigma) { return v * 4.0f * d / (sigma * sigma); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
