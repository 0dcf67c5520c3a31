// ffx_noise.hip — multi-octave Perlin base-colour textures (include/ffx_labels.h): the first step of the dataset
// path, lerp_sampler.sample() at main.py:148-153.  gfx950 only, plain HIP.
//
// Three launches; no workgroup ever waits for another — phases are launch boundaries — and there is no atomic:
//   k_perlin_tile<false>  a 64 x 16 tile per workgroup, four consecutive texels per lane: the noise of the tile, its minimum and maximum
//                         to the workspace (one pair per tile)
//   k_perlin_extremes     one workgroup: the plane's minimum and maximum from the tiles' pairs
//   k_perlin_tile<true>   the same tiles again: the noise RECOMPUTED by the same device function (the library is built with
//                         -ffp-contract=off: the same bits, so the extremes normalise to exactly 0 and 1), normalised, blended, stored —
//                         three float4 per lane in the [h][w][3] layout where rows are 16-byte aligned, scalar stores otherwise
// Per octave a workgroup stages the lattice corners its tile touches in LDS as (cos, sin): one conversion per staged corner.
#include "ffx_common.h"
#include "../../include/ffx_labels.h"

#define PN_TW 64       // tile width
#define PN_TH 16       // tile height: FFX_PERLIN_WORKSPACE_BYTES counts 64 x 16 tiles
#define PN_BLOCK 256   // threads; each takes four horizontally adjacent texels
#define PN_MAX_OCT 8
#define PN_RED_BLOCK 1024
#define PN_CORNERS ((PN_TW + 1) * (PN_TH + 1)) // cells are at least one texel: a tile touches at most this many corners of an octave

struct PerlinK {
  int octaves, h, w;
  int R0[PN_MAX_OCT], R1[PN_MAX_OCT]; // lattice cells per axis
  int c0[PN_MAX_OCT], c1[PN_MAX_OCT]; // texels per cell
  unsigned ang_off[PN_MAX_OCT];       // floats in front of the octave's angles (below 2^31: the lattices' sizes at most double per octave up to 32769^2)
  float amp[PN_MAX_OCT];              // binary32 of persistence^o
};

__device__ __forceinline__ float pn_fade(float t) {
  const float t3 = t * t * t, t4 = t3 * t, t5 = t4 * t;
  return 6.0f * t5 - 15.0f * t4 + 10.0f * t3;
}
// torch.lerp's two-sided form: exact at both ends
__device__ __forceinline__ float pn_lerp(float a, float b, float wgt) { return wgt < 0.5f ? a + wgt * (b - a) : b - (b - a) * (1.0f - wgt); }

// the noise of the lane's four texels (i, j .. j + 3), coordinates beyond the plane clamped into it (such a lane repeats an edge texel:
// harmless to the extremes, and its stores are masked).  Every thread of the workgroup must call it: it stages and synchronises.
__device__ __forceinline__ void pn_tile_noise(const PerlinK &a, const float *__restrict__ angles, const float *__restrict__ pos, float2 *G, int i0, int j0,
                                              int i, int j, float v[4]) {
  const int t = threadIdx.x;
  const int ic = min(i, a.h - 1), i_last = min(i0 + PN_TH - 1, a.h - 1), j_last = min(j0 + PN_TW - 1, a.w - 1);
  v[0] = v[1] = v[2] = v[3] = 0.0f;
  for (int o = 0; o < a.octaves; ++o) {
    const int R0 = a.R0[o], R1 = a.R1[o], c0 = a.c0[o], c1 = a.c1[o];
    const int cy_lo = min(i0 / c0, R0 - 1), cy_hi = min(i_last / c0, R0 - 1), cx_lo = min(j0 / c1, R1 - 1), cx_hi = min(j_last / c1, R1 - 1);
    const int ny = cy_hi - cy_lo + 2, nx = cx_hi - cx_lo + 2; // <= PN_TH + 1, PN_TW + 1
    const float *ang = angles + a.ang_off[o];
    __syncthreads(); // the previous octave's corners have been read
    for (int k = t; k < ny * nx; k += PN_BLOCK) {
      const int gy = k / nx, gx = k - gy * nx;
      // (in float64, rounded once: the correctly rounded gradient for the price of one conversion per staged corner, which serves many texels)
      const double th = (double)ang[(size_t)(cy_lo + gy) * (size_t)(R1 + 1) + (size_t)(cx_lo + gx)];
      G[k] = make_float2((float)cos(th), (float)sin(th));
    }
    __syncthreads();
    const float *fy = pos + (size_t)o * ((size_t)a.h + (size_t)a.w), *fx = fy + a.h;
    const float py = fy[ic], ty = pn_fade(py), amp = a.amp[o];
    const int cy = min(ic / c0, R0 - 1) - cy_lo;
    int jc = min(j, a.w - 1), cxu = jc / c1, rem = jc - cxu * c1; // unclamped cell and the column inside it, stepped along the four texels
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float px = fx[jc], tx = pn_fade(px);
      const int cx = min(cxu, R1 - 1) - cx_lo;
      const float2 g00 = G[cy * nx + cx], g10 = G[(cy + 1) * nx + cx], g01 = G[cy * nx + cx + 1], g11 = G[(cy + 1) * nx + cx + 1];
      const float n00 = py * g00.x + px * g00.y, n10 = (py - 1.0f) * g10.x + px * g10.y;
      const float n01 = py * g01.x + (px - 1.0f) * g01.y, n11 = (py - 1.0f) * g11.x + (px - 1.0f) * g11.y;
      const float oct = 1.41421356237309504880f * pn_lerp(pn_lerp(n00, n10, ty), pn_lerp(n01, n11, ty), tx);
      v[k] = v[k] + amp * oct;
      if (jc < a.w - 1) {
        ++jc;
        if (++rem == c1) { rem = 0; ++cxu; }
      }
    }
  }
}

template <bool WRITE>
__global__ __launch_bounds__(PN_BLOCK) void k_perlin_tile(PerlinK a, const float *__restrict__ angles, const float *__restrict__ pos, float *ws,
                                                          const float *__restrict__ color_a, const float *__restrict__ color_b, int layout, int vec_ok,
                                                          float *__restrict__ out) {
  __shared__ float2 G[PN_CORNERS];
  __shared__ float2 red[PN_BLOCK / 64];
  const int t = threadIdx.x, i0 = blockIdx.y * PN_TH, j0 = blockIdx.x * PN_TW;
  const int i = i0 + (t >> 4), j = j0 + (t & 15) * 4;
  float v[4];
  pn_tile_noise(a, angles, pos, G, i0, j0, i, j, v);
  if (!WRITE) {
    float mn = fminf(fminf(v[0], v[1]), fminf(v[2], v[3])), mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, s));
      mx = fmaxf(mx, __shfl_xor(mx, s));
    }
    if ((t & 63) == 0) red[t >> 6] = make_float2(mn, mx);
    __syncthreads();
    if (t == 0) {
      for (int k = 1; k < PN_BLOCK / 64; ++k) {
        mn = fminf(mn, red[k].x);
        mx = fmaxf(mx, red[k].y);
      }
      float *part = ws + 4 + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
      part[0] = mn;
      part[1] = mx;
    }
    return;
  }
  if (i >= a.h || j >= a.w) return;
  const float lo = ws[0], d = ws[1] - lo;
  float c[3][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u = (v[k] - lo) / d;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][k] = pn_lerp(color_a[ch], color_b[ch], u);
  }
  const size_t p = (size_t)i * (size_t)a.w + (size_t)j, plane = (size_t)a.h * (size_t)a.w;
  if (layout == 1) {
    float *o = out + 3 * p;
    if (vec_ok) { // w % 4 == 0: the four texels are inside the row, and 12 floats from a multiple of 4 texels are 16-byte aligned
      reinterpret_cast<float4 *>(o)[0] = make_float4(c[0][0], c[1][0], c[2][0], c[0][1]);
      reinterpret_cast<float4 *>(o)[1] = make_float4(c[1][1], c[2][1], c[0][2], c[1][2]);
      reinterpret_cast<float4 *>(o)[2] = make_float4(c[2][2], c[0][3], c[1][3], c[2][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < a.w) {
          o[3 * k] = c[0][k];
          o[3 * k + 1] = c[1][k];
          o[3 * k + 2] = c[2][k];
        }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float *o = out + (size_t)ch * plane + p;
      if (vec_ok) {
        *reinterpret_cast<float4 *>(o) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j + k < a.w) o[k] = c[ch][k];
      }
    }
  }
}

// ws[0], ws[1] = the plane's minimum and maximum from the n_tiles pairs behind them
__global__ __launch_bounds__(PN_RED_BLOCK) void k_perlin_extremes(float *ws, int n_tiles) {
  __shared__ float2 red[PN_RED_BLOCK / 64];
  const int t = threadIdx.x;
  const float *part = ws + 4;
  float mn = part[0], mx = part[1]; // (tile 0 always exists)
  for (int k = t; k < n_tiles; k += PN_RED_BLOCK) {
    mn = fminf(mn, part[2 * (size_t)k]);
    mx = fmaxf(mx, part[2 * (size_t)k + 1]);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, s));
    mx = fmaxf(mx, __shfl_xor(mx, s));
  }
  if ((t & 63) == 0) red[t >> 6] = make_float2(mn, mx);
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < PN_RED_BLOCK / 64; ++k) {
      mn = fminf(mn, red[k].x);
      mx = fmaxf(mx, red[k].y);
    }
    ws[0] = mn;
    ws[1] = mx;
  }
}

extern "C" int ffx_perlin_texture(const float *angles, const float *pos, int octaves, int r0, int r1, double persistence, int h, int w, const float *color_a,
                                  const float *color_b, int layout, float *out, void *workspace, ffx_stream stream) {
  if (!angles) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: angles is NULL");
  if (!pos) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: pos is NULL");
  if (!color_a) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: color_a is NULL");
  if (!color_b) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: color_b is NULL");
  if (!out) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: out is NULL");
  if (!workspace) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: workspace is NULL");
  if (octaves < 1 || octaves > PN_MAX_OCT) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: octaves %d outside 1..%d", octaves, PN_MAX_OCT);
  if (h < 1 || h > 32768) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: h %d outside 1..32768", h);
  if (w < 1 || w > 32768) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: w %d outside 1..32768", w);
  if (r0 < 1) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: r0 %d below 1", r0);
  if (r1 < 1) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: r1 %d below 1", r1);
  PerlinK a;
  a.octaves = octaves, a.h = h, a.w = w;
  double amp = 1.0;
  unsigned long long off = 0;
  for (int o = 0; o < PN_MAX_OCT; ++o) {
    const long long R0 = (long long)r0 << o, R1 = (long long)r1 << o; // (r0, r1 < 2^31, o < 8: no overflow)
    if (o < octaves && (R0 > h || R1 > w))
      FFX_FAIL(FFX_ERR_ARG, "perlin_texture: octave %d: a cell of the %lld x %lld lattice is below one texel of %d x %d", o, R0, R1, h, w);
    const bool on = o < octaves;
    a.R0[o] = on ? (int)R0 : 1, a.R1[o] = on ? (int)R1 : 1;
    a.c0[o] = on ? h / (int)R0 : 1, a.c1[o] = on ? w / (int)R1 : 1;
    a.ang_off[o] = (unsigned)off;
    a.amp[o] = (float)amp; // persistence^o by repeated multiplication in double, as the host path's `amplitude *= persistence`
    if (on) off += (unsigned long long)(R0 + 1) * (unsigned long long)(R1 + 1);
    amp *= persistence;
  }
  if (layout != 0 && layout != 1) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: layout %d (0: [3,h,w], 1: [h,w,3])", layout);
  if (((uintptr_t)workspace & 7) != 0) FFX_FAIL(FFX_ERR_ARG, "perlin_texture: workspace must be 8-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 tiles(ffx_cdiv(w, PN_TW), ffx_cdiv(h, PN_TH));
  const int n_tiles = (int)(tiles.x * tiles.y); // at most 512 x 2048
  const int vec_ok = (w % 4 == 0) && ((uintptr_t)out & 15) == 0;
  float *ws = (float *)workspace;
  hipLaunchKernelGGL(k_perlin_tile<false>, tiles, dim3(PN_BLOCK), 0, s, a, angles, pos, ws, color_a, color_b, layout, vec_ok, out);
  FFX_CHECK_LAUNCH("perlin_tile");
  hipLaunchKernelGGL(k_perlin_extremes, dim3(1), dim3(PN_RED_BLOCK), 0, s, ws, n_tiles);
  FFX_CHECK_LAUNCH("perlin_extremes");
  hipLaunchKernelGGL(k_perlin_tile<true>, tiles, dim3(PN_BLOCK), 0, s, a, angles, pos, ws, color_a, color_b, layout, vec_ok, out);
  FFX_CHECK_LAUNCH("perlin_write");
  return FFX_OK;
}
