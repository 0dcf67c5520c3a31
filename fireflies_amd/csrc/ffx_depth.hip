// ffx_depth.hip — the sparse-depth route of K2 for gfx950 (include/ffx_labels.h): the adjoint of the depth layers
// (ffx_splat_depth_bwd), softor over the layers without the [n,size1,size0] stack (ffx_splat_depth_softor_fwd) and its adjoint
// (ffx_splat_depth_softor_bwd).  The arrangement is the K2 family's (ffx_splat.hip): a workgroup per 32x8 texel tile with an ordered
// compaction of the points that reach it for the forward, a workgroup per point that sweeps its own footprint for the adjoints; fp32
// per-texel terms, fp64 sums, wave shuffles -> LDS -> one plain store per output: no atomics, two calls give the same bits.
//
// A layer is  layer_n(x) = (e_n(x) / m_n) z_n  with e_n the splat's value and m_n = e_n at the texel nearest to the point, clamped into the
// texture — every operation as k_splat_dense_fwd<1> performs it (the file is compiled with -ffp-contract=off), so the fused forward
// multiplies the very floats that kernel writes.
#include "ffx_splat_shared.h"
#include "../../include/ffx_labels.h"

// the layer maximum m of a point at (p0s, p1s) texels — the statement of k_splat_dense_fwd<1> — and the offsets / squared distance of the
// texel it is taken at
__device__ __forceinline__ float depth_peak(float p0s, float p1s, float sigma, int size0, int size1, float &yd, float &xd, float &d) {
  const float jn = fminf(fmaxf(rintf(p0s), 0.f), (float)(size0 - 1));
  const float in_ = fminf(fmaxf(rintf(p1s), 0.f), (float)(size1 - 1));
  yd = jn - p0s;
  xd = in_ - p1s;
  d = yd * yd + xd * xd;
  const float q = d / sigma;
  return expf(-(q * q));
}
__device__ __forceinline__ float depth_peak(float p0s, float p1s, float sigma, int size0, int size1) {
  float yd, xd, d;
  return depth_peak(p0s, p1s, sigma, size0, size1, yd, xd, d);
}
// one texel of one layer, as k_splat_dense_fwd<1> writes it
__device__ __forceinline__ float depth_layer(float fj, float fi, float p0s, float p1s, float m, float z, float sigma, float inv_sigma) {
  float d, yd, xd;
  const float v = splat_val(fj, fi, p0s, p1s, sigma, inv_sigma, d, yd, xd);
  return (v / m) * z;
}

// =================================================================================== fused forward
// out = 1 - prod_n (1 - layer_n), the product in ascending point order.  Wave 0 stages the points that reach the tile with their z and m.
// A point beyond reach has layer (0 / m) z = 0 and its factor is exactly 1 — unless its m is not a positive number (it underflowed: the
// point lies far outside the texture), where the dense layer is NaN on every texel: such a point is staged for every tile, and the plane
// comes out as the composition of the dense layers does.
__global__ void __launch_bounds__(SPLAT_BLOCK)
    k_depth_softor_fwd(const float *__restrict__ pts, const float *__restrict__ depth, int n, float sigma, int size0, int size1, float *__restrict__ out) {
  __shared__ float c_p0[CAND_MAX], c_p1[CAND_MAX], c_m[CAND_MAX], c_z[CAND_MAX];
  __shared__ int c_count;
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TILE_W, i0 = blockIdx.y * TILE_H;
  const int j = j0 + (tid % TILE_W), i = i0 + (tid / TILE_W);
  const float inv_sigma = 1.0f / sigma;
  float acc = 1.f;
  for (int chunk = 0; chunk < n; chunk += CAND_MAX) {
    if (tid < 64) { // wave 0: ordered compaction of this chunk
      int count = 0;
      const int lim = min(CAND_MAX, n - chunk);
      for (int base = 0; base < lim; base += 64) {
        const int k = chunk + base + tid;
        bool keep = false;
        float p0s = 0.f, p1s = 0.f, m = 1.f, z = 0.f;
        if (base + tid < lim) {
          p0s = pts[2 * k] * (float)size0;
          p1s = pts[2 * k + 1] * (float)size1;
          z = depth[k];
          m = depth_peak(p0s, p1s, sigma, size0, size1);
          const float dx = fmaxf(fmaxf((float)j0 - p0s, p0s - (float)(j0 + TILE_W - 1)), 0.f);
          const float dy = fmaxf(fmaxf((float)i0 - p1s, p1s - (float)(i0 + TILE_H - 1)), 0.f);
          keep = ((dx * dx + dy * dy) * inv_sigma <= FFX_QCUT) || !(m > 0.f);
        }
        const unsigned long long mk = __ballot(keep);
        const int pos = count + __popcll(mk & ((1ull << tid) - 1ull));
        if (keep) { c_p0[pos] = p0s; c_p1[pos] = p1s; c_m[pos] = m; c_z[pos] = z; }
        count += __popcll(mk);
      }
      if (tid == 0) c_count = count;
    }
    __syncthreads();
    const int cnt = c_count;
    if (j < size0 && i < size1) {
      for (int c = 0; c < cnt; ++c) acc *= (1.0f - depth_layer((float)j, (float)i, c_p0[c], c_p1[c], c_m[c], c_z[c], sigma, inv_sigma));
    }
    __syncthreads();
  }
  if (j < size0 && i < size1) out[(size_t)i * size0 + j] = 1.0f - acc;
}

// =================================================================================== adjoints
// One workgroup per point k; sweeps the texels where e_k is non-zero in binary32.
//   gz_k  = S / m                         S  = sum_x G(x) e_k(x)
//   gp_k  = z (A / m - S c* r* / m)       A  = sum_x G(x) de_k(x)/dp,   dm/dp = m c* r*  at the fixed texel x*  (r*: its offset from p, c* = 4 d* / sigma^2)
// FUSED: G(x) = gout(x) prod_{l != k} (1 - layer_l(x)), the product formed from the other points' factors (never by dividing by the point's
// own, which is 0 at the peak of a point with z = 1); the points whose footprint can overlap this one are staged in LDS with m and z,
// beyond NEIGH_MAX points the plain loop over all of them runs.  Not FUSED: G(x) = gout[k](x).
template <bool FUSED>
__global__ void __launch_bounds__(SPLAT_BLOCK)
    k_depth_bwd(const float *__restrict__ pts, const float *__restrict__ depth, int n, float sigma, int size0, int size1, const float *__restrict__ gout,
                float *__restrict__ gpts, float *__restrict__ gdepth) {
  __shared__ float nb_p0[FUSED ? NEIGH_MAX : 1], nb_p1[FUSED ? NEIGH_MAX : 1], nb_m[FUSED ? NEIGH_MAX : 1], nb_z[FUSED ? NEIGH_MAX : 1];
  __shared__ int nb_count;
  __shared__ double red[3][SPLAT_BLOCK / 64];

  const int k = blockIdx.x, tid = threadIdx.x;
  const float inv_sigma = 1.0f / sigma;
  const float p0s = pts[2 * k] * (float)size0, p1s = pts[2 * k + 1] * (float)size1;
  const float R = sqrtf(FFX_QCUT * sigma) + 1.0f; // radius beyond which e is exactly 0
  const int lo0 = max(0, (int)floorf(fmaxf(p0s - R, -1.f))), hi0 = min(size0, (int)ceilf(fminf(p0s + R, (float)size0)) + 1);
  const int lo1 = max(0, (int)floorf(fmaxf(p1s - R, -1.f))), hi1 = min(size1, (int)ceilf(fminf(p1s + R, (float)size1)) + 1);
  const bool alive = hi0 > lo0 && hi1 > lo1;
  const bool use_list = FUSED && n <= NEIGH_MAX;
  if (use_list) {
    if (tid < 64) {
      int count = 0;
      for (int base = 0; base < n; base += 64) {
        const int l = base + tid;
        bool keep = false;
        float q0 = 0.f, q1 = 0.f;
        if (l < n && l != k) {
          q0 = pts[2 * l] * (float)size0;
          q1 = pts[2 * l + 1] * (float)size1;
          keep = fabsf(q0 - p0s) <= 2.f * R + 2.f && fabsf(q1 - p1s) <= 2.f * R + 2.f;
        }
        const unsigned long long mk = __ballot(keep);
        const int pos = count + __popcll(mk & ((1ull << tid) - 1ull));
        if (keep) { nb_p0[pos] = q0; nb_p1[pos] = q1; nb_m[pos] = depth_peak(q0, q1, sigma, size0, size1); nb_z[pos] = depth[l]; }
        count += __popcll(mk);
      }
      if (tid == 0) nb_count = count;
    }
    __syncthreads();
  }
  double a0 = 0.0, a1 = 0.0, as = 0.0;
  if (alive) {
    const int rw = hi0 - lo0, rh = hi1 - lo1;
    const float *g = gout + (FUSED ? 0 : (size_t)k * size0 * size1);
    for (int t = tid; t < rw * rh; t += SPLAT_BLOCK) {
      const int j = lo0 + t % rw, i = lo1 + t / rw;
      float d, yd, xd;
      const float v = splat_val((float)j, (float)i, p0s, p1s, sigma, inv_sigma, d, yd, xd);
      if (v == 0.f) continue;
      float w = g[(size_t)i * size0 + j];
      if (FUSED) {
        float prod = 1.f;
        if (use_list) {
          const int cnt = nb_count;
          for (int c = 0; c < cnt; ++c) prod *= (1.0f - depth_layer((float)j, (float)i, nb_p0[c], nb_p1[c], nb_m[c], nb_z[c], sigma, inv_sigma));
        } else {
          for (int c = 0; c < n; ++c) {
            if (c == k) continue;
            const float q0 = pts[2 * c] * (float)size0, q1 = pts[2 * c + 1] * (float)size1;
            prod *= (1.0f - depth_layer((float)j, (float)i, q0, q1, depth_peak(q0, q1, sigma, size0, size1), depth[c], sigma, inv_sigma));
          }
        }
        w *= prod;
      }
      const float cf = splat_gcoef(v, d, sigma);
      a0 += (double)(w * (cf * yd));
      a1 += (double)(w * (cf * xd));
      as += (double)(w * v);
    }
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  as = wave_sum(as);
  if ((tid & 63) == 0) { red[0][tid >> 6] = a0; red[1][tid >> 6] = a1; red[2][tid >> 6] = as; }
  __syncthreads();
  if (tid == 0) {
    double A0 = 0.0, A1 = 0.0, S = 0.0;
#pragma unroll
    for (int w = 0; w < SPLAT_BLOCK / 64; ++w) { A0 += red[0][w]; A1 += red[1][w]; S += red[2][w]; }
    float yds, xds, ds;
    const double m = (double)depth_peak(p0s, p1s, sigma, size0, size1, yds, xds, ds);
    const double z = (double)depth[k];
    const double cs = 4.0 * (double)ds / ((double)sigma * (double)sigma);
    gdepth[k] = (float)(S / m);
    gpts[2 * k] = (float)(z * ((A0 - S * cs * (double)yds) / m) * (double)size0);
    gpts[2 * k + 1] = (float)(z * ((A1 - S * cs * (double)xds) / m) * (double)size1);
  }
}

// =================================================================================== host entry points
static int depth_args(const char *what, const float *pts, const float *depth, int n, float sigma, int size0, int size1) {
  if (n < 0) FFX_FAIL(FFX_ERR_ARG, "%s: n = %d is negative", what, n);
  if (size0 < 1 || size1 < 1) FFX_FAIL(FFX_ERR_ARG, "%s: size0 = %d, size1 = %d: both must be at least 1", what, size0, size1);
  if (!(sigma > 0.f)) FFX_FAIL(FFX_ERR_ARG, "%s: sigma = %g must be positive", what, (double)sigma);
  if (n > 0 && !pts) FFX_FAIL(FFX_ERR_ARG, "%s: pts is NULL", what);
  if (n > 0 && !depth) FFX_FAIL(FFX_ERR_ARG, "%s: depth is NULL", what);
  return FFX_OK;
}

int ffx_splat_depth_bwd(const float *pts, const float *depth, int n, float sigma, int size0, int size1, const float *gout, float *gpts, float *gdepth,
                        ffx_stream s) {
  if (const int rc = depth_args("splat_depth_bwd", pts, depth, n, sigma, size0, size1)) return rc;
  if (n == 0) return FFX_OK;
  if (!gout) FFX_FAIL(FFX_ERR_ARG, "splat_depth_bwd: gout is NULL");
  if (!gpts) FFX_FAIL(FFX_ERR_ARG, "splat_depth_bwd: gpts is NULL");
  if (!gdepth) FFX_FAIL(FFX_ERR_ARG, "splat_depth_bwd: gdepth is NULL");
  hipLaunchKernelGGL(k_depth_bwd<false>, dim3(n), dim3(SPLAT_BLOCK), 0, (hipStream_t)s, pts, depth, n, sigma, size0, size1, gout, gpts, gdepth);
  FFX_CHECK_LAUNCH("splat_depth_bwd");
  return FFX_OK;
}

int ffx_splat_depth_softor_fwd(const float *pts, const float *depth, int n, float sigma, int size0, int size1, float *out, ffx_stream s) {
  if (const int rc = depth_args("splat_depth_softor_fwd", pts, depth, n, sigma, size0, size1)) return rc;
  if (!out) FFX_FAIL(FFX_ERR_ARG, "splat_depth_softor_fwd: out is NULL");
  const dim3 grid(ffx_cdiv(size0, TILE_W), ffx_cdiv(size1, TILE_H));
  if (grid.y > 65535) FFX_FAIL(FFX_ERR_UNSUPPORTED, "splat_depth_softor_fwd: size1 = %d is beyond 65535 tiles of %d rows", size1, TILE_H);
  hipLaunchKernelGGL(k_depth_softor_fwd, grid, dim3(SPLAT_BLOCK), 0, (hipStream_t)s, pts, depth, n, sigma, size0, size1, out);
  FFX_CHECK_LAUNCH("splat_depth_softor_fwd");
  return FFX_OK;
}

int ffx_splat_depth_softor_bwd(const float *pts, const float *depth, int n, float sigma, int size0, int size1, const float *gout, float *gpts,
                               float *gdepth, ffx_stream s) {
  if (const int rc = depth_args("splat_depth_softor_bwd", pts, depth, n, sigma, size0, size1)) return rc;
  if (n == 0) return FFX_OK;
  if (!gout) FFX_FAIL(FFX_ERR_ARG, "splat_depth_softor_bwd: gout is NULL");
  if (!gpts) FFX_FAIL(FFX_ERR_ARG, "splat_depth_softor_bwd: gpts is NULL");
  if (!gdepth) FFX_FAIL(FFX_ERR_ARG, "splat_depth_softor_bwd: gdepth is NULL");
  hipLaunchKernelGGL(k_depth_bwd<true>, dim3(n), dim3(SPLAT_BLOCK), 0, (hipStream_t)s, pts, depth, n, sigma, size0, size1, gout, gpts, gdepth);
  FFX_CHECK_LAUNCH("splat_depth_softor_bwd");
  return FFX_OK;
}
