// The camera's operand band: what plain_scene (ffx_trace.hip) proves about cam_ray's two reciprocals before it launches the plain-scene
// instance of k_render_fwd_pk, whose cam_ray<BAND> takes them without the range fix-ups of the compiler's IEEE expansions.  The proof is host
// code without a HIP dependency: a stand-alone program can include it (tests/test_cam_band_cpu.py does); the device forms at the end are
// compiled under hipcc only.
//
// cam_ray forms, per sample at film position (sx, sy):
//   q_k = fmaf(a_k, sx, fmaf(b_k, sy, c_k))  (k = x, y, z; rows 0..2 of s2c),   np = q * iw,   il = 1 / sqrtf(|np|^2),   dl = np * il,   idz = 1 / dl.z
// i.e. sqrtf at |np|^2, a reciprocal at |np| = sqrtf(|np|^2) and a reciprocal at dl.z.
//
// The fix-ups and when they do nothing (gfx9 ISA, V_DIV_SCALE_F32 / V_DIV_FMAS_F32 / V_DIV_FIXUP_F32; LLVM's f32 sqrt expansion):
//   * 1.0f / d is  ds = div_scale(d, d, 1), ns = div_scale(1, d, 1) | VCC;  r = rcp(ds);  a Newton chain of fmas on (ns, ds, r);
//     div_fmas(VCC);  div_fixup(., d, 1).  With the numerator 1 (biased exponent 127), div_scale returns its operand unchanged and clears
//     VCC unless exponent(1) - exponent(d) >= 96 (|d| < 2^-95), d is denormal, 1 / d is denormal (|d| > 2^126), the quotient is
//     denormal (same), or the numerator's exponent is <= 23 (never: it is 1).  With VCC clear div_fmas is a plain fma.  div_fixup
//     replaces the chain's result only for NaN, zero or infinite operands and for quotients that leave float's range; otherwise it
//     copies the magnitude and sets the sign of n / d, which the chain's result already carries.  So for finite 2^-95 <= |d| <= 2^126
//     the expansion is: seed, the fma chain, nothing else.
//   * sqrtf(x) multiplies x by 2^32 first iff x < 2^-96 (and the root by 2^-16 after), takes the hardware root s, corrects it by one
//     ulp from the residuals fma(-(s - 1ulp), s, x) <= 0 and fma(-(s + 1ulp), s, x) > 0, and returns x itself iff x is +-0 or +inf
//     (v_cmp_class).  For finite x >= 2^-96 it is: seed, two residuals, two selects.
// The band proven here is far inside both:  2^-40 <= |np|^2 <= 2^40  (so 2^-20 <= |np| <= 2^20)  and  2^-40 <= |dl.z| <= 2^40.
//
// The proof.  q_k is affine in (sx, sy): over a rectangle its extrema are at the corners.  The film is sx, sy in [0, 1]; the kernels form
// sx = ((float)px + jx) * inv_w with jx in [0, 1), which rounding can carry to px + 1 and a last bit beyond 1: the rectangle taken is
// [-2^-10, 1 + 2^-10]^2.  Float rounding of q_k: two fmas, each within half an ulp of a value no larger than |a_k| + |b_k| + |c_k| (times the
// rectangle's 1 + 2^-10), so the computed q_k lies within e_k = 2^-21 (|a_k| + |b_k| + |c_k|) of the exact one; the corner interval is widened
// by e_k.  qz must keep one sign over the widened interval (dl.z != 0, and one form of the sign everywhere).  Then, all in double,
//   |np|^2 in [ (sum_k min |q_k|^2) iw^2 (1 - 2^-18),  (sum_k max |q_k|^2) iw^2 (1 + 2^-18) ]
// (min |q_k| = 0 where the interval holds 0; the factor covers the roundings of q * iw, of the squares and of their sum — sums of
// non-negative terms keep relative errors, a dozen roundings of 2^-24 each), and
//   |dl.z| = |np.z| * il  in  [ min |qz| / sqrt(sum_k max |q_k|^2) * (1 - 2^-18),  1 + 2^-18 ].
// In band iff w_uniform, iw finite and non-zero, every bound finite, qz one-signed and both intervals inside the band.  A camera that is
// not proven in band is simply not a plain scene: it renders through the generic instance and its IEEE forms.
#ifndef FFX_BAND_H
#define FFX_BAND_H
#include <cmath>

#define FFX_BAND_LO 9.094947017729282e-13 /* 2^-40 */
#define FFX_BAND_HI 1099511627776.0       /* 2^40 */

// what was bounded (for tests and diagnostics): [np2_lo, np2_hi] holds every |np|^2 the kernel can form, [dz_lo, dz_hi] every |dl.z|
struct FfxCamBand { double np2_lo, np2_hi, dz_lo, dz_hi; };

static inline bool ffx_cam_in_band(const float *s2c, int w_uniform, float iw_u, FfxCamBand *out = nullptr) {
  FfxCamBand b = {0.0, 0.0, 0.0, 0.0};
  if (out) *out = b;
  if (!w_uniform || !std::isfinite(iw_u) || iw_u == 0.f) return false;
  const double lo_s = -0x1p-10, hi_s = 1.0 + 0x1p-10, iw = (double)iw_u;
  double qmin2 = 0.0, qmax2 = 0.0, qz_min = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double a = s2c[4 * k + 0], bb = s2c[4 * k + 1], c = s2c[4 * k + 3];
    if (!std::isfinite(a) || !std::isfinite(bb) || !std::isfinite(c)) return false;
    double lo = INFINITY, hi = -INFINITY;
    for (int corner = 0; corner < 4; ++corner) {
      const double v = a * ((corner & 1) ? hi_s : lo_s) + bb * ((corner & 2) ? hi_s : lo_s) + c;
      lo = std::fmin(lo, v);
      hi = std::fmax(hi, v);
    }
    const double e = 0x1p-21 * (std::fabs(a) + std::fabs(bb) + std::fabs(c));
    lo -= e;
    hi += e;
    const double mn = (lo > 0.0) ? lo : (hi < 0.0 ? -hi : 0.0), mx = std::fmax(std::fabs(lo), std::fabs(hi));
    if (k == 2) {
      if (!(mn > 0.0)) return false; // qz reaches zero or changes sign on the film
      qz_min = mn;
    }
    qmin2 += mn * mn;
    qmax2 += mx * mx;
  }
  const double down = 1.0 - 0x1p-18, up = 1.0 + 0x1p-18;
  b.np2_lo = qmin2 * iw * iw * down;
  b.np2_hi = qmax2 * iw * iw * up;
  b.dz_lo = qz_min / std::sqrt(qmax2) * down;
  b.dz_hi = up;
  if (out) *out = b;
  if (!std::isfinite(b.np2_lo) || !std::isfinite(b.np2_hi) || !std::isfinite(b.dz_lo)) return false;
  return b.np2_lo >= FFX_BAND_LO && b.np2_hi <= FFX_BAND_HI && b.dz_lo >= FFX_BAND_LO && b.dz_hi <= FFX_BAND_HI;
}

// The in-band forms on the host, with the hardware seed as an argument (tests: the chain is exact for every seed within an ulp of the
// correctly rounded one).  cam_ray<BAND> performs the same operations on v_rcp_f32 / v_sqrt_f32's results.
static inline float ffx_band_rcp_chain(float d, float seed) {
  const float r0 = seed;
  const float r1 = fmaf(fmaf(-d, r0, 1.0f), r0, r0);
  const float q0 = 1.0f * r1;
  const float q1 = fmaf(fmaf(-d, q0, 1.0f), r1, q0);
  return fmaf(fmaf(-d, q1, 1.0f), r1, q1);
}
static inline float ffx_band_sqrt_chain(float x, float seed) {
  float s = seed;
  const float dn = std::nextafterf(seed, 0.0f), upn = std::nextafterf(seed, INFINITY);
  const float vp = fmaf(-dn, seed, x), vs = fmaf(-upn, seed, x);
  if (vp <= 0.f) s = dn;
  if (vs > 0.f) s = upn;
  return s;
}
#ifdef __HIPCC__
// The device forms (cam_ray<BAND>, ffx_trace.hip; tools/ubench/band_exact.hip compares them with the IEEE forms on the device): 1.0f / d and
// sqrtf(x) for operands the launch proved inside the camera's band (plain_scene) — the compiler's IEEE expansions without the steps that do nothing there — v_div_scale returns its operands and clears VCC, v_div_fmas is then a plain fma, v_div_fixup copies its first
// operand, the root neither rescales nor takes its zero / infinity arm.  What remains is the expansion's own seed and fma sequence, operation for
// operation: the same bits.
__device__ __forceinline__ float rcp_band(float d) {
  const float r0 = __builtin_amdgcn_rcpf(d);
  const float r1 = fmaf(fmaf(-d, r0, 1.0f), r0, r0);
  const float q1 = fmaf(fmaf(-d, r1, 1.0f), r1, r1); // (the quotient's first estimate is 1 * r1)
  return fmaf(fmaf(-d, q1, 1.0f), r1, q1);
}
__device__ __forceinline__ float sqrt_band(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float dn = __int_as_float(__float_as_int(s) - 1), up = __int_as_float(__float_as_int(s) + 1);
  const float vp = fmaf(-dn, s, x), vs = fmaf(-up, s, x);
  float r = vp <= 0.f ? dn : s;
  r = vs > 0.f ? up : r;
  return r;
}
#endif
#endif
