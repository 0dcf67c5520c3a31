// The camera band's exact forms against the IEEE forms, on the device (gfx950): cam_ray<BAND>'s rcp_band / sqrt_band (fireflies_amd/csrc/ffx_band.h)
// and the compiler's 1.0f / x, sqrtf(x), 1.0f / sqrtf(x), on operands inside the band (2^-40 .. 2^40, either sign for the reciprocal), on the band's
// edges and the floats next to them, and outside it.  Prints how many results differ bit for bit: 0 inside and on the edges is what the plain-scene
// instance of k_render_fwd_pk rests on; outside the band differences are expected (that is what the launch's proof keeps out) and are only counted.
//
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I fireflies_amd/csrc -o band_exact tools/ubench/band_exact.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "ffx_band.h"

// per operand: bit 0 the reciprocal, bit 1 the reciprocal of -x, bit 2 the root, bit 3 the reciprocal root (cam_ray's il) differs
__global__ void __launch_bounds__(256) k_compare(const float *__restrict__ x, long n, unsigned *__restrict__ counts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  const float a0 = 1.0f / v, b0 = rcp_band(v);
  const float a1 = 1.0f / -v, b1 = rcp_band(-v);
  const float a2 = sqrtf(v), b2 = sqrt_band(v);
  const float a3 = 1.0f / sqrtf(v), b3 = rcp_band(sqrt_band(v));
  if (__float_as_uint(a0) != __float_as_uint(b0)) atomicAdd(&counts[0], 1u);
  if (__float_as_uint(a1) != __float_as_uint(b1)) atomicAdd(&counts[1], 1u);
  if (__float_as_uint(a2) != __float_as_uint(b2)) atomicAdd(&counts[2], 1u);
  if (__float_as_uint(a3) != __float_as_uint(b3)) atomicAdd(&counts[3], 1u);
}

#define CHECK(e)                                                                   \
  do {                                                                             \
    hipError_t err_ = (e);                                                         \
    if (err_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));                    \
      return 2;                                                                    \
    }                                                                              \
  } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() { // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int run(const char *what, const std::vector<float> &h, float *d_x, unsigned *d_c, bool must_agree, int &bad) {
  unsigned c[4] = {0, 0, 0, 0};
  CHECK(hipMemcpy(d_x, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemset(d_c, 0, sizeof c));
  hipLaunchKernelGGL(k_compare, dim3((unsigned)((h.size() + 255) / 256)), dim3(256), 0, 0, d_x, (long)h.size(), d_c);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(c, d_c, sizeof c, hipMemcpyDeviceToHost));
  printf("%-44s %9zu operands   differing: 1/x %u   1/-x %u   sqrt %u   1/sqrt %u%s\n", what, h.size(), c[0], c[1], c[2], c[3],
         must_agree ? ((c[0] | c[1] | c[2] | c[3]) ? "   <-- MISMATCH" : "   ok") : "   (outside the band: counted only)");
  if (must_agree && (c[0] | c[1] | c[2] | c[3])) ++bad;
  return 0;
}

int main() {
  const size_t n_rand = (size_t)1 << 24;
  float *d_x;
  unsigned *d_c;
  CHECK(hipMalloc(&d_x, n_rand * sizeof(float)));
  CHECK(hipMalloc(&d_c, 4 * sizeof(unsigned)));
  int bad = 0;
  const uint32_t e_lo = 127 - 40, e_hi = 127 + 40; // biased exponents of the band's edges
  std::vector<float> h(n_rand);
  for (size_t i = 0; i < n_rand; ++i) h[i] = from_bits(((e_lo + rnd32() % 80u) << 23) | (rnd32() & 0x7fffffu)); // 2^-40 <= x < 2^40, every mantissa alike
  if (run("random operands inside the band", h, d_x, d_c, true, bad)) return 2;
  h.clear();
  for (uint32_t e = e_lo; e < e_hi; ++e) // every binade of the band: its first floats, its last (the all-ones mantissas among them), its middle
    for (uint32_t k = 0; k < 64; ++k) {
      h.push_back(from_bits((e << 23) | k));
      h.push_back(from_bits((e << 23) | (0x7fffffu - k)));
      h.push_back(from_bits((e << 23) | (0x400000u - 32u + k)));
    }
  h.push_back(from_bits(e_hi << 23)); // 2^40 itself
  if (run("band edges, binade ends and middles", h, d_x, d_c, true, bad)) return 2;
  h.clear();
  for (uint32_t k = 1; k <= 64; ++k) { h.push_back(from_bits((e_lo << 23) - k)); h.push_back(from_bits((e_hi << 23) + k)); } // the floats just outside
  if (run("just outside the band (64 floats each side)", h, d_x, d_c, false, bad)) return 2;
  h.clear();
  for (uint32_t e = 0; e < 255; ++e) // every binade outside the band, the denormals (e = 0) included
    if (e < e_lo || e > e_hi)
      for (uint32_t k = 0; k < 16; ++k) h.push_back(from_bits((e << 23) | (rnd32() & 0x7fffffu)));
  h.push_back(0.0f);
  h.push_back(from_bits(0x7f800000u));
  if (run("far outside: every other binade, 0, inf", h, d_x, d_c, false, bad)) return 2;
  printf("%s\n", bad ? "FAILED: the in-band forms differ from the IEEE forms inside the band" : "inside the band and on its edges: 0 results differ");
  (void)bits;
  return bad ? 1 : 0;
}
