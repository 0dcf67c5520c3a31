// ffx_trace.hip — K7 (primary visibility), K8 (render), K9 (render adjoint) for gfx950.
//
// Replaces sensor.sample_ray + scene.ray_intersect (fireflies/graphics/depth.py:35-46,72-84,
// 110-125,152-165) and mi.render / its Dr.Jit backward (examples/vocalfold_scene.py:69,102;
// main.py:156) — all Mitsuba [EXT].  The arithmetic of ray generation, the triangle test and
// shading follows the same documented operation order as oracle/ffx_oracle.c, so
// depths and ids agree with the oracle bit for bit apart from rare 1-ulp boundary cases.
//
// Execution model.  The render kernels and K7 are WAVE-PACKET kernels: one wavefront = the 64
// samples of one pixel (or a compact pixel block at low spp), wave-uniform control flow.  Their default
// traversal is the 64-wide walk (lanes test 64 child boxes of a wide node against the packet as a whole; exact
// triangle tests with the lanes back on the rays), falling back to the binary packet walk (scalar-cache node
// fetch, per-ray box tests with the node as SGPR operands, VGPR lane stack) for packets the interval test is bad
// at.  The per-lane kernels further down (one lane = one ray, LDS stack) serve arbitrary rays (k_trace_rays)
// and remain as the A/B baseline (FFX_TRAVERSAL=lane).
// XCD placement: giving each XCD a contiguous band of the image (FFX_XCD_REMAP=1) costs 30 % here: tile cost varies
// by 10x across the image, so whole XCDs idle while the one that owns the vocal folds finishes.  Default
// (FFX_XCD_REMAP=128): within every 1024 consecutive one-wave workgroups each XCD walks 128 CONSECUTIVE ones — a
// 16x8-pixel patch — so the four waves of a 2x2-pixel tile and their neighbours share an L2: as fast as the plain
// round-robin deal (+0..2 %), a third of its HBM traffic (FETCH 37 -> 13.5 MB, WRITE 10.2 -> 3.1 MB per launch).
#include <stdlib.h>
#include <string.h>

#include <limits.h>
#include <mutex>

#include "ffx_common.h"
#include "ffx_band.h"
#include "ffx_rect.h"
#include "../../include/ffx_labels.h" // ffx_trace_rays_bwd

#define TR_BLOCK 256
#define RAY_EPS 8.940696716308594e-05f
#define SHADOW_EPS (10.0f * RAY_EPS)

struct CamK {
  float s2c[16];
  float tw[12]; // rows 0..2 of to_world
  float near_clip, far_clip, inv_w, inv_h;
  int W, H;
  // a perspective sensor's sample_to_camera has m12 = m13 = 0: the homogeneous w of a near-plane point is the constant m15 and
  // 1 / w is formed once on the host (the same IEEE quotient the per-sample division gave: identical rays).  Measured with
  // tools/k8ab.py: within the noise (the ten VALU it saves are 0.7 % of a pixel's) — kept because it is free.
  int w_uniform;
  float iw_u;
};

// the gaussian reconstruction filter's constants (ffx_scene_desc.rfilter): g(x) = max(0, exp(alpha x^2) - bias).  A sample needs the five weights
// of its window along each axis, at x0 + a, a = 0..4: instead of five exponentials, exp(alpha (x + 1)^2) = exp(alpha x^2) exp(2 alpha x) exp(alpha)
// — two exponentials and eight multiplies with k[n] = exp(alpha (2 n + 1)) from the host (round 5; `rec`: |alpha| <= 8, i.e. stddev >= 0.25:
// the factor exp(2 alpha x0) stays inside float's range — narrower filters keep the five exponentials).  Every kernel that forms weights
// calls rf_weights, so forward, adjoint and cache agree bit for bit; the oracle's five expf differ in the last bits (1e-6 of a weight).
struct RfC { float alpha, bias, aL, aL2, k[4]; int rec; };
// the columns of a pre-row (ShadeK.mat_pre; mat_pre_row fills them, RowPre reads them), m1 = 1 - metallic: eta, 1 / eta^2, a2 = max(0.001, roughness^2)^2, 1 / a2,
// metallic, the Fresnel mix's coefficients of the Schlick weight (metallic + m1 spec_tint) and of the dielectric term (m1 (1 - spec_tint)), the diffuse weight
// m1 (1 - spec_trans), 2 roughness, the lobe flags below (an integer's bits), roughness^2, the tint term m1 spec_tint ((eta - 1) / (eta + 1))^2
enum { FFX_PRE_ETA, FFX_PRE_INV_ETA2, FFX_PRE_A2, FFX_PRE_INV_A2, FFX_PRE_METALLIC, FFX_PRE_C_SW, FFX_PRE_C_FD, FFX_PRE_BRDF, FFX_PRE_ROUGH2, FFX_PRE_FLAGS, FFX_PRE_R2,
       FFX_PRE_TINT_TERM, FFX_PRE_FLOATS /* floats per pre-row */ };
#define FFX_PRE_ANISO 1u
#define FFX_PRE_TINT 2u
#define FFX_PRE_CLEARCOAT 4u
#define FFX_PRE_FLAT 8u
#define FFX_PRE_SHEEN 16u
struct ShadeK {
  CamK cam;
  int proj_on, spot_on, shadows;
  float p_w2l[12];
  float p_c2s[16];
  float p_pos[3], p_axis[3], p_color[3];
  float p_scale;
  int tw, th, tc;
  float s_w2l[12];
  float s_pos[3], s_int[3];
  float cos_cut, cos_beam, cutoff, inv_trans;
  int s_rigid; // the 3x3 part of s_w2l is a rotation (orthonormal rows to 2e-6): the packet kernels take the cosine to the spot's axis from its third row alone
  int mat_stride;    // floats per row of the material table: 3 (Lambert albedo) or FFX_MAT_STRIDE
  const float *mats; // the material table (the render calls' shape_albedo)
  // texture-valued base colours (ffx_scene_desc.base_tex): rows select one with FFX_MAT_BASE_TEX
  int n_base_tex;
  int btw[FFX_MAX_BASE_TEX], bth[FFX_MAX_BASE_TEX];
  const float *btex[FFX_MAX_BASE_TEX];
  const float *slot_uv;
  // the material table as a kernel argument (ffx_scene_desc.mat_h): the kernels then read the rows from their own kernarg segment
  int mat_inline;
  float mat_h[FFX_MAX_MAT_H];
  // per-row constants of the inline material rows (round 5; shade_prepare -> mat_pre_row): what every BSDF evaluation of a row re-derived from its
  // parameters — alpha^2 and its reciprocal, 1 / eta^2, the Fresnel mix's coefficients, the diffuse weight, which optional lobes are on
  int mat_pre_on;
  float mat_pre[8 * FFX_PRE_FLOATS];
  // tile bins of the three apexes (ffx_common.h BinsK): the packet kernels try them before the tree walks
  BinsK bins;
  // reconstruction filter (ffx_scene_desc.rfilter = gaussian; the *_filtered entry points only): g(x) = max(0, exp(rf_alpha x^2) - rf_bias)
  RfC rf;
};
// The first kernel argument, read in place.  The scene constants (ShadeK, ~100 dwords + the inline material rows) are the first
// argument of the render kernels.  Read through the by-value copy the compiler loads them all up front and, out of SGPRs, parks
// them in VGPR lanes (v_writelane / v_readlane: ~480 spill instructions on the VALU, the unit that bounds these kernels); through
// this pointer — which the compiler cannot see through — each phase re-reads what it needs with scalar loads from the kernarg
// segment (no VALU work at all), and per-lane indexed tables (the material rows) are ordinary global loads from it.
template <typename T>
__device__ __forceinline__ const T &kernarg_first() {
  const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const T *)p;
}
__device__ __forceinline__ const ShadeK &kernarg_shade() { return kernarg_first<ShadeK>(); }
// What the plain-scene instances of k_render_fwd_pk read instead of forming it per pixel or per walk (rect_tables): the film's pixel-rectangle
// tables (ffx_rect.h: W column entries, then H row entries from entry `row0`) with their two half extents, and the grids' sizes as the floats
// bins_shadow compares against.  It is k_render_fwd_pk's LAST argument — behind every other one, so no existing kernarg offset moves and no other
// kernel's code does — and is read in place like the first (kernarg_rect, defined behind the kernel).
struct RectK { const void *tab; float hx, hy; uint32_t row0, pad; float gxf[FFX_N_APEX], gyf[FFX_N_APEX]; };
__device__ __forceinline__ const RectK &kernarg_rect();
// the material table of a launch: its own kernel arguments, or the caller's device array
__device__ __forceinline__ const float *mat_table(const ShadeK &k) { return k.mat_inline ? k.mat_h : k.mats; }

struct Hit { float t; int prim, shape, slot; };

// ------------------------------------------------------------------------------------------ traversal
// Ray/box slab test, t = (plane - o) * (1/d): exact cancellation at the origin, so no absolute pad is
// needed; the far side is widened by 2 ulp.  A direction component of (nearly) zero is replaced by
// +-1e-20 FOR THE BOX TEST ONLY: 1/d stays finite, planes the origin lies between give t = -/+ huge
// (axis imposes no constraint) and planes it lies outside of give same-signed huge values (box
// rejected).  With 1/0 = inf the products 0*inf = NaN would silently drop the axis and such rays
// (every pixel-corner ray of the centre row / column when jitter is off) would walk the whole tree.
struct RayBox { v3 o, id; };
// The walks that use this test (the per-lane walk and the generic packet walk) cull a box against the current hit distance WIDENED by 3 ulp,
// like the octant and wide walks (their `sw`): a box that ends exactly on the hit — a flat box in a coordinate plane, which the refit's
// relative pad leaves as it is — has the entry distance (plane - o) * rcp(d), rounded up to three times where t = T/det is rounded once, and
// may hold a triangle at the same t with a smaller id.  Against the bare distance the tie was dropped on one such ray in five
// (tests/tie_scenes.py: sheets_far_from_their_plane).
#define FFX_TIE_WIDEN 1.0000004f
__device__ __forceinline__ float safe_rcp_dir(float d) {
  float a = fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d;
  return __builtin_amdgcn_rcpf(a);
}
__device__ __forceinline__ RayBox make_raybox(v3 o, v3 d) {
  RayBox r;
  r.o = o;
  r.id = V3(safe_rcp_dir(d.x), safe_rcp_dir(d.y), safe_rcp_dir(d.z));
  return r;
}
__device__ __forceinline__ bool slab(const float lo[3], const float hi[3], const RayBox &rb, float tmin, float tmax, float &tn_out) {
  float ax = (lo[0] - rb.o.x) * rb.id.x, bx = (hi[0] - rb.o.x) * rb.id.x;
  float ay = (lo[1] - rb.o.y) * rb.id.y, by = (hi[1] - rb.o.y) * rb.id.y;
  float az = (lo[2] - rb.o.z) * rb.id.z, bz = (hi[2] - rb.o.z) * rb.id.z;
  float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
  float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.0000004f;
  tf = fminf(tf, tmax);
  tn_out = tn;
  return tn <= tf;
}

// Moller-Trumbore, division-free rejection; identical order to the oracle.
__device__ __forceinline__ bool tri_hit(const TriRec *__restrict__ rec, v3 o, v3 d, float tmin, float &t_out, int &prim, int &shape) {
  const float4 *r4 = reinterpret_cast<const float4 *>(rec);
  float4 a = r4[0], b = r4[1], c = r4[2];
  v3 v0 = V3(a.x, a.y, a.z), e1 = V3(a.w, b.x, b.y), e2 = V3(b.z, b.w, c.x);
  v3 pv = vcross(d, e2);
  float det = vdot(e1, pv);
  v3 tv = vsub(o, v0);
  v3 qv = vcross(tv, e1);
  float U = vdot(tv, pv), Vv = vdot(d, qv), T = vdot(e2, qv);
  if (det < 0.f) { det = -det; U = -U; Vv = -Vv; T = -T; }
  if (!(det > 0.f)) return false;
  if (!(U >= 0.f) || !(Vv >= 0.f) || !(U + Vv <= det)) return false;
  float t = T / det;
  if (!(t > tmin)) return false;
  t_out = t;
  prim = __float_as_int(c.y);
  shape = __float_as_int(c.z);
  return true;
}

// The same test for rays that share their origin with a whole batch (primary rays: the camera; shadow
// rays: the emitter they are traced from): Moller-Trumbore's scalars as three dot products with the
// triangle's APEX vectors (ffx_common.h).  The apex vectors are formed here in the same order as in
// k_apex_records and the oracle, so all three produce identical bits.
struct ApexVec { v3 A, B, C; float T; };
__device__ __forceinline__ ApexVec apex_vectors(v3 v0, v3 e1, v3 e2, v3 o) {
  ApexVec a;
  a.A = vcross(e2, e1);
  const v3 tv = vsub(o, v0);
  a.B = vcross(e2, tv);
  a.C = vcross(tv, e1);
  a.T = vdot(e2, a.C);
  return a;
}
__device__ __forceinline__ bool tri_hit_apex(const TriRec *__restrict__ rec, v3 o, v3 d, float tmin, float &t_out, int &prim, int &shape) {
  const float4 *r4 = reinterpret_cast<const float4 *>(rec);
  float4 a = r4[0], b = r4[1], c = r4[2];
  const ApexVec av = apex_vectors(V3(a.x, a.y, a.z), V3(a.w, b.x, b.y), V3(b.z, b.w, c.x), o);
  float det = vdot(d, av.A), U = vdot(d, av.B), Vv = vdot(d, av.C), T = av.T;
  if (det < 0.f) { det = -det; U = -U; Vv = -Vv; T = -T; }
  if (!(det > 0.f)) return false;
  if (!(U >= 0.f) || !(Vv >= 0.f) || !(U + Vv <= det)) return false;
  float t = T / det;
  if (!(t > tmin)) return false;
  t_out = t;
  prim = __float_as_int(c.y);
  shape = __float_as_int(c.z);
  return true;
}

// ANY = false: closest hit in (tmin, tmax], ties broken by the smaller primitive id.
// ANY = true : returns true as soon as a hit with tmin < t < tmax is found.
// `stack` points at this lane's first slot; consecutive entries are `stride` ints apart.
// APEX: the ray origin is a batch-wide apex (see tri_hit_apex); false for arbitrary rays.
template <bool ANY, bool APEX>
__device__ __forceinline__ bool traverse(const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, v3 o, v3 d, float tmin, float tmax, Hit &h,
                                         int *stack, int stride) {
  h.t = tmax;
  h.prim = -1;
  h.shape = -1;
  h.slot = -1;
  const RayBox rb = make_raybox(o, d);
  int sp = 0;
  int cur = 0;
  while (true) {
    const float4 *n4 = reinterpret_cast<const float4 *>(nodes + cur);
    float4 q0 = n4[0], q1 = n4[1], q2 = n4[2];
    int4 ch = *reinterpret_cast<const int4 *>(n4 + 3);
    float lo0[3] = {q0.x, q0.y, q0.z}, hi0[3] = {q0.w, q1.x, q1.y};
    float lo1[3] = {q1.z, q1.w, q2.x}, hi1[3] = {q2.y, q2.z, q2.w};
    float t0, t1;
    bool h0 = (ch.x != FFX_EMPTY_CHILD) && slab(lo0, hi0, rb, tmin, h.t * FFX_TIE_WIDEN, t0);
    bool h1 = (ch.y != FFX_EMPTY_CHILD) && slab(lo1, hi1, rb, tmin, h.t * FFX_TIE_WIDEN, t1);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      int c = side ? ch.y : ch.x;
      bool hs = side ? h1 : h0;
      if (hs && c < 0) {
        uint32_t lc = (uint32_t)~c;
        int first = (int)(lc >> 3), count = (int)(lc & 7u) + 1;
        for (int i = 0; i < count; ++i) {
          float t;
          int prim, shape;
          if (APEX ? tri_hit_apex(recs + first + i, o, d, tmin, t, prim, shape) : tri_hit(recs + first + i, o, d, tmin, t, prim, shape)) {
            if (ANY) {
              if (t < tmax) return true;
            } else if (t <= tmax && (h.prim < 0 || t < h.t || (t == h.t && prim < h.prim))) {
              h.t = t; h.prim = prim; h.shape = shape; h.slot = first + i;
            }
          }
        }
        if (side) h1 = false; else h0 = false;
      }
    }
    // a leaf may have shortened the ray: drop inner children that now start behind the hit
    if (h0 && t0 > h.t * FFX_TIE_WIDEN) h0 = false;
    if (h1 && t1 > h.t * FFX_TIE_WIDEN) h1 = false;
    if (h0 && h1) {
      int nearc = ch.x, farc = ch.y;
      if (t1 < t0) { nearc = ch.y; farc = ch.x; }
      stack[sp * stride] = farc;
      ++sp;
      cur = nearc;
    } else if (h0) {
      cur = ch.x;
    } else if (h1) {
      cur = ch.y;
    } else {
      if (sp == 0) break;
      --sp;
      cur = stack[sp * stride];
    }
  }
  return h.prim >= 0;
}

// ------------------------------------------------------------------------------------------ camera
__device__ __forceinline__ void sample_jitter(uint32_t seed_key, uint32_t idx, float &jx, float &jy) {
  uint32_t a = hash32((2u * idx) ^ seed_key), b = hash32((2u * idx + 1u) ^ seed_key);
  jx = (float)(a >> 8) * (1.0f / 16777216.0f);
  jy = (float)(b >> 8) * (1.0f / 16777216.0f);
}

// The plain-scene instance's two launch-proven diets, each with a build switch for single-item A/B libraries (tools/build_variant_lib.sh -D...; not
// run-time knobs): -DFFX_K8_NO_BAND keeps cam_ray's IEEE forms, -DFFX_K8_NO_OFF32 keeps the 64-bit texel and record addresses.
#ifdef FFX_K8_NO_BAND
#define FFX_K8_BAND false
#else
#define FFX_K8_BAND true
#endif
#ifdef FFX_K8_NO_OFF32
#define FFX_K8_OFF32 false
#else
#define FFX_K8_OFF32 true
#endif
// ... and a third: -DFFX_K8_NO_RECTTAB keeps the per-pixel arithmetic of the bin rectangle (and the uniform work next to it) that the plain-scene
// instances otherwise take from the film's tables (ffx_rect.h, rect_tables below).
#ifdef FFX_K8_NO_RECTTAB
#define FFX_K8_RECTTAB false
#else
#define FFX_K8_RECTTAB true
#endif
// (its parts beside the tables, for single-item A/B libraries as well: -DFFX_K8_NO_RECT_UNI keeps the tile origin per pixel and the vector form of the
// `live` test, -DFFX_K8_NO_RECT_GF the conversion of the grids' sizes per shadow walk, -DFFX_K8_NO_RECT_SL the vector loads of the bins' header words
// and list bounds)
#ifdef FFX_K8_NO_RECT_UNI
#define FFX_K8_RECT_UNI false
#else
#define FFX_K8_RECT_UNI true
#endif
#ifdef FFX_K8_NO_RECT_GF
#define FFX_K8_RECT_GF false
#else
#define FFX_K8_RECT_GF true
#endif
#ifdef FFX_K8_NO_RECT_SL
#define FFX_K8_RECT_SL false
#else
#define FFX_K8_RECT_SL true
#endif
// (rcp_band, sqrt_band: ffx_band.h — the IEEE expansions of 1.0f / d and sqrtf(x) without the steps that do nothing inside the camera's band)
// BAND (k_render_fwd_pk's plain-scene instance only): the launch proved w_uniform and the band of |np|^2, |np| and dl.z
template <bool BAND = false>
__device__ __forceinline__ void cam_ray(const CamK &k, float sx, float sy, v3 &o, v3 &d, float &near_t, float &far_t) {
  const float *m = k.s2c;
  float qx = fmaf(m[0], sx, fmaf(m[1], sy, m[3]));
  float qy = fmaf(m[4], sx, fmaf(m[5], sy, m[7]));
  float qz = fmaf(m[8], sx, fmaf(m[9], sy, m[11]));
  // one IEEE reciprocal + multiplies instead of a division per component (same order as the oracle)
  float iw;
  if (BAND || k.w_uniform) iw = k.iw_u; // (wave-uniform branch)
  else iw = 1.0f / fmaf(m[12], sx, fmaf(m[13], sy, m[15]));
  v3 np = V3(qx * iw, qy * iw, qz * iw);
  const float il = BAND ? rcp_band(sqrt_band(vdot(np, np))) : 1.0f / sqrtf(vdot(np, np));
  v3 dl = V3(np.x * il, np.y * il, np.z * il);
  d = xf_dir(k.tw, dl);
  o = V3(k.tw[3], k.tw[7], k.tw[11]);
  const float idz = BAND ? rcp_band(dl.z) : 1.0f / dl.z;
  near_t = k.near_clip * idz;
  far_t = k.far_clip * idz;
}

// ------------------------------------------------------------------------------------------ K7 kernels
__global__ void __launch_bounds__(TR_BLOCK)
    k_trace_primary(CamK cam, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, int spp, int jitter, uint32_t seed_key, long total,
                    float *__restrict__ t_out, int32_t *__restrict__ shape_out, int32_t *__restrict__ prim_out) {
  extern __shared__ int s_stack[];
  long idx = (long)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (idx >= total) return;
  long pix = idx / spp;
  int x = (int)(pix % cam.W), y = (int)(pix / cam.W);
  float jx = 0.f, jy = 0.f;
  if (jitter) sample_jitter(seed_key, (uint32_t)idx, jx, jy);
  v3 o, d;
  float nt, ft;
  cam_ray(cam, ((float)x + jx) * cam.inv_w, ((float)y + jy) * cam.inv_h, o, d, nt, ft);
  Hit h;
  bool hit = traverse<false, true>(nodes, recs, o, d, nt, ft, h, s_stack + threadIdx.x, TR_BLOCK);
  t_out[idx] = hit ? (h.t - nt) : 0.f;
  if (shape_out) shape_out[idx] = h.shape;
  if (prim_out) prim_out[idx] = h.prim;
}

__global__ void __launch_bounds__(TR_BLOCK)
    k_trace_rays(const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const float *__restrict__ org, const float *__restrict__ dir, int n,
                 float tmax, float *__restrict__ t_out, int32_t *__restrict__ shape_out, int32_t *__restrict__ prim_out) {
  extern __shared__ int s_stack[];
  int i = blockIdx.x * TR_BLOCK + threadIdx.x;
  if (i >= n) return;
  Hit h;
  bool hit = traverse<false, false>(nodes, recs, V3(org[3 * i], org[3 * i + 1], org[3 * i + 2]), V3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]), 0.f, tmax, h,
                                    s_stack + threadIdx.x, TR_BLOCK);
  t_out[i] = hit ? h.t : 0.f;
  if (shape_out) shape_out[i] = h.shape;
  if (prim_out) prim_out[i] = h.prim;
}

// Adjoint of k_trace_rays's t with respect to the rays (ffx_trace_rays_bwd): the hit stays on the plane of its triangle,
// t = N . (v0 - o) / (N . d) with N = e1 x e2, so dt/do = -N / (N . d) and dt/dd = -t N / (N . d).  A lane per ray.  The forward returns the
// primitive's id, the records lie in leaf order: the lane walks the tree again with the forward's t as the far end — the boxes are culled
// against the hit from the first step, the walk visits a handful of nodes — and takes the record of the hit it finds, which is the forward's
// (same tests, same tie-break).  A miss, or a walk that ends on another primitive than the forward named (the pose changed in between):
// zeros.  The quotients are formed in binary64 from the record's binary32 edges.
__global__ void __launch_bounds__(TR_BLOCK)
    k_trace_rays_bwd(const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const float *__restrict__ org, const float *__restrict__ dir, int n,
                     const float *__restrict__ t_in, const int32_t *__restrict__ prim_in, const float *__restrict__ gt, float *__restrict__ gorig,
                     float *__restrict__ gdir) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * TR_BLOCK + threadIdx.x;
  if (i >= n) return;
  double go[3] = {0.0, 0.0, 0.0}, gd[3] = {0.0, 0.0, 0.0};
  const int prim = prim_in[i];
  const float t = t_in[i];
  if (prim >= 0 && t > 0.f) {
    const v3 o = V3(org[3 * i], org[3 * i + 1], org[3 * i + 2]), d = V3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    Hit h;
    if (traverse<false, false>(nodes, recs, o, d, 0.f, t, h, s_stack + threadIdx.x, TR_BLOCK) && h.prim == prim) {
      const float4 *r4 = reinterpret_cast<const float4 *>(recs + h.slot);
      const float4 a = r4[0], b = r4[1], c = r4[2];
      const double e1[3] = {a.w, b.x, b.y}, e2[3] = {b.z, b.w, c.x};
      const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const double nd = N[0] * (double)d.x + N[1] * (double)d.y + N[2] * (double)d.z;
      const double s = -(double)gt[i] / nd;
#pragma unroll
      for (int c3 = 0; c3 < 3; ++c3) { go[c3] = s * N[c3]; gd[c3] = s * (double)t * N[c3]; }
    }
  }
#pragma unroll
  for (int c3 = 0; c3 < 3; ++c3) { gorig[3 * i + c3] = (float)go[c3]; gdir[3 * i + c3] = (float)gd[c3]; }
}

// ------------------------------------------------------------------------------------------ shading
#define FFX_PI_F 3.14159265358979323846f
// Reciprocal, quotient and square root of the shading terms: the hardware seed (v_rcp / v_sqrt / v_rsq,
// 1 ulp) plus one fma Newton step.  The result equals the correctly rounded IEEE value except in rare
// last-bit cases (Markstein), at 3 / 5 / 7 VALU instructions instead of the 10 / 10 / 14 of the
// compiler's IEEE expansions (which also cover denormal and overflow ranges that cannot occur here:
// arguments are lengths and depths of visible surface points).  Ray generation and the triangle test
// keep the IEEE forms: they decide WHICH primitive is hit.
__device__ __forceinline__ float rcp_nr(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(r, fmaf(-x, r, 1.0f), r);
}
__device__ __forceinline__ float div_nr(float a, float b) {
  const float r = rcp_nr(b);
  const float q = a * r;
  return fmaf(fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ float sqrt_nr(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float h = 0.5f * __builtin_amdgcn_rsqf(x);
  const float s1 = fmaf(fmaf(-s, s, x), h, s);
  return x > 0.f ? s1 : s; // sqrt(0) = 0 (rsq(0) = inf would give NaN)
}
// 1 / sqrt(x) of a squared emitter distance (x > 0): the hardware seed plus one Newton step — five instructions where rcp_nr(sqrt_nr(x)) took ten
// (two transcendental seeds, two refinements), the same value to the last bit or two
__device__ __forceinline__ float rsqrt_nr(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  return fmaf(0.5f * y, fmaf(-(x * y), y, 1.0f), y);
}

// Shading normal of a hit on a record flagged by ffx_smooth (include/ffx.h): the three vertex normals stored next to the
// record, interpolated with Moller-Trumbore's barycentrics of the hit (P = v0 + u e1 + v e2, recomputed here from the record:
// the walks do not carry them), normalised and faced to the viewer by the sign of ITS OWN cosine (the `twosided` wrapper flips
// in the shading frame).  Same operation order as the oracle's shade_sample; FAST: the Newton-refined reciprocals of the packet
// kernels instead of IEEE division (equal except for rare last bits).  A zero-length interpolated normal keeps the geometric one.
template <bool FAST>
__device__ __forceinline__ void hit_barycentrics(float4 ra, float4 rb, float4 rc, v3 o, v3 d, float &bu, float &bv) {
  const v3 e1 = V3(ra.w, rb.x, rb.y), e2 = V3(rb.z, rb.w, rc.x);
  const v3 pv = vcross(d, e2);
  const float det = vdot(e1, pv);
  const v3 tv = vsub(o, V3(ra.x, ra.y, ra.z));
  const v3 qv = vcross(tv, e1);
  const float idet = FAST ? rcp_nr(det) : 1.0f / det;
  bu = vdot(tv, pv) * idet;
  bv = vdot(d, qv) * idet;
}
// base colour of a hit on a row with FFX_MAT_BASE_TEX = k + 1 (ffx.h ffx_scene_desc.base_tex): the slot's texture coordinates
// interpolated with the hit's barycentrics, repeat wrap, bilinear between texel centres — the oracle's base_tex_lookup
__device__ __forceinline__ void base_tex_sample(const ShadeK &c, int k, int slot, float bu, float bv, float (&rgb)[3]) {
  const float *uv = c.slot_uv + 6 * (size_t)slot;
  const float bw = (1.0f - bu) - bv;
  float u = fmaf(bw, uv[0], fmaf(bu, uv[2], bv * uv[4])), v = fmaf(bw, uv[1], fmaf(bu, uv[3], bv * uv[5]));
  u = u - floorf(u);
  v = v - floorf(v);
  const int w = c.btw[k], h = c.bth[k];
  const float fx = fmaf(u, (float)w, -0.5f), fy = fmaf(v, (float)h, -0.5f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1; // in [-1, w]: one conditional step wraps them
  x0 = x0 < 0 ? x0 + w : x0; x1 = x1 >= w ? x1 - w : x1; y0 = y0 < 0 ? y0 + h : y0; y1 = y1 >= h ? y1 - h : y1;
  x0 = x0 >= w ? x0 - w : x0; y0 = y0 >= h ? y0 - h : y0; x1 = x1 < 0 ? x1 + w : x1; y1 = y1 < 0 ? y1 + h : y1;
  const float *t = c.btex[k];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float t00 = t[((size_t)y0 * w + x0) * 3 + ch], t01 = t[((size_t)y0 * w + x1) * 3 + ch];
    const float t10 = t[((size_t)y1 * w + x0) * 3 + ch], t11 = t[((size_t)y1 * w + x1) * 3 + ch];
    rgb[ch] = (1.0f - ay) * ((1.0f - ax) * t00 + ax * t01) + ay * ((1.0f - ax) * t10 + ax * t11);
  }
}
template <bool FAST>
__device__ __forceinline__ v3 interpolated_normal(const float4 *__restrict__ nrec, int slot, float4 ra, float4 rb, float4 rc, v3 o, v3 d, v3 ng) {
  float bu, bv;
  hit_barycentrics<FAST>(ra, rb, rc, o, d, bu, bv);
  const float bw = (1.0f - bu) - bv;
  const float4 n0 = nrec[3 * (size_t)slot], n1 = nrec[3 * (size_t)slot + 1], n2 = nrec[3 * (size_t)slot + 2];
  const v3 ni = V3(fmaf(bw, n0.x, fmaf(bu, n1.x, bv * n2.x)), fmaf(bw, n0.y, fmaf(bu, n1.y, bv * n2.y)), fmaf(bw, n0.z, fmaf(bu, n1.z, bv * n2.z)));
  const float l2 = vdot(ni, ni);
  if (!(l2 > 0.f)) return ng;
  const float il = FAST ? rcp_nr(sqrt_nr(l2)) : 1.0f / sqrtf(l2);
  v3 ns = V3(ni.x * il, ni.y * il, ni.z * il);
  if (vdot(ns, d) > 0.f) ns = V3(-ns.x, -ns.y, -ns.z);
  return ns;
}

// BSDF of a material row (include/ffx.h FFX_MAT_*, model 1: the reflection side of Mitsuba's `principled`), for the
// viewer direction wv and an emitter direction wl at a surface with unit normal n facing the viewer:
//     pi * f(wv, wl) * cos_o = base_color * A + B   per colour channel.
// The model is material_eval of oracle/ffx_oracle.c (which cites its sources), arranged for the kernel:
//   * the directions are reduced to five cosines (MatGeo) first — for both emitters, so that the surface point, the normal
//     and the ray die before the lobes are evaluated; the lobes then run one after the other on those scalars;
//   * Smith's G1 is taken as 2 c / (c + sqrt(c^2 + xy)) (= 2 / (1 + sqrt(1 + xy / c^2))), so the specular lobe
//     D G / (4 cos_i) collapses to D cos_o / ((cos_i + s_i)(cos_o + s_o)): one quotient instead of five;
//   * an isotropic material (anisotropic = 0, the plugin's default) needs no tangent frame at all;
//   * quotients and roots are the bare hardware seeds (brcp / bdiv / bsqrt below).
// Equal to the oracle within a few ulp per term (the parity tests state the tolerance).  The caller handles model 0.
__device__ __forceinline__ float sqrf(float x) { return x * x; }
__device__ __forceinline__ float schlick_weight(float c) {
  float m = 1.0f - c;
  m = fminf(fmaxf(m, 0.f), 1.f);
  return sqrf(sqrf(m)) * m;
}
// reciprocal, quotient and square root inside the BSDF: the bare hardware seeds (1 ulp) — the BSDF scales a sample's
// radiance, it does not decide what is hit, and the parity tests state its tolerance
__device__ __forceinline__ float brcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float bdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float bsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// geometry of one (viewer, emitter) pair — all the BSDF needs of the directions, as scalars: five cosines and the three
// GGX quadratic forms (which take the tangent frame for an anisotropic material: formed here, where the vectors are)
struct MatGeo {
  float cos_i, cos_o, ch, ci_h, co_h; // n.wv, n.wl, n.h, wv.h, wl.h
  float tmp, xy_i, xy_o, axay;        // (hx/ax)^2 + (hy/ay)^2 + hz^2, (ax ix)^2 + (ay iy)^2, the same for wl, ax * ay
  float s2;                           // sin^2(theta_h) = hx^2 + hy^2 — NEVER as 1 - ch^2: near-mirror rows (alpha = 0.0025) and a glossy
                                      // clearcoat (alpha = 0.001) divide it by alpha^2, which turned the rounding of ch into 0.4 % of a highlight
};
static __constant__ constexpr float FFX_LUM_W[3] = {0.212671f, 0.715160f, 0.072169f}; // the luminance weights w of the tint terms
__device__ __forceinline__ float lum3(float r, float g, float b) { return FFX_LUM_W[0] * r + FFX_LUM_W[1] * g + FFX_LUM_W[2] * b; }
// where the BSDF takes a row's constants from.  RowRaw: the material row m itself, derived per evaluation with the hardware seeds.  RowPre: the row
// plus the constants the host has derived from it once (ShadeK.mat_pre, columns FFX_PRE_*): no squares, clamps and reciprocals of parameters per
// evaluation, one flag word instead of five parameter loads and compares — with the host's IEEE values where RowRaw forms hardware seeds (a
// last-bit difference in 1 / a2, 1 / eta^2 and the tint term, inside the parity tolerance).  PLAIN (k_render_fwd_pk's plain-scene instance): the
// host found no lobe flag set in any row — the flag word is the constant 0, the optional lobes' tests and arms are not compiled
struct RowRaw {
  const float *__restrict__ m;
  __device__ __forceinline__ float m1() const { return 1.0f - m[FFX_MAT_METALLIC]; }
  __device__ __forceinline__ bool aniso() const { return m[FFX_MAT_ANISOTROPIC] != 0.f; }
  __device__ __forceinline__ bool tint() const { return m[FFX_MAT_SPEC_TINT] != 0.f; }
  __device__ __forceinline__ bool clearcoat() const { return m[FFX_MAT_CLEARCOAT] > 0.f; }
  __device__ __forceinline__ bool flat() const { return m[FFX_MAT_FLATNESS] > 0.f; }
  __device__ __forceinline__ bool sheen() const { return m[FFX_MAT_SHEEN] > 0.f && m1() > 0.f; }
  __device__ __forceinline__ float r2() const { return sqrf(m[FFX_MAT_ROUGHNESS]); }
  __device__ __forceinline__ float a2() const { return sqrf(fmaxf(0.001f, r2())); }
  __device__ __forceinline__ float tmp_iso(float s2, float ch) const { return bdiv(s2, a2()) + sqrf(ch); }
  __device__ __forceinline__ float rough2() const { return 2.0f * m[FFX_MAT_ROUGHNESS]; }
  __device__ __forceinline__ float eta() const { return m[FFX_MAT_ETA]; }
  __device__ __forceinline__ float inv_eta2() const { return sqrf(brcp(eta())); }
  __device__ __forceinline__ float metallic() const { return m[FFX_MAT_METALLIC]; }
  __device__ __forceinline__ float Fb(float sw, float F_d) const { return metallic() * sw + m1() * m[FFX_MAT_SPEC_TINT] * sw + m1() * (1.0f - m[FFX_MAT_SPEC_TINT]) * F_d; }
  __device__ __forceinline__ float tint_term() const { return m1() * m[FFX_MAT_SPEC_TINT] * sqrf((eta() - 1.0f) * brcp(eta() + 1.0f)); }
  __device__ __forceinline__ float brdf() const { return m1() * (1.0f - m[FFX_MAT_SPEC_TRANS]); }
};
template <bool PLAIN = false>
struct RowPre {
  const float *__restrict__ m, *__restrict__ p;
  __device__ __forceinline__ uint32_t flags() const { return PLAIN ? 0u : __float_as_uint(p[FFX_PRE_FLAGS]); }
  __device__ __forceinline__ bool aniso() const { return flags() & FFX_PRE_ANISO; }
  __device__ __forceinline__ bool tint() const { return flags() & FFX_PRE_TINT; }
  __device__ __forceinline__ bool clearcoat() const { return flags() & FFX_PRE_CLEARCOAT; }
  __device__ __forceinline__ bool flat() const { return flags() & FFX_PRE_FLAT; }
  __device__ __forceinline__ bool sheen() const { return flags() & FFX_PRE_SHEEN; }
  __device__ __forceinline__ float r2() const { return p[FFX_PRE_R2]; }
  __device__ __forceinline__ float a2() const { return p[FFX_PRE_A2]; }
  __device__ __forceinline__ float tmp_iso(float s2, float ch) const { return fmaf(s2, p[FFX_PRE_INV_A2], sqrf(ch)); }
  __device__ __forceinline__ float rough2() const { return p[FFX_PRE_ROUGH2]; }
  __device__ __forceinline__ float eta() const { return p[FFX_PRE_ETA]; }
  __device__ __forceinline__ float inv_eta2() const { return p[FFX_PRE_INV_ETA2]; }
  __device__ __forceinline__ float metallic() const { return p[FFX_PRE_METALLIC]; }
  __device__ __forceinline__ float Fb(float sw, float F_d) const { return fmaf(p[FFX_PRE_C_SW], sw, p[FFX_PRE_C_FD] * F_d); }
  __device__ __forceinline__ float tint_term() const { return p[FFX_PRE_TINT_TERM]; }
  __device__ __forceinline__ float brdf() const { return p[FFX_PRE_BRDF]; }
};
template <class Row>
__device__ __forceinline__ void material_geometry(const Row &row, v3 n, v3 wv, v3 wl, MatGeo &g) {
  g.cos_i = vdot(n, wv);
  g.cos_o = vdot(n, wl);
  v3 wh = V3(wv.x + wl.x, wv.y + wl.y, wv.z + wl.z);
  const float ihl = __builtin_amdgcn_rsqf(vdot(wh, wh));
  wh = V3(wh.x * ihl, wh.y * ihl, wh.z * ihl);
  g.ci_h = vdot(wv, wh);
  g.co_h = vdot(wl, wh);
  g.ch = vdot(n, wh);
  if (row.aniso()) { // calc_dist_params + the shading frame coordinate_system(n)
    const float r2 = row.r2(), aspect = bsqrt(1.0f - 0.9f * row.m[FFX_MAT_ANISOTROPIC]);
    const float ax = fmaxf(0.001f, bdiv(r2, aspect)), ay = fmaxf(0.001f, r2 * aspect);
    const float sg = copysignf(1.0f, n.z), ca = -brcp(sg + n.z), cb = n.x * n.y * ca;
    const v3 fs = V3(sg * (sqrf(n.x) * ca) + 1.0f, sg * cb, -sg * n.x), ft = V3(cb, fmaf(n.y, n.y * ca, sg), -n.y);
    const float hx = vdot(wh, fs), hy = vdot(wh, ft);
    g.s2 = sqrf(hx) + sqrf(hy);
    g.tmp = sqrf(bdiv(hx, ax)) + sqrf(bdiv(hy, ay)) + sqrf(g.ch);
    g.xy_i = sqrf(ax * vdot(wv, fs)) + sqrf(ay * vdot(wv, ft));
    g.xy_o = sqrf(ax * vdot(wl, fs)) + sqrf(ay * vdot(wl, ft));
    g.axay = ax * ay;
  } else {
    const float a2 = row.a2();
    const v3 cx = vcross(n, wh); // |n x h|^2 = sin^2(theta_h), well conditioned at the peak (same order as the oracle's material_geometry)
    g.s2 = vdot(cx, cx);
    g.tmp = row.tmp_iso(g.s2, g.ch);
    g.xy_i = a2 * fmaxf(1.0f - sqrf(g.cos_i), 0.f);
    g.xy_o = a2 * fmaxf(1.0f - sqrf(g.cos_o), 0.f);
    g.axay = a2;
  }
}
__device__ __forceinline__ float ggx1_cc(float c, float c_dot_h) { // smith_ggx1 with alpha = 0.25 (clearcoat)
  const float c2 = sqrf(c);
  float r = bdiv(2.0f * c, c + bsqrt(c2 + 0.0625f * (1.0f - c2)));
  if (c_dot_h * c <= 0.f) r = 0.f;
  return r;
}
// the lobes, one after the other, each reading the material values it needs from the row when it needs them (the row is
// 64 bytes in the vector L1; holding all of it plus the directions in registers cost the kernel two waves of occupancy)
// TEX: the base colour is (b0, b1, b2) — the row's texture sampled at the hit — instead of the row's own m[0..2]
// TAU (the appearance adjoint): *tau receives pi tau, the numerators of the tint terms that A divides by lum (A = A0 + pi tau / lum;
// 0 when lum <= 0, where the tints went to B)
template <bool TEX = false, bool TAU = false, class Row>
__device__ __forceinline__ void material_terms(const Row &row, const MatGeo &g, float &A, float &B, float b0 = 0.f, float b1 = 0.f, float b2 = 0.f, float *tau = nullptr) {
  const float *__restrict__ m = row.m;
  const float cos_i = g.cos_i, cos_o = g.cos_o, ch = g.ch, ci_h = g.ci_h, co_h = g.co_h;
  A = 0.f; B = 0.f;
  if (TAU) *tau = 0.f;
  if (!(cos_i > 0.f && cos_o > 0.f)) return;
  const bool facing = ci_h > 0.f && co_h > 0.f; // (cos_i, cos_o > 0)
  float a = 0.f, b = 0.f, tu = 0.f;
  const float eta = row.eta();
  const float ct2 = 1.0f - (1.0f - ci_h * ci_h) * row.inv_eta2();
  const float ct = ct2 > 0.f ? bsqrt(ct2) : 0.f; // cosine of the transmitted direction
  const float sw = schlick_weight(eta > 1.0f ? fabsf(ci_h) : ct);
  float F_d;
  {
    const float c = fabsf(ci_h);
    const float ds = c + eta * ct, dp = ct + eta * c, ir = brcp(ds * dp); // one reciprocal for both amplitudes
    const float a_s = (c - eta * ct) * dp * ir, a_p = (ct - eta * c) * ds * ir;
    F_d = 0.5f * (a_s * a_s + a_p * a_p);
    if (eta == 1.0f) F_d = 0.f;
    else if (c == 0.f) F_d = 1.f;
  }
  const float metallic = row.metallic();
  if (facing && F_d > 0.f) { // main specular reflection lobe: F D G / (4 cos_i)
    const float dden = FFX_PI_F * g.axay * sqrf(g.tmp);
    const float s_i = bsqrt(sqrf(cos_i) + g.xy_i), s_o = bsqrt(sqrf(cos_o) + g.xy_o);
    // D G / (4 cos_i) = cos_o / (dden (cos_i + s_i)(cos_o + s_o))
    float common = bdiv(cos_o, dden * ((cos_i + s_i) * (cos_o + s_o)));
    if (!(ch > 1e-20f * dden)) common = 0.f; // D * cos_h > 1e-20
    float Fa = metallic * (1.0f - sw), Fb = row.Fb(sw, F_d); // Fb = (metallic + m1 spec_tint) sw + m1 (1 - spec_tint) F_d, m1 = 1 - metallic
    if (row.tint()) {
      const float lum = TEX ? lum3(b0, b1, b2) : lum3(m[0], m[1], m[2]);
      const float t = row.tint_term() * (1.0f - sw); // m1 spec_tint R0 (1 - sw)
      if (lum > 0.f) { Fa += bdiv(t, lum); if (TAU) tu += t * common; }
      else Fb += t;
    }
    a += Fa * common;
    b += Fb * common;
  }
  if (row.clearcoat() && facing) {
    const float cc = m[FFX_MAT_CLEARCOAT];
    const float Fcc = sw + (1.0f - sw) * 0.04f;
    const float alpha = 0.1f + (0.001f - 0.1f) * m[FFX_MAT_CLEARCOAT_GLOSS], a2 = sqrf(alpha), c2 = sqrf(ch);
    float Dcc = bdiv(a2 - 1.0f, FFX_PI_F * logf(a2) * (g.s2 + a2 * c2)); // GTR1: 1 + (a2 - 1) cos^2 = sin^2 + a2 cos^2, without the cancellation
    if (!(Dcc * ch > 1e-20f)) Dcc = 0.f;
    const float Gcc = ggx1_cc(cos_i, ci_h) * ggx1_cc(cos_o, co_h);
    b += cc * 0.25f * Fcc * Dcc * Gcc * cos_o;
  }
  const float brdf = row.brdf();
  if (brdf > 0.f) { // diffuse + retro-reflection (+ fake subsurface)
    const float Fo = schlick_weight(cos_o), Fi = schlick_weight(cos_i);
    const float f_diff = (1.0f - 0.5f * Fi) * (1.0f - 0.5f * Fo);
    const float Rr = row.rough2() * sqrf(co_h);
    const float f_retro = Rr * (Fo + Fi + Fo * Fi * (Rr - 1.0f));
    float dterm = f_diff + f_retro;
    if (row.flat()) {
      const float flat = m[FFX_MAT_FLATNESS];
      const float Fss90 = Rr * 0.5f;
      const float Fss = (1.0f + (Fss90 - 1.0f) * Fo) * (1.0f + (Fss90 - 1.0f) * Fi);
      const float f_ss = 1.25f * (Fss * (brcp(cos_o + cos_i) - 0.5f) + 0.5f);
      dterm = dterm + (f_ss - dterm) * flat;
    }
    a += brdf * cos_o * 0.3183098861837907f * dterm;
  }
  if (row.sheen()) {
    const float sv = m[FFX_MAT_SHEEN] * (1.0f - metallic) * schlick_weight(fabsf(co_h)) * cos_o;
    const float lum = TEX ? lum3(b0, b1, b2) : lum3(m[0], m[1], m[2]), sheen_tint = m[FFX_MAT_SHEEN_TINT];
    if (lum > 0.f) { a += bdiv(sv * sheen_tint, lum); b += sv * (1.0f - sheen_tint); if (TAU) tu += sv * sheen_tint; }
    else b += sv;
  }
  A = a * FFX_PI_F;
  B = b * FFX_PI_F;
  if (TAU) *tau = tu * FFX_PI_F;
}

// ---- the BSDF's adjoint (FFX_RENDER_GRAD_MATERIAL): d (uA A + uB B) / d (the row's eleven parameters FFX_MAT_ROUGHNESS ..
// FFX_MAT_CLEARCOAT_GLOSS), A and B as material_terms forms them, by one hand-derived reverse pass.  The geometry keeps the frame projections of
// the anisotropic form for every row: d/d anisotropic at 0 needs them although the isotropic forward never forms the frame.  One-sided derivatives
// into [0, 1] where the forward skips a lobe whose parameter is 0 (clearcoat, sheen, flatness, spec_tint, anisotropic; the diffuse and sheen lobes
// at metallic = 1, the diffuse lobe at spec_trans = 1); active fmaxf(0.001, .) clamps give 0.  The eta column is d/d eta, except at eta = 1
// where the forward skips the specular lobe and d/d eta vanishes: there it holds the limit of (d/d eta) / (eta - 1) as eta -> 1+, the factor
// that a `specular` leaf at 0 chains with the finite limit of (eta - 1) d eta / d specular (mi.py, scenes.specular_to_eta_grad).
#define FFX_MAT_GRAD_COLS FFX_RENDER_MATERIAL_COLS // columns FFX_MAT_ROUGHNESS .. FFX_MAT_CLEARCOAT_GLOSS (include/ffx.h FFX_RENDER_MATERIAL_FLOATS)
static_assert(FFX_MAT_CLEARCOAT_GLOSS - FFX_MAT_ROUGHNESS + 1 == FFX_MAT_GRAD_COLS, "the material block's columns are the row's parameters in order");
struct MatGeoD {
  float cos_i, cos_o, ch, ci_h, co_h, s2; // as MatGeo
  float hx, hy, vx, vy, lx, ly;           // the half vector, wv and wl in the shading frame coordinate_system(n)
};
__device__ __forceinline__ void material_geometry_d(v3 n, v3 wv, v3 wl, MatGeoD &g) {
  g.cos_i = vdot(n, wv);
  g.cos_o = vdot(n, wl);
  v3 wh = V3(wv.x + wl.x, wv.y + wl.y, wv.z + wl.z);
  const float ihl = __builtin_amdgcn_rsqf(vdot(wh, wh));
  wh = V3(wh.x * ihl, wh.y * ihl, wh.z * ihl);
  g.ci_h = vdot(wv, wh);
  g.co_h = vdot(wl, wh);
  g.ch = vdot(n, wh);
  const float sg = copysignf(1.0f, n.z), ca = -brcp(sg + n.z), cb = n.x * n.y * ca;
  const v3 fs = V3(sg * (sqrf(n.x) * ca) + 1.0f, sg * cb, -sg * n.x), ft = V3(cb, fmaf(n.y, n.y * ca, sg), -n.y);
  g.hx = vdot(wh, fs); g.hy = vdot(wh, ft);
  g.vx = vdot(wv, fs); g.vy = vdot(wv, ft);
  g.lx = vdot(wl, fs); g.ly = vdot(wl, ft);
  g.s2 = sqrf(g.hx) + sqrf(g.hy);
}
// lum: the luminance of the sample's base colour (the tint terms divide by it).  gr[j] += d (uA A + uB B) / d m[FFX_MAT_ROUGHNESS + j]
__device__ __forceinline__ void material_terms_vjp(const float *__restrict__ m, const MatGeoD &g, float lum, float uA, float uB, float (&gr)[FFX_MAT_GRAD_COLS]) {
  enum { R = 0, AN, ME, STR, ETA, STI, SH, SHT, FL, CC, CCG };
  const float cos_i = g.cos_i, cos_o = g.cos_o, ch = g.ch, ci_h = g.ci_h, co_h = g.co_h;
  if (!(cos_i > 0.f && cos_o > 0.f)) return;
  const bool facing = ci_h > 0.f && co_h > 0.f;
  const float wa = uA * FFX_PI_F, wb = uB * FFX_PI_F; // (A = pi a, B = pi b)
  const float eta = m[FFX_MAT_ETA];
  const float ct2 = 1.0f - (1.0f - ci_h * ci_h) * sqrf(brcp(eta));
  const float ct = ct2 > 0.f ? bsqrt(ct2) : 0.f;
  const float sw = schlick_weight(eta > 1.0f ? fabsf(ci_h) : ct);
  const float c = fabsf(ci_h);
  const float dct = ct2 > 0.f ? bdiv(1.0f - c * c, eta * eta * eta * ct) : 0.f; // d ct / d eta
  const float ds = c + eta * ct, dp = ct + eta * c, ir = brcp(ds * dp);
  const float a_s = (c - eta * ct) * dp * ir, a_p = (ct - eta * c) * ds * ir;
  float F_d = 0.5f * (a_s * a_s + a_p * a_p), dFd = a_s * (-2.0f * c * (ct + eta * dct) * sqrf(brcp(ds))) + a_p * (2.0f * c * (eta * dct - ct) * sqrf(brcp(dp)));
  if (eta == 1.0f) F_d = 0.f;
  else if (c == 0.f) { F_d = 1.f; dFd = 0.f; }
  const float metallic = m[FFX_MAT_METALLIC], m1 = 1.0f - metallic, spec_tint = m[FFX_MAT_SPEC_TINT];
  // roughness, anisotropic -> ax, ay (calc_dist_params; aspect = 1 and ax = ay = max(0.001, roughness^2) for an isotropic row)
  const float rough = m[FFX_MAT_ROUGHNESS], r2 = sqrf(rough), aspect = bsqrt(1.0f - 0.9f * m[FFX_MAT_ANISOTROPIC]);
  const float axr = bdiv(r2, aspect), ayr = r2 * aspect, ax = fmaxf(0.001f, axr), ay = fmaxf(0.001f, ayr);
  float d_sw = 0.f, d_eta = 0.f, d_ax = 0.f, d_ay = 0.f;
  if (facing && (F_d > 0.f || eta == 1.0f)) { // main specular lobe: F D G / (4 cos_i) = F P
    const float tmp = sqrf(bdiv(g.hx, ax)) + sqrf(bdiv(g.hy, ay)) + sqrf(ch);
    const float xy_i = sqrf(ax * g.vx) + sqrf(ay * g.vy), xy_o = sqrf(ax * g.lx) + sqrf(ay * g.ly), axay = ax * ay;
    const float dden = FFX_PI_F * axay * sqrf(tmp);
    const float s_i = bsqrt(sqrf(cos_i) + xy_i), s_o = bsqrt(sqrf(cos_o) + xy_o);
    float P = bdiv(cos_o, dden * ((cos_i + s_i) * (cos_o + s_o)));
    if (!(ch > 1e-20f * dden)) P = 0.f;
    const float ga = wa * P, gb = wb * P, gt = lum > 0.f ? bdiv(ga, lum) : gb; // (gt: the tint term t goes to a / lum, or to b when lum <= 0)
    if (eta == 1.0f) { // the lobe is skipped; (d F_d / d eta) / (eta - 1) -> a_s'^2 + a_p'^2 = (1 + (1 - 2c^2)^2) / (4 c^4), (d R0 / d eta) / (eta - 1) -> 1/2
      const float c2 = c * c;
      const float dF1 = c > 0.f ? bdiv(1.0f + sqrf(1.0f - 2.0f * c2), 4.0f * c2 * c2) : 0.f;
      d_eta = gb * m1 * (1.0f - spec_tint) * dF1 + gt * m1 * spec_tint * (1.0f - sw) * 0.5f;
    } else {
      const float R0 = sqrf((eta - 1.0f) * brcp(eta + 1.0f)), t = m1 * spec_tint * R0 * (1.0f - sw);
      const float Fa = metallic * (1.0f - sw) + (lum > 0.f ? bdiv(t, lum) : 0.f);
      const float Fb = metallic * sw + m1 * spec_tint * sw + m1 * (1.0f - spec_tint) * F_d + (lum > 0.f ? 0.f : t);
      gr[ME] += ga * (1.0f - sw) + gb * (sw - spec_tint * sw - (1.0f - spec_tint) * F_d) - gt * spec_tint * R0 * (1.0f - sw);
      gr[STI] += gb * m1 * (sw - F_d) + gt * m1 * R0 * (1.0f - sw);
      d_sw += -ga * metallic + gb * (metallic + m1 * spec_tint) - gt * m1 * spec_tint * R0;
      d_eta = gb * m1 * (1.0f - spec_tint) * dFd + gt * m1 * spec_tint * (1.0f - sw) * (4.0f * (eta - 1.0f) * brcp(sqrf(eta + 1.0f) * (eta + 1.0f)));
      // P = cos_o / (pi axay tmp^2 (cos_i + s_i)(cos_o + s_o)) -> axay, tmp, xy_i, xy_o -> ax, ay
      const float k = (wa * Fa + wb * Fb) * P;
      const float d_axay = -bdiv(k, axay), d_tmp = -2.0f * bdiv(k, tmp);
      const float d_xyi = -bdiv(k, 2.0f * s_i * (cos_i + s_i)), d_xyo = -bdiv(k, 2.0f * s_o * (cos_o + s_o));
      d_ax = d_axay * ay - 2.0f * d_tmp * bdiv(sqrf(g.hx), ax * ax * ax) + 2.0f * ax * (d_xyi * sqrf(g.vx) + d_xyo * sqrf(g.lx));
      d_ay = d_axay * ax - 2.0f * d_tmp * bdiv(sqrf(g.hy), ay * ay * ay) + 2.0f * ay * (d_xyi * sqrf(g.vy) + d_xyo * sqrf(g.ly));
    }
  }
  const float cc = m[FFX_MAT_CLEARCOAT];
  if (cc >= 0.f && facing) { // clearcoat: b += cc / 4 Fcc Dcc Gcc cos_o
    const float Fcc = sw + (1.0f - sw) * 0.04f;
    const float alpha = 0.1f + (0.001f - 0.1f) * m[FFX_MAT_CLEARCOAT_GLOSS], a2 = sqrf(alpha), c2 = sqrf(ch);
    const float L = logf(a2), Q = g.s2 + a2 * c2;
    float Dcc = bdiv(a2 - 1.0f, FFX_PI_F * L * Q);
    if (!(Dcc * ch > 1e-20f)) Dcc = 0.f;
    const float k = wb * 0.25f * ggx1_cc(cos_i, ci_h) * ggx1_cc(cos_o, co_h) * cos_o;
    gr[CC] += k * Fcc * Dcc;
    d_sw += k * cc * 0.96f * Dcc;
    const float dD = Dcc * (brcp(a2 - 1.0f) - brcp(a2 * L) - bdiv(c2, Q)); // d Dcc / d a2
    gr[CCG] += k * cc * Fcc * dD * 2.0f * alpha * (0.001f - 0.1f);
  }
  const float str = m[FFX_MAT_SPEC_TRANS];
  if (m1 >= 0.f && 1.0f - str >= 0.f) { // diffuse + retro-reflection (+ fake subsurface): a += (1 - metallic)(1 - spec_trans) cos_o / pi dterm
    const float Fo = schlick_weight(cos_o), Fi = schlick_weight(cos_i);
    const float f_diff = (1.0f - 0.5f * Fi) * (1.0f - 0.5f * Fo);
    const float Rr = 2.0f * rough * sqrf(co_h);
    const float d0 = f_diff + Rr * (Fo + Fi + Fo * Fi * (Rr - 1.0f));
    const float flat = m[FFX_MAT_FLATNESS];
    const float Fss90 = Rr * 0.5f;
    const float Fss = (1.0f + (Fss90 - 1.0f) * Fo) * (1.0f + (Fss90 - 1.0f) * Fi);
    const float iso = brcp(cos_o + cos_i) - 0.5f;
    const float f_ss = 1.25f * (Fss * iso + 0.5f);
    const float dterm = flat > 0.f ? d0 + (f_ss - d0) * flat : d0;
    const float dretro = Fo + Fi + Fo * Fi * (2.0f * Rr - 1.0f);
    const float dss = 1.25f * iso * 0.5f * (Fo * (1.0f + (Fss90 - 1.0f) * Fi) + Fi * (1.0f + (Fss90 - 1.0f) * Fo));
    const float k = wa * cos_o * 0.3183098861837907f, brdf = m1 * (1.0f - str);
    gr[ME] -= (1.0f - str) * k * dterm;
    gr[STR] -= m1 * k * dterm;
    if (flat >= 0.f) gr[FL] += k * brdf * (f_ss - d0);
    gr[R] += k * brdf * (flat > 0.f ? (1.0f - flat) * dretro + flat * dss : dretro) * 2.0f * sqrf(co_h);
  }
  const float sheen = m[FFX_MAT_SHEEN];
  if (sheen >= 0.f && m1 >= 0.f) { // sheen: sv = sheen (1 - metallic) schlick(|co_h|) cos_o, to a (tint / lum) and b (1 - tint)
    const float sh = schlick_weight(fabsf(co_h)) * cos_o, stt = m[FFX_MAT_SHEEN_TINT];
    const float gsv = lum > 0.f ? wa * bdiv(stt, lum) + wb * (1.0f - stt) : wb;
    gr[SH] += gsv * m1 * sh;
    gr[ME] -= gsv * sheen * sh;
    if (lum > 0.f) gr[SHT] += sheen * m1 * sh * (bdiv(wa, lum) - wb);
  }
  // eta: through F_d and R0 (d_eta), and through sw when eta < 1 (sw = schlick(ct))
  if (eta < 1.0f && ct2 > 0.f && ct < 1.0f) d_eta += d_sw * (-5.0f * sqrf(sqrf(1.0f - ct))) * dct;
  gr[ETA] += d_eta;
  // ax = max(0.001, roughness^2 / aspect), ay = max(0.001, roughness^2 aspect), aspect = sqrt(1 - 0.9 anisotropic)
  const float dx = axr > 0.001f ? d_ax : 0.f, dy = ayr > 0.001f ? d_ay : 0.f;
  gr[R] += 2.0f * rough * (bdiv(dx, aspect) + dy * aspect);
  gr[AN] += 0.45f * r2 * (bdiv(dx, aspect * aspect * aspect) - bdiv(dy, aspect));
}

struct SampleTerms {
  int hit, shape, has_proj;
  int ubx, uby; // unclamped bilinear base texel (for the per-sample cache)
  int ix0, ix1, iy0, iy1;
  float wx0, wx1, wy0, wy1;
  float proj_fac;
  float spot[3];
  float proj_fac_b, spot_b[3]; // material rows: the part of the BSDF that does not scale with base_color
  float base[3];               // textured base colours only (MATM == 2 / the lane kernels): the sample's base colour
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the bilinear footprint of a projector sample at (u, v) in [0, 1]^2 of a tw x th texture: base texel, four clamped taps, their weights
__device__ __forceinline__ void sample_footprint(SampleTerms &st, float u, float v, int tw, int th) {
  float fx = fmaf(u, (float)tw, -0.5f), fy = fmaf(v, (float)th, -0.5f);
  float x0 = floorf(fx), y0 = floorf(fy);
  float ax = fx - x0, ay = fy - y0;
  int ix0 = (int)x0, iy0 = (int)y0;
  st.ubx = ix0; st.uby = iy0;
  st.ix0 = clampi(ix0, 0, tw - 1);
  st.ix1 = clampi(ix0 + 1, 0, tw - 1);
  st.iy0 = clampi(iy0, 0, th - 1);
  st.iy1 = clampi(iy0 + 1, 0, th - 1);
  st.wx0 = 1.0f - ax; st.wx1 = ax;
  st.wy0 = 1.0f - ay; st.wy1 = ay;
  st.has_proj = 1;
}
// pi f cos = base * bA + bB of a principled row from either source, directions -> cosines (MatGeo) -> lobes
template <bool TEX, class Row>
__device__ __forceinline__ void row_lobes(const Row &row, v3 n, v3 wv, v3 wi, const float (&base)[3], float &bA, float &bB) {
  MatGeo g;
  material_geometry(row, n, wv, wi, g);
  material_terms<TEX>(row, g, bA, bB, base[0], base[1], base[2]);
}
// the packet kernels' BSDF of one emitter at pos for the sample at P (normal n, viewer wv, base colour `base` with TEX): pi f cos = base * bA + bB,
// bA = cos for a Lambert row (!mat_on); the emitter's factor fac becomes fac * bA and fac_b receives fac * bB.  The row source is chosen here, once:
// prow, the row's pre-row (wave-uniform: the rows travel with the call and the host derived their constants), or null — the raw row mrow
template <bool TEX, bool PLAIN>
__device__ __forceinline__ void emitter_terms(const float *mrow, const float *prow, bool mat_on, v3 P, v3 n, v3 wv, const float (&base)[3], const float *pos, float &fac,
                                              float &fac_b) {
  v3 wi = vsub(V3(pos[0], pos[1], pos[2]), P);
  const float idist = __builtin_amdgcn_rsqf(vdot(wi, wi));
  wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
  float bA = vdot(n, wi), bB = 0.f;
  if (mat_on) {
    if (PLAIN || prow) row_lobes<TEX>(RowPre<PLAIN>{mrow, prow}, n, wv, wi, base, bA, bB);
    else row_lobes<TEX>(RowRaw{mrow}, n, wv, wi, base, bA, bB);
  }
  fac_b = fac * bB;
  fac = fac * bA;
}
// is `shape`'s row of the material table mt a principled one (model != 0: it has a BSDF beyond base_color / pi)?
__device__ __forceinline__ bool principled_row(const ShadeK &c, const float *mt, int shape) { return c.mat_stride == FFX_MAT_STRIDE && mt[(size_t)FFX_MAT_STRIDE * shape + FFX_MAT_MODEL] != 0.f; }
// the BSDF of a shape's raw row for the lane kernels: pi f cos = base * A + B (and pi tau in T, TAU) at normal n, viewer wv, emitter wl; the base
// colour is `base` where the row is textured.  false: a Lambert row — A, B, T and *cos_o are left as they are
template <bool TAU>
__device__ __forceinline__ bool row_terms(const ShadeK &c, const float *mt, int shape, bool textured, const float (&base)[3], v3 n, v3 wv, v3 wl, float &A, float &B,
                                          float &T, float *cos_o = nullptr) {
  if (!principled_row(c, mt, shape)) return false;
  const RowRaw row{mt + (size_t)FFX_MAT_STRIDE * shape};
  MatGeo mg;
  material_geometry(row, n, wv, wl, mg);
  if (textured) material_terms<true, TAU>(row, mg, A, B, base[0], base[1], base[2], &T);
  else material_terms<false, TAU>(row, mg, A, B, 0.f, 0.f, 0.f, &T);
  if (cos_o) *cos_o = mg.cos_o;
  return true;
}

// ---- the projector texture at a sample and its adjoint: the pieces the render kernels and their adjoints below are built from ----
// a sample's four bilinear taps: the float offsets of texels (x0, y0), (x1, y0), (x0, y1), (x1, y1) in a tw-wide, tc-channel texture, and their weights
struct Taps { size_t o00, o01, o10, o11; float wx0, wx1, wy0, wy1; };
__device__ __forceinline__ Taps make_taps(int x0, int x1, int y0, int y1, float wx0, float wx1, float wy0, float wy1, int tw, int tc) {
  return {((size_t)y0 * tw + x0) * tc, ((size_t)y0 * tw + x1) * tc, ((size_t)y1 * tw + x0) * tc, ((size_t)y1 * tw + x1) * tc, wx0, wx1, wy0, wy1};
}
__device__ __forceinline__ Taps sample_taps(const SampleTerms &st, int tw, int tc) { return make_taps(st.ix0, st.ix1, st.iy0, st.iy1, st.wx0, st.wx1, st.wy0, st.wy1, tw, tc); }
// (v * wy) * wx to each of the four texels: emit(texel offset, ch, value)
template <class E>
__device__ __forceinline__ void taps_scatter(const Taps &t, int ch, float v, E &&emit) {
  emit(t.o00, ch, v * t.wy0 * t.wx0);
  emit(t.o01, ch, v * t.wy0 * t.wx1);
  emit(t.o10, ch, v * t.wy1 * t.wx0);
  emit(t.o11, ch, v * t.wy1 * t.wx1);
}
struct AtomicInto { // the usual emitter: a float atomic into the gradient
  float *g;
  __device__ __forceinline__ void operator()(size_t o, int ch, float v) const { atomicAdd(g + o + ch, v); }
};
// the projector's texture value at a sample, per colour channel: wy0 * (wx0 * t00 + wx1 * t01) + wy1 * (wx0 * t10 + wx1 * t11), times the projector's
// colour for one-channel textures (ONE_CH: the caller knows it is one)
// OFF32 (k_render_fwd_pk's plain-scene instance; the launch proved every buffer named in plain_scene below 2^32 bytes, texture sides below 2^24):
// a T at a 32-bit byte offset from a wave-uniform base — the load takes its scalar base and a 32-bit vector offset, no 64-bit address arithmetic
template <class T>
__device__ __forceinline__ const T &at32(const void *base, uint32_t byte_off) { return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off); }
template <bool ONE_CH = false, bool OFF32 = false>
__device__ __forceinline__ void proj_tex_value(const ShadeK &c, const SampleTerms &st, const float *__restrict__ tex, float (&tv)[3]) {
  static_assert(!OFF32 || ONE_CH, "32-bit texel offsets: the plain-scene instance's one-channel texture");
  if constexpr (OFF32) {
    const uint32_t r0 = __umul24((uint32_t)st.iy0, (uint32_t)c.tw), r1 = __umul24((uint32_t)st.iy1, (uint32_t)c.tw);
    const float t00 = at32<float>(tex, (r0 + (uint32_t)st.ix0) << 2), t01 = at32<float>(tex, (r0 + (uint32_t)st.ix1) << 2);
    const float t10 = at32<float>(tex, (r1 + (uint32_t)st.ix0) << 2), t11 = at32<float>(tex, (r1 + (uint32_t)st.ix1) << 2);
    const float v = st.wy0 * (st.wx0 * t00 + st.wx1 * t01) + st.wy1 * (st.wx0 * t10 + st.wx1 * t11);
    tv[0] = v * c.p_color[0]; tv[1] = v * c.p_color[1]; tv[2] = v * c.p_color[2];
    return;
  }
  const int tc = ONE_CH ? 1 : c.tc;
  const size_t o00 = ((size_t)st.iy0 * c.tw + st.ix0) * tc, o01 = ((size_t)st.iy0 * c.tw + st.ix1) * tc;
  const size_t o10 = ((size_t)st.iy1 * c.tw + st.ix0) * tc, o11 = ((size_t)st.iy1 * c.tw + st.ix1) * tc;
  const float v = st.wy0 * (st.wx0 * tex[o00] + st.wx1 * tex[o01]) + st.wy1 * (st.wx0 * tex[o10] + st.wx1 * tex[o11]);
  if (tc == 1) {
    tv[0] = v * c.p_color[0]; tv[1] = v * c.p_color[1]; tv[2] = v * c.p_color[2];
  } else {
    tv[0] = v;
#pragma unroll
    for (int ch = 1; ch < 3; ++ch) tv[ch] = st.wy0 * (st.wx0 * tex[o00 + ch] + st.wx1 * tex[o01 + ch]) + st.wy1 * (st.wx0 * tex[o10 + ch] + st.wx1 * tex[o11 + ch]);
  }
}
// a sample's colour from its terms: alb * (spot + tv * proj_fac) + (spot_b + tv * proj_fac_b), the second bracket only where rows exist (`rows`)
template <bool ONE_CH = false, bool OFF32 = false>
__device__ __forceinline__ void sample_colour(const ShadeK &c, const SampleTerms &st, const float *__restrict__ tex, const float *alb, bool rows, float (&L)[3]) {
  float r[3] = {st.spot[0], st.spot[1], st.spot[2]}, b[3] = {st.spot_b[0], st.spot_b[1], st.spot_b[2]};
  if (st.has_proj) {
    float tv[3];
    proj_tex_value<ONE_CH, OFF32>(c, st, tex, tv);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      r[ch] += tv[ch] * st.proj_fac;
      if (rows) b[ch] += tv[ch] * st.proj_fac_b;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    L[ch] = alb[ch] * r[ch];
    if (rows) L[ch] += b[ch];
  }
}
// what a one-channel texture's adjoint takes from a pixel's gradient g: sum over the channels of g * alb * colour, and of g * colour; left to right
__device__ __forceinline__ float g_alb_colour(const float (&g)[3], const float *alb, const float (&col)[3]) {
  return g[0] * alb[0] * col[0] + g[1] * alb[1] * col[1] + g[2] * alb[2] * col[2];
}
__device__ __forceinline__ float g_colour(const float (&g)[3], const float (&col)[3]) { return g[0] * col[0] + g[1] * col[1] + g[2] * col[2]; }
// the value a sample sends to its taps.  One channel: g_alb_colour * fac * inv_spp, plus g_colour * fac_b * inv_spp where fac_b != 0
__device__ __forceinline__ float tap_value_1ch(const float (&g)[3], const float *alb, const float (&col)[3], float fac, float fac_b, float inv_spp) {
  float ws = g_alb_colour(g, alb, col) * fac * inv_spp;
  if (fac_b != 0.f) ws += g_colour(g, col) * fac_b * inv_spp;
  return ws;
}
// ... three channels, per channel: g * alb * fac * inv_spp, plus g * fac_b * inv_spp where fac_b != 0
__device__ __forceinline__ float tap_value_3ch(float g, float alb, float fac, float fac_b, float inv_spp) {
  float ws = g * alb * fac * inv_spp;
  if (fac_b != 0.f) ws += g * fac_b * inv_spp;
  return ws;
}
// a sample's gradient into its four texels through `emit`: one value for a one-channel texture, one per channel for three; skip_zero: no emit of a zero value
template <class E>
__device__ __forceinline__ void sample_scatter(const Taps &t, int tc, const float (&g)[3], const float *alb, const float (&col)[3], float fac, float fac_b,
                                               float inv_spp, bool skip_zero, E &&emit) {
  if (tc == 1) {
    const float ws = tap_value_1ch(g, alb, col, fac, fac_b, inv_spp);
    if (!skip_zero || ws != 0.f) taps_scatter(t, 0, ws, emit);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float ws = tap_value_3ch(g[ch], alb[ch], fac, fac_b, inv_spp);
      if (!skip_zero || ws != 0.f) taps_scatter(t, ch, ws, emit);
    }
  }
}
// the value a footprint element (weights w, and wb of the rows' base-colour-free part) sends to its texel.  One channel, with the pixel's factors
// ws = g_alb_colour * inv_spp and wsb = g_colour * inv_spp: ws * w, plus wsb * wb where wb != 0
__device__ __forceinline__ float foot_value_1ch(float ws, float wsb, float w, float wb) {
  float val = ws * w;
  if (wb != 0.f) val += wsb * wb;
  return val;
}
// ... three channels, per channel: g * alb * inv_spp * w + g * inv_spp * wb
__device__ __forceinline__ float foot_value_3ch(float g, float alb, float inv_spp, float w, float wb) { return g * alb * inv_spp * w + g * inv_spp * wb; }

// what a path vertex needs beyond the emitters' terms: the lifted origin of its secondary ray, its normals, whether the row's base
// colour came from a texture.  ok = 0: no vertex (a miss, a degenerate triangle)
struct PathVtx { v3 Po, ng, ns; int textured, ok; };
struct PathVtxP : PathVtx { v3 P; }; // ... with the hit itself, for the walk that evaluates further emitters there (shade_sample's !EMIT: pv points to one)
// what the appearance adjoint needs beyond the emitters' terms: the tint parts pi tau of both emitters' factors (proj_t scales like
// proj_fac, spot_t like s_f), the spot's factors at unit intensity (spot = s_int s_f, spot_b = s_int s_fb), and where a textured base colour was read
struct AppTerms { float proj_t, spot_t, s_f, s_fb; int tix, slot; float bu, bv; };
// what the BSDF's adjoint needs (FFX_RENDER_GRAD_MATERIAL): the shading normal, both emitters' directions and the factors that multiply
// pi f cos into their terms (proj_fac = kp bA, spot's f = ks bA; 0: the emitter does not light the sample)
struct MatVtx { v3 ns, wp, ws; float kp, ks; };

// the sample's hit in (nt, ft] and next-event estimation there: projector and spot terms, shadow rays, base colour.  PATH (the path kernels):
// the ray has an arbitrary origin (no apex form) and *pv receives the vertex.  APP (k_render_bwd_appearance): *ap receives AppTerms.  MAT
// (k_render_bwd_material): *mv receives MatVtx.  !EMIT (k_lights_fwd): the hit and the vertex only — neither of the two main emitters is
// evaluated and none of their shadow rays is spent (the terms stay zero); pv->P receives the hit
template <bool PATH = false, bool APP = false, bool MAT = false, bool EMIT = true>
__device__ __forceinline__ void shade_sample(const ShadeK &c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const float4 *__restrict__ nrec, v3 o,
                                             v3 d, float nt, float ft, SampleTerms &st, int *stack, int stride, PathVtx *pv = nullptr, AppTerms *ap = nullptr,
                                             MatVtx *mv = nullptr) {
  Hit h;
  st.hit = traverse<false, !PATH>(nodes, recs, o, d, nt, ft, h, stack, stride);
  if (PATH) pv->ok = 0;
  if (APP) { ap->proj_t = ap->spot_t = ap->s_f = ap->s_fb = 0.f; ap->tix = 0; }
  if (MAT) { mv->kp = mv->ks = 0.f; }
  st.has_proj = 0;
  st.proj_fac = 0.f; st.proj_fac_b = 0.f;
  st.spot[0] = st.spot[1] = st.spot[2] = 0.f;
  st.spot_b[0] = st.spot_b[1] = st.spot_b[2] = 0.f;
  st.shape = h.shape;
  if (!st.hit) return;
  const float4 *r4 = reinterpret_cast<const float4 *>(recs + h.slot);
  float4 ra = r4[0], rb = r4[1], rc = r4[2];
  v3 P = V3(fmaf(h.t, d.x, o.x), fmaf(h.t, d.y, o.y), fmaf(h.t, d.z, o.z));
  v3 ng = vcross(V3(ra.w, rb.x, rb.y), V3(rb.z, rb.w, rc.x));
  float nl = sqrtf(vdot(ng, ng));
  if (!(nl > 0.f)) return;
  const float inl = 1.0f / nl;
  ng = V3(ng.x * inl, ng.y * inl, ng.z * inl);
  if (vdot(ng, d) > 0.f) ng = V3(-ng.x, -ng.y, -ng.z);
  float pmax = fmaxf(fabsf(P.x), fmaxf(fabsf(P.y), fabsf(P.z)));
  float off = (1.0f + pmax) * RAY_EPS;
  v3 Po = V3(fmaf(off, ng.x, P.x), fmaf(off, ng.y, P.y), fmaf(off, ng.z, P.z));
  // shading normal (ffx_smooth): BSDF and emitter cosines use it; the geometric normal keeps the side tests
  v3 ns = ng;
  if (rc.w != 0.f && nrec) ns = interpolated_normal<false>(nrec, h.slot, ra, rb, rc, o, d, ng);
  // base colour: the shape's row, or (FFX_MAT_BASE_TEX) its texture at the hit
  const float *mt = mat_table(c);
  const float *row0 = mt + (size_t)c.mat_stride * h.shape;
  st.base[0] = row0[0]; st.base[1] = row0[1]; st.base[2] = row0[2];
  bool textured = false;
  if (c.mat_stride == FFX_MAT_STRIDE && c.n_base_tex > 0) {
    const int tix = (int)row0[FFX_MAT_BASE_TEX];
    if (tix > 0 && tix <= c.n_base_tex) {
      float bu, bv;
      hit_barycentrics<false>(ra, rb, rc, o, d, bu, bv);
      base_tex_sample(c, tix - 1, h.slot, bu, bv, st.base);
      textured = true;
      if (APP) { ap->tix = tix; ap->slot = h.slot; ap->bu = bu; ap->bv = bv; }
    }
  }
  if (PATH) { pv->Po = Po; pv->ng = ng; pv->ns = ns; pv->textured = textured ? 1 : 0; pv->ok = 1; }
  if (PATH && !EMIT) static_cast<PathVtxP *>(pv)->P = P;
  if (MAT) mv->ns = ns;

  if (EMIT && c.proj_on) {
    v3 pl = xf_point(c.p_w2l, P);
    if (pl.z > 0.f) {
      const float *m = c.p_c2s;
      float qx = fmaf(m[0], pl.x, fmaf(m[1], pl.y, fmaf(m[2], pl.z, m[3])));
      float qy = fmaf(m[4], pl.x, fmaf(m[5], pl.y, fmaf(m[6], pl.z, m[7])));
      float qw = fmaf(m[12], pl.x, fmaf(m[13], pl.y, fmaf(m[14], pl.z, m[15])));
      const float iqw = 1.0f / qw;
      float u = qx * iqw, v = qy * iqw;
      if (u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f) {
        v3 ppos = V3(c.p_pos[0], c.p_pos[1], c.p_pos[2]);
        v3 wi = vsub(ppos, P);
        float d2 = vdot(wi, wi);
        const float idist = 1.0f / sqrtf(d2);
        wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
        float cos_s = vdot(ns, wi);
        float cos_p = -vdot(V3(c.p_axis[0], c.p_axis[1], c.p_axis[2]), wi);
        if (cos_s > 0.f && cos_p > 0.f && vdot(ng, wi) > 0.f) {
          bool vis = true;
          if (c.shadows) { // traced FROM the emitter (the batch's apex) to the lifted surface point: t in (0, 1 - eps)
            Hit hs;
            vis = !traverse<true, true>(nodes, recs, ppos, vsub(Po, ppos), 0.f, 1.0f - SHADOW_EPS, hs, stack, stride);
          }
          if (vis) {
            float bA = cos_s, bB = 0.f, bT = 0.f; // Lambert; material rows: pi f cos = base_color * bA + bB
            row_terms<APP>(c, mt, h.shape, textured, st.base, ns, V3(-d.x, -d.y, -d.z), wi, bA, bB, bT);
            st.proj_fac = (c.p_scale / (pl.z * pl.z * cos_p)) * bA;
            st.proj_fac_b = (c.p_scale / (pl.z * pl.z * cos_p)) * bB;
            if (APP) ap->proj_t = (c.p_scale / (pl.z * pl.z * cos_p)) * bT;
            if (MAT) { mv->kp = c.p_scale / (pl.z * pl.z * cos_p); mv->wp = wi; }
            sample_footprint(st, u, v, c.tw, c.th);
          }
        }
      }
    }
  }
  if (EMIT && c.spot_on) {
    v3 spos = V3(c.s_pos[0], c.s_pos[1], c.s_pos[2]);
    v3 wi = vsub(spos, P);
    float d2 = vdot(wi, wi);
    const float idist = 1.0f / sqrtf(d2);
    wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
    float cos_s = vdot(ns, wi);
    if (cos_s > 0.f && vdot(ng, wi) > 0.f) {
      v3 ll = xf_dir(c.s_w2l, V3(-wi.x, -wi.y, -wi.z));
      float ln = sqrtf(vdot(ll, ll));
      float cos_t = ll.z / ln;
      float fall = 0.f;
      if (cos_t >= c.cos_beam) fall = 1.f;
      else if (cos_t > c.cos_cut) fall = (c.cutoff - acosf(cos_t)) * c.inv_trans;
      if (fall > 0.f) {
        bool vis = true;
        if (c.shadows) {
          Hit hs;
          vis = !traverse<true, true>(nodes, recs, spos, vsub(Po, spos), 0.f, 1.0f - SHADOW_EPS, hs, stack, stride);
        }
        if (vis) {
          float bA = cos_s, bB = 0.f, bT = 0.f;
          row_terms<APP>(c, mt, h.shape, textured, st.base, ns, V3(-d.x, -d.y, -d.z), wi, bA, bB, bT);
          float f = fall * bA / d2 * 0.3183098861837907f, fb = fall * bB / d2 * 0.3183098861837907f;
          if (APP) { ap->s_f = f; ap->s_fb = fb; ap->spot_t = fall * bT / d2 * 0.3183098861837907f; }
          if (MAT) { mv->ks = fall / d2 * 0.3183098861837907f; mv->ws = wi; }
          st.spot[0] = c.s_int[0] * f;
          st.spot[1] = c.s_int[1] * f;
          st.spot[2] = c.s_int[2] * f;
          st.spot_b[0] = c.s_int[0] * fb;
          st.spot_b[1] = c.s_int[1] * fb;
          st.spot_b[2] = c.s_int[2] * fb;
        }
      }
    }
  }
}

// blockIdx -> tile.  Workgroups b, b+8, b+16, ... share an XCD (and its L2).  mode 1 gives each XCD a
// contiguous 1/8 band of the image (best L2 locality, but bands differ a lot in cost: the XCD that
// owns the vocal folds finishes last while others idle); mode 0 is the identity (XCDs interleave at
// tile granularity: balanced; the whole BVH fits every XCD's L2 anyway).  Pure performance.
// mode >= 2: blocked interleave with block size B = mode: within every group of 8*B workgroups, XCD k
// walks B CONSECUTIVE work items — the waves resident on one CU then work on adjacent pixels and share
// scalar-cache / L2 lines of the lower tree levels, while the groups stay small enough to balance.
__device__ __forceinline__ int xcd_remap(int b, int nblocks, int mode) {
  if (mode == 0) return b;
  if (mode == 1) {
    int per = (nblocks + 7) / 8;
    return (b % 8) * per + (b / 8);
  }
  const int B = mode, G = 8 * B;
  if ((B & (B - 1)) == 0) { // a power of two (the default, 128): shifts instead of two integer divisions per wave
    const int lb = 31 - __builtin_clz(B);
    const int g = b >> (lb + 3), r = b & (G - 1);
    if (((g + 1) << (lb + 3)) > nblocks) return b; // ragged last group: identity
    return (g << (lb + 3)) + ((r & 7) << lb) + (r >> 3);
  }
  const int g = b / G, r = b % G;
  if ((g + 1) * G > nblocks) return b; // ragged last group: identity
  return g * G + (r % 8) * B + (r / 8);
}

__global__ void __launch_bounds__(TR_BLOCK)
    k_render_fwd(ShadeK c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const float4 *__restrict__ nrec, const float *__restrict__ albedo,
                 const float *__restrict__ tex, int spp, uint32_t seed_key, int tiles_x, int n_tiles, int remap, int fp16, void *__restrict__ img) {
  extern __shared__ int s_dyn[];
  __shared__ float s_red[3][3][64]; // waves 1..3 -> wave 0
  int tile = xcd_remap(blockIdx.x, gridDim.x, remap);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int W = c.cam.W, H = c.cam.H;
  int px = (tile % tiles_x) * 8 + (lane & 7), py = (tile / tiles_x) * 8 + (lane >> 3);
  bool live = tile < n_tiles && px < W && py < H;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
  if (live) {
    const uint32_t pix = (uint32_t)py * (uint32_t)W + (uint32_t)px;
    for (int s = wave; s < spp; s += TR_BLOCK / 64) {
      uint32_t idx = pix * (uint32_t)spp + (uint32_t)s;
      float jx, jy;
      sample_jitter(seed_key, idx, jx, jy);
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      SampleTerms st;
      shade_sample(kernarg_shade(), nodes, recs, nrec, o, d, nt, ft, st, s_dyn + threadIdx.x, TR_BLOCK);
      if (!st.hit) continue;
      float L[3];
      sample_colour(c, st, tex, st.base, c.mat_stride != 3, L); // (st.base: the shape's row, or its base-colour texture at the hit)
      acc0 += L[0];
      acc1 += L[1];
      acc2 += L[2];
    }
  }
  if (wave > 0) {
    s_red[wave - 1][0][lane] = acc0;
    s_red[wave - 1][1][lane] = acc1;
    s_red[wave - 1][2][lane] = acc2;
  }
  __syncthreads();
  if (wave == 0 && live) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      acc0 += s_red[w][0][lane];
      acc1 += s_red[w][1][lane];
      acc2 += s_red[w][2][lane];
    }
    float inv_spp = 1.0f / (float)spp;
    size_t o = ((size_t)py * W + px) * 3;
    if (fp16 & 1) {
      _Float16 *p = (_Float16 *)img;
      p[o] = (_Float16)(acc0 * inv_spp);
      p[o + 1] = (_Float16)(acc1 * inv_spp);
      p[o + 2] = (_Float16)(acc2 * inv_spp);
    } else {
      float *p = (float *)img;
      p[o] = acc0 * inv_spp;
      p[o + 1] = acc1 * inv_spp;
      p[o + 2] = acc2 * inv_spp;
    }
  }
}

// K9: replay the same samples, scatter d(loss)/d(img) * d(img)/d(tex) through the bilinear weights.
__global__ void __launch_bounds__(TR_BLOCK)
    k_render_bwd(ShadeK c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const float4 *__restrict__ nrec, const float *__restrict__ albedo, int spp,
                 uint32_t seed_key, int tiles_x, int n_tiles, int remap, const float *__restrict__ gimg, float *__restrict__ gtex) {
  extern __shared__ int s_dyn[];
  int tile = xcd_remap(blockIdx.x, gridDim.x, remap);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int W = c.cam.W, H = c.cam.H;
  int px = (tile % tiles_x) * 8 + (lane & 7), py = (tile / tiles_x) * 8 + (lane >> 3);
  if (!(tile < n_tiles && px < W && py < H)) return;
  const uint32_t pix = (uint32_t)py * (uint32_t)W + (uint32_t)px;
  const float g[3] = {gimg[(size_t)pix * 3], gimg[(size_t)pix * 3 + 1], gimg[(size_t)pix * 3 + 2]};
  if (g[0] == 0.f && g[1] == 0.f && g[2] == 0.f) return;
  const float inv_spp = 1.0f / (float)spp;
  const int tc = c.tc;
  for (int s = wave; s < spp; s += TR_BLOCK / 64) {
    uint32_t idx = pix * (uint32_t)spp + (uint32_t)s;
    float jx, jy;
    sample_jitter(seed_key, idx, jx, jy);
    v3 o, d;
    float nt, ft;
    cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
    SampleTerms st;
    shade_sample(kernarg_shade(), nodes, recs, nrec, o, d, nt, ft, st, s_dyn + threadIdx.x, TR_BLOCK);
    if (!st.hit || !st.has_proj) continue;
    sample_scatter(sample_taps(st, c.tw, tc), tc, g, st.base, c.p_color, st.proj_fac, st.proj_fac_b, inv_spp, false, AtomicInto{gtex});
  }
}


// wave ballot of a predicate: the compiler's builtin reads the lane mask directly, whereas HIP's
// __ballot(int) materialises 0/1 in a VGPR and compares it again (two VALU instructions per call)
__device__ __forceinline__ unsigned long long wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// popcount of a lane mask as a 32-bit SCALAR (the compiler widens a comparison of two popcountll
// results to 64 bits, which has no scalar compare and lands on the VALU)
__device__ __forceinline__ int wpop(unsigned long long m) { int r; asm("s_bcnt1_i32_b64 %0, %1" : "=s"(r) : "s"(m) : "scc"); return r; }
// ------------------------------------------------------------------------------------------ wave-packet traversal
// One wavefront = one packet of 64 coherent rays (4x4 pixels x 4 samples, or their shadow rays).
// Control flow is WAVE-UNIFORM: the packet walks the union of its rays' paths.  Because the node
// index is uniform, a node / triangle record is fetched ONCE per wave through the scalar cache
// (s_load) into SGPRs and feeds the per-lane slab / Moller-Trumbore arithmetic as scalar operands;
// the vector memory pipe is not used at all during traversal.  The traversal stack is a single
// VGPR addressed with v_writelane / v_readlane (entry i lives in lane i): no LDS, no barriers.
// Per-lane results are identical to the per-lane traversal (same tests, closest hit with the
// primitive-id tie-break is order independent).
// v_writelane_b32: vec[lane] = val (val, lane wave-uniform, in SGPRs).  clang exposes readlane but not
// writelane; the s_nop covers the "VALU wrote the SGPR used as lane select" hazard, which hipcc
// cannot see inside an asm statement.
__device__ __forceinline__ int writelane_i32(int val, int lane, int vec) {
  // gfx9 VALU ops may read ONE SGPR over the constant bus: the lane select travels in M0
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tv_writelane_b32 %0, %1, m0" : "+v"(vec) : "s"(val), "s"(lane) : "m0");
  return vec;
}
// the same, updating the stack register in place (no copy of the whole VGPR around the push)
__device__ __forceinline__ void push_lane(int &vec, int val, int lane) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tv_writelane_b32 %0, %1, m0" : "+v"(vec) : "s"(val), "s"(lane) : "m0");
}
// dst = mask ? v : dst, in place (keeps a loop-carried value in one register across the branch that updates it)
__device__ __forceinline__ void msel_into(float &dst, unsigned long long mask, float v) {
  asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(v), "s"(mask));
}
__device__ __forceinline__ void msel_into(int &dst, unsigned long long mask, int v) {
  asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(v), "s"(mask));
}

// A scalar seen as an array of one.  The generic packet walk, shade_sample_pk and the two tile kernels were written for R rays
// per lane and still run their single-trip loops over one-element arrays: the compiler turns such an array into registers only
// after it has unrolled the loop, late in its pipeline, and with the same statements written straight-line every render kernel
// that reaches them comes out different (other registers, spills moved both ways: tools/isa_same.py).  They keep that form
// behind one-ray signatures until a change to these kernels is measured anyway.  For the same reason the walks take their ray
// by const reference: by value the render kernels came out different too.
template <typename T> __device__ __forceinline__ const T (&as1(const T &x))[1] { return reinterpret_cast<const T (&)[1]>(x); }
template <typename T> __device__ __forceinline__ T (&as1(T &x))[1] { return reinterpret_cast<T (&)[1]>(x); }

// Generic packet walk (min/max slab test, no assumption on direction signs), one ray per lane — a packed
// two-rays-per-lane variant was measured slower and removed.  The kernels reach this loop for the rare
// packets whose rays disagree on a direction sign and for the packets the 64-wide walk hands back;
// everything else takes the octant loops below.  Same apex triangle test, same results.
// (The body's one-element arrays and single-trip loops: see as1.)
template <bool ANY>
__device__ __forceinline__ void traverse_packet(const BvhNode *__restrict__ nodes, const TriApex *__restrict__ recs, const v3 &o_, const v3 &d_, const float &tmin_,
                                                const float &tmax_, const bool &active_, Hit &h_, bool &found_) {
  const v3 (&o)[1] = as1(o_), (&d)[1] = as1(d_);
  const float (&tmin)[1] = as1(tmin_), (&tmax)[1] = as1(tmax_);
  const bool (&active)[1] = as1(active_);
  Hit (&h)[1] = as1(h_);
  bool (&found)[1] = as1(found_);
  RayBox rb[1];
#pragma unroll
  for (int r = 0; r < 1; ++r) {
    h[r].t = active[r] ? tmax[r] : -INFINITY; // an inactive ray fails every slab test
    h[r].prim = -1;
    h[r].shape = -1;
    h[r].slot = -1;
    found[r] = false;
    rb[r] = make_raybox(o[r], d[r]);
  }
  int stack_v = 0;
  int sp = 0;
  int cur = 0;
  while (true) {
    cur = __builtin_amdgcn_readfirstlane(cur);
    // ONE 64-byte scalar fetch per node (uniform address -> scalar loads), no conditional loads
    const float4 *n4 = reinterpret_cast<const float4 *>(nodes + cur);
    const float4 q0 = n4[0], q1 = n4[1], q2 = n4[2];
    const int4 ch = *reinterpret_cast<const int4 *>(n4 + 3);
    const int c0 = ch.x, c1 = ch.y;
    const float lo0[3] = {q0.x, q0.y, q0.z}, hi0[3] = {q0.w, q1.x, q1.y};
    const float lo1[3] = {q1.z, q1.w, q2.x}, hi1[3] = {q2.y, q2.z, q2.w};
    float t0[1], t1[1];
    bool h0[1], h1[1];
    bool any0 = false, any1 = false;
#pragma unroll
    for (int r = 0; r < 1; ++r) {
      h0[r] = slab(lo0, hi0, rb[r], tmin[r], h[r].t * FFX_TIE_WIDEN, t0[r]) & (c0 != FFX_EMPTY_CHILD);
      h1[r] = slab(lo1, hi1, rb[r], tmin[r], h[r].t * FFX_TIE_WIDEN, t1[r]) & (c1 != FFX_EMPTY_CHILD);
      any0 |= h0[r];
      any1 |= h1[r];
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int c = side ? c1 : c0;
      if (c < 0 && c != FFX_EMPTY_CHILD && wballot(side ? any1 : any0) != 0ull) { // wave-uniform
        const uint32_t lc = (uint32_t)~c;
        const int first = (int)(lc >> 3), count = (int)(lc & 7u) + 1;
        for (int i = 0; i < count; ++i) {
          const float4 *r4 = reinterpret_cast<const float4 *>(recs + first + i);
          const float4 ra = r4[0], rb4 = r4[1], rc = r4[2];
          const int prim = __float_as_int(rc.z), shape = __float_as_int(rc.w);
          // apex record: det = d.A, U = d.B, V = d.C, t = T/det (ffx_common.h)
          const v3 A = V3(ra.x, ra.y, ra.z), B = V3(ra.w, rb4.x, rb4.y), C = V3(rb4.z, rb4.w, rc.x);
          const float Tq = rc.y;
          // three stages with WAVE-UNIFORM early-outs (same arithmetic and acceptance rule as
          // tri_hit_apex): the rays of a packet nearly always fail together at the first barycentric
          // test, so the remaining dot product and the IEEE division are skipped for the whole wave.
          // (U <= det is implied by V >= 0 and U + V <= det.)
          bool p1[1], neg[1], any1 = false;
          float detA[1], Us[1];
#pragma unroll
          for (int r = 0; r < 1; ++r) {
            const float det = vdot(d[r], A);
            const float U = vdot(d[r], B);
            neg[r] = det < 0.f;
            detA[r] = neg[r] ? -det : det;
            Us[r] = neg[r] ? -U : U;
            p1[r] = (side ? h1[r] : h0[r]) & (detA[r] > 0.f) & (Us[r] >= 0.f) & (Us[r] <= detA[r]);
            any1 |= p1[r];
          }
          if (wballot(any1) == 0ull) continue;
          bool p2[1], any2 = false;
#pragma unroll
          for (int r = 0; r < 1; ++r) {
            const float Vv = vdot(d[r], C);
            const float Vs = neg[r] ? -Vv : Vv;
            p2[r] = p1[r] & (Vs >= 0.f) & (Us[r] + Vs <= detA[r]);
            any2 |= p2[r];
          }
          if (wballot(any2) == 0ull) continue;
#pragma unroll
          for (int r = 0; r < 1; ++r) {
            const float t = (neg[r] ? -Tq : Tq) / detA[r];
            const bool hit = p2[r] & (t > tmin[r]);
            if (ANY) {
              const bool occ = hit & (t < tmax[r]);
              found[r] = found[r] | occ;
              h[r].t = occ ? -INFINITY : h[r].t;
            } else {
              const bool better = hit & (t <= tmax[r]) & ((h[r].prim < 0) | (t < h[r].t) | ((t == h[r].t) & (prim < h[r].prim)));
              h[r].t = better ? t : h[r].t;
              h[r].prim = better ? prim : h[r].prim;
              h[r].shape = better ? shape : h[r].shape;
              h[r].slot = better ? first + i : h[r].slot;
            }
          }
        }
      }
    }
    if (ANY) {
      bool undecided = false;
#pragma unroll
      for (int r = 0; r < 1; ++r) undecided |= active[r] & !found[r];
      if (wballot(undecided) == 0ull) break; // every ray of the packet is decided
    }
    bool g0 = false, g1 = false, first1 = false, first0 = false;
#pragma unroll
    for (int r = 0; r < 1; ++r) {
      const float hw = h[r].t * FFX_TIE_WIDEN;
      const bool a0 = h0[r] & (c0 >= 0) & (t0[r] <= hw), a1 = h1[r] & (c1 >= 0) & (t1[r] <= hw);
      g0 |= a0;
      g1 |= a1;
      first1 |= a1 & (!a0 | (t1[r] < t0[r]));
      first0 |= a0 & (!a1 | (t0[r] <= t1[r]));
    }
    const unsigned long long m0 = wballot(g0), m1 = wballot(g1);
    if (m0 != 0ull && m1 != 0ull) {
      // visit first the child that most lanes enter first
      const bool swap = wpop(wballot(first1)) > wpop(wballot(first0));
      stack_v = writelane_i32(swap ? c0 : c1, sp, stack_v);
      ++sp;
      cur = swap ? c1 : c0;
    } else if (m0 != 0ull) {
      cur = c0;
    } else if (m1 != 0ull) {
      cur = c1;
    } else {
      if (sp == 0) break;
      --sp;
      cur = __builtin_amdgcn_readlane(stack_v, sp);
    }
  }
}

// ------------------------------------------------------------------------------------------ octant-specialised packet walk
// All rays of a one-pixel packet (and of its shadow packets) almost always share the signs of their
// direction components.  Then, per axis, which of the two box planes is entered first is known for the
// whole packet, and the slab test needs neither min/max nor a subtract:
//     t_near[a] = near_plane[a] * id[a] - oidN[a]        t_far[a] = far_plane[a] * id[a] - oidF[a]
// one v_fma_f32 per plane with the node plane as the SGPR operand: 12 VALU per box instead of 27
// (3 v_mov + 6 sub + 6 mul + 6 min/max + ...).  oid = o*id; the fma form loses the exact cancellation
// of (plane - o)*id, so its rounding error |oid|*2^-24 is covered by a per-axis pad e = |oid|*2^-22
// folded into the two constants oidN = oid + e (entry can only move earlier) and oidF = oid - e (exit
// only later): boxes are hit at least as often as in exact arithmetic, and the triangle test — which
// alone decides the result — is unchanged.  The loop is compiled once per octant (OCT bit a set =
// direction component a negative) and selected per walk by a wave-uniform switch; packets with mixed
// signs take the generic loop.
#ifndef FFX_PK1_WAVES
// resident waves per SIMD the 1-ray packet kernels are register-budgeted for.  8 -> 64 VGPRs / 78 SGPRs.  With
// the 64-wide walk the hot loops fit: what spills (9 dwords) are loop-invariant addresses and pixel indices,
// stored once per wave and reloaded in the per-pixel epilogue.  Measured through the bench loop (tools/k8sweep.sh):
// 5 / 6 / 7 / 8 waves: 1235 / 1325 / 1376 / 1404 renders/s — the walk waits on one vector load per step, more
// resident waves hide it.  (The binary walk preferred 7: its spills were inside the node loop.)
#define FFX_PK1_WAVES 8
#endif
// `scale` = 1/tmax of the ray: the octant box test works in units of the ray's own parameter range, so
// every distance it compares lies in [0, 1] (see slab_oct).  The scale multiplies 1/d once, hence enters
// plane*m and o*m alike: a purely relative change of the results, no new cancellation error.
struct RayOct { v3 id, oidN, oidF; };
__device__ __forceinline__ RayOct make_rayoct(v3 o, v3 d, float scale) {
  RayOct r;
  r.id = V3(safe_rcp_dir(d.x) * scale, safe_rcp_dir(d.y) * scale, safe_rcp_dir(d.z) * scale);
  const v3 oid = V3(o.x * r.id.x, o.y * r.id.y, o.z * r.id.z);
  const float k = 2.384185791015625e-07f; // 2^-22
  const v3 e = V3(fabsf(oid.x) * k, fabsf(oid.y) * k, fabsf(oid.z) * k);
  r.oidN = V3(oid.x + e.x, oid.y + e.y, oid.z + e.z);
  r.oidF = V3(oid.x - e.x, oid.y - e.y, oid.z - e.z);
  return r;
}
// Predicates are kept as explicit 64-bit lane masks: v_cmp writes them straight into an SGPR pair,
// they are combined on the scalar ALU, tested with s_cmp (no ballot) and consumed by v_cndmask through
// inverse_ballot.  (A `bool` that is not itself a compare costs v_cndmask + v_cmp_ne per ballot.)
typedef unsigned long long wmask;
// hides a uniform mask from common-subexpression elimination: the compiler otherwise evaluates one
// `g != 0` for two branches up front and keeps the outcome as s_cselect'ed lane masks (4 extra SALU)
__device__ __forceinline__ wmask launder_mask(wmask m) { asm("" : "+s"(m)); return m; }
typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ wmask m_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 4); }  // ordered <
__device__ __forceinline__ wmask m_le(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 5); }  // ordered <=
__device__ __forceinline__ wmask m_gt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 2); }  // ordered >
__device__ __forceinline__ wmask m_ge(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 3); }  // ordered >=
__device__ __forceinline__ wmask m_eq(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 1); }  // ordered ==
__device__ __forceinline__ wmask m_ult(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 36); }
template <typename T>
__device__ __forceinline__ T msel(wmask m, T a, T b) { return __builtin_amdgcn_inverse_ballot_w64(m) ? a : b; }
// min/max without the sNaN-quieting v_max(x,x) the compiler puts in front of fminf/fmaxf operands it
// cannot prove canonical (the loop-carried hit distance): inputs here are never NaN
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// max3 with the VOP3 clamp bit: the result is clamped to [0, 1] at no cost
__device__ __forceinline__ float vmax3_sat(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmin2(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// a * b with b wave-uniform, as ONE v_mul with a scalar operand (written out so that the vectoriser does not pair the
// multiplies of a pixel's channels into v_pk_mul_f32, whose VGPR copy of b it hoists out of every loop and spills)
__device__ __forceinline__ float vmul_s(float a, float b_uniform) { float r; asm("v_mul_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b_uniform)); return r; }
// b is wave-uniform (an SGPR): VOP2's first source may be scalar — no v_mov in front of the min
__device__ __forceinline__ float vmin2_s(float a, uint32_t b_bits) { float r; asm("v_min_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b_bits)); return r; }

// Box test of the octant loops: one v_fma_f32 per plane with the node plane as the SGPR operand.
// Per plane the ray carries a multiplier and a constant,
//     entered-first plane:  m = id[a],      c = oidN[a]
//     left-last plane:      m = id[a] * k,  c = oidF[a] * k      (k = 1 + 3*2^-23, the far-side widening)
// which of lo/hi is which is fixed by the octant at compile time.  (v_pk_fma_f32 with the node planes
// as an SGPR pair was measured: it occupies ~1.5 issue slots on gfx950 and needs three more VGPRs, and
// the kernel got 8% slower — profiles/r1_issue_mix.txt.)
struct RaySlab { v3 id, idk, cN, cF; };
__device__ __forceinline__ RaySlab make_rayslab(const RayOct &rb) {
  const float k = 1.0000004f;
  RaySlab r;
  r.id = rb.id;
  r.idk = V3(rb.id.x * k, rb.id.y * k, rb.id.z * k);
  r.cN = rb.oidN;
  r.cF = V3(rb.oidF.x * k, rb.oidF.y * k, rb.oidF.z * k);
  return r;
}
// Distances are in units of the ray's parameter range (RayOct::scale), so a box can only matter if it is
// entered within [0, 1): the lower bound max(tn, tmin) becomes the free `clamp` bit of v_max3_f32 (the
// near clip distance is tiny: boxes nearer than it cost a visit at most, the triangle test still
// enforces t > tmin), and the upper bound is the scaled hit distance `hts` <= 0.9990002 (so an entry
// distance clamped down to 1 still fails).  10 VALU per box.
template <int OCT>
__device__ __forceinline__ wmask slab_oct(const float lo[3], const float hi[3], const RaySlab &rs, float hts, float &tn_out) {
  const float nx = (OCT & 1) ? hi[0] : lo[0], fx = (OCT & 1) ? lo[0] : hi[0];
  const float ny = (OCT & 2) ? hi[1] : lo[1], fy = (OCT & 2) ? lo[1] : hi[1];
  const float nz = (OCT & 4) ? hi[2] : lo[2], fz = (OCT & 4) ? lo[2] : hi[2];
  const float tn = vmax3_sat(fmaf(nx, rs.id.x, -rs.cN.x), fmaf(ny, rs.id.y, -rs.cN.y), fmaf(nz, rs.id.z, -rs.cN.z));
  const float tf = vmin2(vmin3(fmaf(fx, rs.idk.x, -rs.cF.x), fmaf(fy, rs.idk.y, -rs.cF.y), fmaf(fz, rs.idk.z, -rs.cF.z)), hts);
  tn_out = tn;
  return m_le(tn, tf);
}

// The scalar ALU issues at the same rate as the VALU (one instruction per SIMD per 4 cycles), so the
// uniform bookkeeping is written to stay short: 32-bit byte offsets for node / record addressing, a
// fast path for nodes whose children are both inner nodes (no leaf or empty-child logic at all), and
// nested uniform branches instead of combined predicates.
#ifdef FFX_BINCHECK
// self-check build (-DFFX_BINCHECK): [0] binned primary walks whose result differs from the tree walk's (per wave), [1] first-record latch,
// [2..4] the first one (pixel, lane; primitives; slots); [8..11] projector shadow walks; [16..19] spot shadow walks
__device__ unsigned long long g_ffx_chk[24];
#endif
#ifdef FFX_STATS
// debug build only (-DFFX_STATS): per-launch totals of packet walks / node steps / triangle tests
__device__ unsigned long long g_ffx_stats[48]; // [32..47]: tile bins (closest-hit 32.., any-hit 40..: walks served, chunk steps, exact tests, second barycentric, fallbacks to the tree)
#define FFX_STAT(i) do { if (threadIdx.x % 64 == 0) atomicAdd(&g_ffx_stats[i], 1ull); } while (0)
#define FFX_STAT_MAX(i, v) do { if (threadIdx.x % 64 == 0) atomicMax(&g_ffx_stats[i], (unsigned long long)(v)); } while (0)
#else
#define FFX_STAT(i) do { } while (0)
#define FFX_STAT_MAX(i, v) do { } while (0)
#endif
#ifdef FFX_TIMERS // separate debug build (-DFFX_TIMERS): the counters above perturb the timing by two orders of magnitude
// phase timers (shader clock, s_memtime): FFX_TSTART(t); ... FFX_TSTOP(t, slot) adds the elapsed cycles of this wave to slot
// (accumulated per workgroup in LDS and flushed once at the end of the kernel: a global atomic per stamp
// would sit in front of every s_waitcnt vmcnt(0) of the walk and measure itself)
__device__ unsigned long long g_ffx_tim[32];
static __shared__ unsigned long long s_ffx_tim[32];
#define FFX_TSTART(t) unsigned long long t = __builtin_amdgcn_s_memtime()
#define FFX_TSTOP(t, i) do { const unsigned long long t_now_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x % 64 == 0) s_ffx_tim[i] += t_now_ - t; t = t_now_; } while (0)
#define FFX_TINIT() do { if (threadIdx.x < 32) s_ffx_tim[threadIdx.x] = 0ull; __builtin_amdgcn_wave_barrier(); } while (0)
#define FFX_TFLUSH() do { __builtin_amdgcn_wave_barrier(); if (threadIdx.x < 32 && s_ffx_tim[threadIdx.x] != 0ull) atomicAdd(&g_ffx_tim[threadIdx.x], s_ffx_tim[threadIdx.x]); } while (0)
#else
#define FFX_TSTART(t) do { } while (0)
#define FFX_TSTOP(t, i) do { } while (0)
#define FFX_TINIT() do { } while (0)
#define FFX_TFLUSH() do { } while (0)
#endif
template <bool ANY, int OCT>
__device__ __forceinline__ void traverse_packet_oct(const BvhNode *__restrict__ nodes, const TriApex *__restrict__ recs, const RayOct &rb, float scale, v3 d,
                                                    float tmin, float tmax, wmask active, Hit &h, bool &found) {
  h.t = msel(active, tmax, -INFINITY); // an inactive ray fails every slab test
  // the hit distance in box-test units, widened by 2 ulp (a box touching the current hit must still be
  // entered: an equal-t triangle with a smaller id may be inside); refreshed after every leaf
  const float sw = scale * 1.0000002f;
  float hts = h.t * sw;
  h.prim = -1;
  h.shape = -1;
  h.slot = -1;
  wmask occluded = 0; // ANY: rays that have found an occluder
  int stack_v = 0;
  int sp = 0;
  int cur = 0; // wave-uniform throughout: node fetches are scalar loads
  const char *nbase = reinterpret_cast<const char *>(nodes);
  const char *rbase = reinterpret_cast<const char *>(recs);
  const RaySlab rs = make_rayslab(rb);
  FFX_STAT(ANY ? 4 : 0);
  while (true) {
    FFX_STAT(ANY ? 5 : 1);
    // the whole 64-byte node with ONE scalar load (s_load_dwordx16); the empty asm makes all 16 dwords
    // live, otherwise the compiler fetches the 14 it needs with three loads (x8 + x4 + x2) — and scalar
    // loads share the issue port that co-limits this loop
    const v16i nd = *reinterpret_cast<const v16i *>(nbase + ((uint32_t)cur << 6));
    asm volatile("" ::"s"(nd));
    const int c0 = nd.sc, c1 = nd.sd;
    float t0, t1;
    const float lo0[3] = {__int_as_float(nd.s0), __int_as_float(nd.s1), __int_as_float(nd.s2)};
    const float hi0[3] = {__int_as_float(nd.s3), __int_as_float(nd.s4), __int_as_float(nd.s5)};
    const float lo1[3] = {__int_as_float(nd.s6), __int_as_float(nd.s7), __int_as_float(nd.s8)};
    const float hi1[3] = {__int_as_float(nd.s9), __int_as_float(nd.sa), __int_as_float(nd.sb)};
    wmask g0 = slab_oct<OCT>(lo0, hi0, rs, hts, t0);
    wmask g1 = slab_oct<OCT>(lo1, hi1, rs, hts, t1);
    if (__builtin_expect((c0 | c1) < 0, 0)) { // a leaf or an empty child on at least one side (2 of 27 steps)
      FFX_STAT(ANY ? 12 : 8);
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int c = side ? c1 : c0;
        if (c >= 0) continue;
        const wmask hs = side ? g1 : g0;
        if (side) g1 = 0ull; else g0 = 0ull; // never descended into
        if (c == FFX_EMPTY_CHILD) continue;
        if (hs == 0ull) continue;
        const uint32_t lc = (uint32_t)~c;
        const uint32_t first = lc >> 3, count = (lc & 7u) + 1u;
        uint32_t roff = first * 48u;
        for (uint32_t i = 0; i < count; ++i, roff += 48u) {
          FFX_STAT(ANY ? 6 : 2);
          // the 48-byte apex record with two scalar loads (x8 + x4) issued together, instead of four staged ones
          const v8i r8 = *reinterpret_cast<const v8i *>(rbase + roff);
          const v4i r4 = *reinterpret_cast<const v4i *>(rbase + roff + 32);
          asm volatile("" ::"s"(r8), "s"(r4));
          const int prim = r4.z; // (the shape id is read back through h.slot)
          // apex record: det = d.A, U = d.B, V = d.C, t = T/det; staged with wave-uniform early-outs
          // (same arithmetic and acceptance rule as tri_hit_apex)
          const v3 A = V3(__int_as_float(r8.s0), __int_as_float(r8.s1), __int_as_float(r8.s2));
          const v3 B = V3(__int_as_float(r8.s3), __int_as_float(r8.s4), __int_as_float(r8.s5));
          const v3 C = V3(__int_as_float(r8.s6), __int_as_float(r8.s7), __int_as_float(r4.x));
          const float det = vdot(d, A);
          const float U = vdot(d, B);
          const wmask neg = m_lt(det, 0.f);
          const float detA = fabsf(det);
          const float Us = msel(neg, -U, U);
          const wmask p1 = hs & m_gt(detA, 0.f) & m_ge(Us, 0.f) & m_le(Us, detA);
          if (p1 == 0ull) continue;
          FFX_STAT(ANY ? 7 : 3);
          const float Vv = vdot(d, C);
          const float Vs = msel(neg, -Vv, Vv);
          const wmask p2 = p1 & m_ge(Vs, 0.f) & m_le(Us + Vs, detA);
          if (p2 == 0ull) continue;
          const float T = __int_as_float(r4.y);
          const float t = msel(neg, -T, T) / detA;
          const wmask hit = p2 & m_gt(t, tmin);
          if (ANY) {
            const wmask occ = hit & m_lt(t, tmax);
            occluded |= occ;
            msel_into(h.t, occ, -INFINITY);
          } else {
            // h.t <= tmax always and h.prim == -1 (the largest unsigned) until the first hit, so
            // (t <= tmax) & (no hit yet | t < h.t | (t == h.t & prim < h.prim)) reduces to:
            const wmask better = hit & (m_lt(t, h.t) | (m_eq(t, h.t) & m_ult((uint32_t)prim, (uint32_t)h.prim)));
            msel_into(h.t, better, t);
            msel_into(h.prim, better, prim);
            msel_into(h.slot, better, (int)(first + i));
          }
        }
      }
      if (ANY && (active & ~occluded) == 0ull) break; // every ray of the packet is decided
      // the hit distance may have shrunk: re-test the (at most one) remaining inner child
      hts = h.t * sw;
      if (g0 != 0ull) g0 &= m_le(t0, hts);
      if (g1 != 0ull) g1 &= m_le(t1, hts);
    }
    if (g0 != 0ull) {
      if (g1 != 0ull) {
        // both: visit first the child that most lanes enter first, push the other
        FFX_STAT(ANY ? 13 : 9);
        const wmask lt = m_lt(t1, t0);
        const bool swap = wpop(g1 & (~g0 | lt)) > wpop(g0 & ~(g1 & lt));
        push_lane(stack_v, swap ? c0 : c1, sp);
        ++sp;
        cur = swap ? c1 : c0;
      } else {
        cur = c0;
      }
    } else if (launder_mask(g1) != 0ull) { // (laundered: tested here, not hoisted above the g0 branch as a lane mask)
      cur = c1;
    } else {
      if (sp == 0) break;
      FFX_STAT(ANY ? 14 : 10);
      --sp;
      cur = __builtin_amdgcn_readlane(stack_v, sp);
    }
  }
  found = __builtin_amdgcn_inverse_ballot_w64(occluded);
}

// ------------------------------------------------------------------------------------------ 64-wide packet walk
// tools/ubench/issue_rates.hip (profiles/r2_issue_rates.txt) measured what bounds the binary packet walk
// above: on gfx950 a VALU instruction with an SGPR source operand, and every min/max/compare/select,
// issues once per ~4.3 cycles per SIMD, while mul/add/fma on VGPR operands issue every ~2.3 — and the
// binary walk's box test is ten 4.3-cycle instructions PER BOX, each computing the same answer in 64 lanes
// (the rays of a one-pixel packet are practically one ray).  This walk turns the lanes around for the box
// tests: a node has up to 64 children and LANE j TESTS CHILD j against the packet as a whole,
//     enter >= max_a (near_plane_a - o_a) * N_a        leave <= min_a (far_plane_a - o_a) * F_a
// with N_a / F_a the smallest / largest |1/d_a| of the packet's rays (they share their origin o, so the
// interval test costs exactly what a single ray costs: six fma on VGPR operands + four 4.3-cycle ops for 64
// boxes).  Triangles sit in clusters of up to 64 consecutive leaf slots whose boxes are tested the same way;
// only the triangles that survive are tested exactly, with the lanes back on the rays (same apex test, same
// acceptance rule: results are identical to the binary walk, closest hit with the primitive-id tie-break
// is order independent).  Boxes are float32 (ffx_common.h: WideChild, 32 B per child: a node is one
// coalesced 2 KB load).  The traversal stack (reference, entry distance) is in LDS.
// `elems`: the wide nodes (64 children each) followed by the triangle boxes in leaf-slot order — ONE array of
// 32-byte elements, so that a reference (cluster << 31 | element << 6 | count - 1) addresses both kinds alike;
// `tq0` = element index of leaf slot 0.
struct WideScene { const WideChild *elems; const WideHdr *hdr; int32_t root; uint32_t tq0; };
#define FFX_WSTACK (63 * FFX_WIDE_MAX_DEPTH + 6)
// per-walk constants, uniform across the wave: tn_a = fma(q_near_a, mN_a, -kN_a), tf_a = fma(q_far_a, mF_a, -kF_a).
// Packets whose rays disagree on a direction sign go to the binary walk (`dis != 0` in traverse_wide).  A wide
// walk for them was tried — a mixed axis as a wedge with two entry bounds and no exit bound — and removed; dropping
// the axis instead is conservative too, but a packet with two mixed axes — a pixel next to the image centre — then
// walks every box in its depth range: one such wave took 7 ms.
struct WidePk { v3 mN, kN, mF, kF; };

// wave-wide min / max of the bit patterns of NON-NEGATIVE floats (they order like unsigned integers): four
// fused DPP steps inside each row of 16 lanes (quad swap, quad-pair swap, half-row mirror, row mirror: one
// VALU instruction each; the s_nop covers the "VALU wrote the VGPR a DPP op reads" hazard the compiler
// cannot see inside an asm statement), then row_bcast:15 / :31 carry the row results to lane 63 (see
// wave_reduce3_nn) — one readlane, no scalar min/max.
template <bool MAX>
__device__ __forceinline__ uint32_t wave_reduce_nn(uint32_t v) {
  // ONE asm block (the compiler pads every asm statement with its own hazard nop)
#define FFX_R1(OP, CTRL, MASK) "s_nop 1\n\t" OP " %0, %0, %0 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"
#define FFX_R1_ALL(OP) FFX_R1(OP, "quad_perm:[1,0,3,2]", "0xf") FFX_R1(OP, "quad_perm:[2,3,0,1]", "0xf") FFX_R1(OP, "row_half_mirror", "0xf") \
    FFX_R1(OP, "row_mirror", "0xf") FFX_R1(OP, "row_bcast:15", "0xa") FFX_R1(OP, "row_bcast:31", "0xc")
  if (MAX) asm(FFX_R1_ALL("v_max_u32_dpp") : "+v"(v));
  else asm(FFX_R1_ALL("v_min_u32_dpp") : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
#ifndef FFX_WIDE_FAT
#define FFX_WIDE_FAT 0.04f // see traverse_wide
#endif
// three reductions at once (make_widepk: the three axes).  The chains are interleaved, so that the two instructions
// between a DPP write and the next DPP read of the same register ARE the wait states the hazard asks for (no s_nop per
// step), and the rows are combined by row_bcast:15 / row_bcast:31 (rows 1, 3 take lane 15 of the row before; rows 2, 3
// take lane 31): the wave's result sits in lane 63 — one readlane and no scalar min/max per value.
// Checked against a shuffle reduction on random data by tools/ubench/reduce3_check.hip.
#define FFX_R3_STEP(OP, CTRL, MASK)                               \
  OP " %0, %0, %0 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t" \
  OP " %1, %1, %1 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t" \
  OP " %2, %2, %2 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"
#define FFX_R3_ALL(OP)                                                                                                                            \
  "s_nop 1\n\t" FFX_R3_STEP(OP, "quad_perm:[1,0,3,2]", "0xf") FFX_R3_STEP(OP, "quad_perm:[2,3,0,1]", "0xf") FFX_R3_STEP(OP, "row_half_mirror", "0xf") \
      FFX_R3_STEP(OP, "row_mirror", "0xf") FFX_R3_STEP(OP, "row_bcast:15", "0xa") FFX_R3_STEP(OP, "row_bcast:31", "0xc")
template <bool MAX>
__device__ __forceinline__ void wave_reduce3_nn(uint32_t (&v)[3]) {
  if (MAX) asm(FFX_R3_ALL("v_max_u32_dpp") : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
  else asm(FFX_R3_ALL("v_min_u32_dpp") : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] = (uint32_t)__builtin_amdgcn_readlane((int)v[a], 63);
}
__device__ __forceinline__ uint32_t mbcnt64(wmask m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
__device__ __forceinline__ int wff1(wmask m) { return __builtin_ctzll(m); }

// the packet constants of one walk.  `aid` = |scaled 1/d| of the lane's ray per axis, `oct0` the packet's octant
// (the direction signs its active rays share); `spread` > FFX_WIDE_FAT: a fat packet (see traverse_wide).
__device__ __forceinline__ WidePk make_widepk(const v3 &o, const v3 &aid, const wmask &active, uint32_t oct0, float &spread) {
  const float oo[3] = {o.x, o.y, o.z};
  float mN[3], kN[3], mF[3], kF[3];
  const float kw = 1.0000004f;
  WidePk pk;
  // smallest / largest |1/d_a| over the active rays, the three axes in interleaved chains
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint32_t v = __float_as_uint(a == 0 ? aid.x : (a == 1 ? aid.y : aid.z));
    lo[a] = msel(active, v, 0x7f800000u); // +inf  (aid is finite: safe_rcp_dir clamps tiny components)
    hi[a] = msel(active, v, 0u);
  }
  wave_reduce3_nn<false>(lo);
  wave_reduce3_nn<true>(hi);
  // Everything from here on is wave-uniform float arithmetic, which this machine can only do on the vector ALU at the
  // 4-cycle rate of scalar-operand instructions: it is written to be short.  Signs are applied to the bit patterns
  // (scalar ALU); the two paddings of each side are one fma (2^-20 >= 2^-22 + 2^-21 + the roundings they cover:
  // of o * m, of m * k and of the box test's own fma); the fat-packet measure
  //     max_a (1/mn_a - 1/mx_a) / max_a (1/mn_a) <= FAT   <=>   for all a:  M (mx_a - mn_a) <= FAT mn_a mx_a,  M = min_a mn_a
  // needs no reciprocal.
  const float PAD = 9.5367431640625e-07f; // 2^-20
  const float M = fminf(__uint_as_float(lo[0]), fminf(__uint_as_float(lo[1]), __uint_as_float(lo[2])));
  bool fat = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint32_t sgn = ((oct0 >> a) & 1u) << 31;
    const float mn = __uint_as_float(lo[a]), mx = __uint_as_float(hi[a]);
    fat |= M * (mx - mn) > FFX_WIDE_FAT * (mn * mx);
    const float sN = __uint_as_float(lo[a] ^ sgn), sFk = __uint_as_float(hi[a] ^ sgn) * kw;
    const float oidn = oo[a] * sN, oidf = oo[a] * sFk;
    mN[a] = sN;
    kN[a] = fmaf(fabsf(oidn), PAD, oidn);   // the entry can only move earlier
    mF[a] = sFk;
    kF[a] = fmaf(-fabsf(oidf), PAD, oidf);  // the exit only later (on top of the far-side widening kw)
  }
  pk.mN = V3(mN[0], mN[1], mN[2]); pk.kN = V3(kN[0], kN[1], kN[2]);
  pk.mF = V3(mF[0], mF[1], mF[2]); pk.kF = V3(kF[0], kF[1], kF[2]);
  spread = fat ? 1.0f : 0.0f;
  return pk;
}

// returns false if the walk was abandoned because it exceeded its budget of steps / exact tests (the caller
// then repeats it on the binary walk, whose per-ray box tests cope with incoherent packets)
#ifndef FFX_WIDE_MAX_WORK
#define FFX_WIDE_MAX_WORK 96 // steps + exact triangle tests of one walk (typical: 7 + 7; measured 24 / 48 / 64 / 96 / 192: 0.77 / 0.70 / 0.65 / 0.65 / 0.65 ms vocal fold, 4.2 / 3.5 / 3.4 / 3.3 / 3.3 ms colon)
#endif
template <bool ANY, int OCT>
__device__ __forceinline__ bool traverse_wide_oct(const WideScene &ws, const TriApex *__restrict__ recs, const WidePk &pk, const v3 &d, const float &tmin, const float &tmax,
                                                  const float &sw, const wmask &active, Hit &h, wmask &occluded, uint2 *__restrict__ stack) {
  const uint32_t lane16 = (threadIdx.x & 63u) << FFX_WIDE_ELEM_SHIFT; // byte offset of this lane's element within a node / cluster
  int budget = FFX_WIDE_MAX_WORK;
  h.t = msel(active, tmax, -INFINITY);
  h.prim = -1;
  h.shape = -1;
  h.slot = -1;
  occluded = 0ull;
  // the packet's hit distance in box-test units (the largest over its rays: a box matters while ANY ray can
  // still reach it), as the bit pattern of a non-negative float; refreshed whenever a ray's hit improves
  auto packet_hts = [&]() -> uint32_t {
    return wave_reduce_nn<true>(__float_as_uint(fmaxf(0.f, h.t * sw))); // -inf (inactive / occluded) drops out against 0
  };
  // before any hit every active ray's distance is its tmax, which the unit of the box test maps to 0.999 * (1 + a few
  // ulp) by construction (sw = 0.999 / tmax * 1.0000002): a constant just above that is a valid (conservative) packet
  // bound — and saves the wave-wide maximum at the start of every walk.  It stays below 1, the value the clamp gives
  // boxes beyond the rays' range.
  uint32_t hb = __float_as_uint(0.9991f);
  int sp = 0;
  int32_t cur = ws.root;
  const char *ebase = reinterpret_cast<const char *>(ws.elems);
  const char *rbase = reinterpret_cast<const char *>(recs);
  FFX_STAT(ANY ? 4 : 0);
#ifdef FFX_STATS
  unsigned n_steps = 0, n_tris = 0;
#endif
  FFX_TSTART(tw);
  // ONE loop with ONE exit: every way out of a step (walk complete, every ray decided, budget spent) is folded into the
  // wave-uniform flag `go`, and every way on (descend, pop) into `nxt`.  Written with returns / continues from inside the
  // nested loops, the compiler's control-flow structuriser turned the exits into state variables and a dispatch
  // chain of ~15 scalar instructions and half a dozen branches per step.
  bool go, completed = true;
  do {
    go = true;
    bool descend = false;
    int32_t nxt = 0;
    FFX_STAT(ANY ? 5 : 1);
#ifdef FFX_STATS
    ++n_steps;
    FFX_STAT_MAX(ANY ? 15 : 11, ((unsigned long long)n_steps << 32) | n_tris);
    if (n_steps == 13) FFX_STAT(ANY ? 28 : 24); // walks with more than 12 steps, and the steps beyond
    if (n_steps > 12) FFX_STAT(ANY ? 29 : 25);
#endif
    // ---- fetch: lane j reads child j of an inner node or box j of a cluster: one 16-byte load per lane, no
    // divergence (lanes beyond the count re-read the last element and are masked out of the result)
    const uint32_t cnt1 = (uint32_t)cur & 63u;
    const uint32_t eoff = ((uint32_t)cur & 0x7fffffc0u) >> (6 - FFX_WIDE_ELEM_SHIFT); // element index * element size
    // lane j reads element j whatever the count: the unused children of a wide node hold inverted boxes (never hit), a
    // cluster's run is followed by other triangles' boxes (masked below; the array is padded by 64 elements) — so the
    // scalar side of the step is three instructions: the lane's byte offset is ONE vector add on a loop-invariant base.
    const uint32_t voff = eoff + lane16;
    const float4 qa = *reinterpret_cast<const float4 *>(ebase + voff);
    const uint4 q = *reinterpret_cast<const uint4 *>(ebase + voff + 16); // hi.y, hi.z, ref, pad  (q.z = ref)
    const float lx = qa.x, ly = qa.y, lz = qa.z, hx = qa.w, hy = __uint_as_float(q.x), hz = __uint_as_float(q.y);
#define FFX_QREF q.z
    // which plane is entered first is known at compile time
    const float nx = (OCT & 1) ? hx : lx, fx = (OCT & 1) ? lx : hx;
    const float ny = (OCT & 2) ? hy : ly, fy = (OCT & 2) ? ly : hy;
    const float nz = (OCT & 4) ? hz : lz, fz = (OCT & 4) ? lz : hz;
    const float tn = vmax3_sat(fmaf(nx, pk.mN.x, -pk.kN.x), fmaf(ny, pk.mN.y, -pk.kN.y), fmaf(nz, pk.mN.z, -pk.kN.z));
    const float tf = vmin2_s(vmin3(fmaf(fx, pk.mF.x, -pk.kF.x), fmaf(fy, pk.mF.y, -pk.kF.y), fmaf(fz, pk.mF.z, -pk.kF.z)), hb);
    wmask hit = m_le(tn, tf);
    FFX_TSTOP(tw, ANY ? 8 : 0);
    if (cur < 0) {
      hit &= ~0ull >> (63u - cnt1); // only the cluster's own triangles
      // ---- cluster: the surviving triangles are tested exactly, lanes back on the rays
      FFX_STAT(ANY ? 12 : 8);
      const uint32_t slot0 = (eoff >> FFX_WIDE_ELEM_SHIFT) - ws.tq0;
      while (hit != 0ull) {
        const uint32_t j = (uint32_t)wff1(hit);
        asm("s_bitset0_b64 %0, %1" : "+s"(hit) : "s"(j)); // hit &= hit - 1 in one scalar instruction instead of three
        --budget;
        FFX_STAT(ANY ? 6 : 2);
#ifdef FFX_STATS
        ++n_tris;
        if (n_tris == 17) FFX_STAT(ANY ? 20 : 16);  // walks with more than 16 exact tests ...
        if (n_tris > 16) FFX_STAT(ANY ? 21 : 17);   // ... and the tests beyond the 16th
        if (n_tris == 65) FFX_STAT(ANY ? 22 : 18);
        if (n_tris > 64) FFX_STAT(ANY ? 23 : 19);
#endif
        const uint32_t slot = slot0 + j;
        const uint32_t roff = slot * 48u;
        const v8i r8 = *reinterpret_cast<const v8i *>(rbase + roff);
        const v4i r4 = *reinterpret_cast<const v4i *>(rbase + roff + 32);
        asm volatile("" ::"s"(r8), "s"(r4));
        const int prim = r4.z;
        const v3 A = V3(__int_as_float(r8.s0), __int_as_float(r8.s1), __int_as_float(r8.s2));
        const v3 B = V3(__int_as_float(r8.s3), __int_as_float(r8.s4), __int_as_float(r8.s5));
        const v3 C = V3(__int_as_float(r8.s6), __int_as_float(r8.s7), __int_as_float(r4.x));
        const float T = __int_as_float(r4.y);
        // apex test, staged with wave-uniform early-outs (identical arithmetic to traverse_packet_oct)
        const float det = vdot(d, A);
        const float U = vdot(d, B);
        const wmask neg = m_lt(det, 0.f);
        const float detA = fabsf(det);
        const float Us = msel(neg, -U, U);
        const wmask alive = ANY ? (active & ~occluded) : active;
        const wmask p1 = alive & m_gt(detA, 0.f) & m_ge(Us, 0.f) & m_le(Us, detA);
        if (p1 == 0ull) continue;
        FFX_STAT(ANY ? 7 : 3);
        const float Vv = vdot(d, C);
        const float Vs = msel(neg, -Vv, Vv);
        const wmask p2 = p1 & m_ge(Vs, 0.f) & m_le(Us + Vs, detA);
        if (p2 == 0ull) continue;
        const float t = msel(neg, -T, T) / detA;
        const wmask hitm = p2 & m_gt(t, tmin);
        if (ANY) {
          const wmask occ = hitm & m_lt(t, tmax);
          occluded |= occ;
          msel_into(h.t, occ, -INFINITY);
          // every ray of the packet decided: leave the cluster, end the walk (else the undecided rays keep their full
          // length: the packet's hit distance does not change)
          if (occ != 0ull && (active & ~occluded) == 0ull) { go = false; hit = 0ull; }
        } else {
          const wmask better = hitm & (m_lt(t, h.t) | (m_eq(t, h.t) & m_ult((uint32_t)prim, (uint32_t)h.prim)));
          msel_into(h.t, better, t);
          msel_into(h.prim, better, prim);
          msel_into(h.slot, better, (int)slot);
          if (better != 0ull) {
            hb = packet_hts();
            hit &= m_le(tn, __uint_as_float(hb)); // the remaining triangles of this cluster against the shorter rays
          }
        }
      }
      FFX_TSTOP(tw, ANY ? 9 : 1);
    } else if (hit != 0ull) {
      FFX_STAT(ANY ? 13 : 9);
      // ---- inner node: descend into the child entered first, push the others with their entry distances.
      // key = entry distance (6 low mantissa bits dropped: it only orders and culls, conservatively) | lane
      const uint32_t key = (__float_as_uint(tn) & ~63u) | (threadIdx.x & 63u);
      uint32_t near_lane = (uint32_t)wff1(hit);
      if (wpop(hit) != 1) { // several children: nearest first, the others onto the stack
        near_lane = wave_reduce_nn<false>(msel(hit, key, 0xffffffffu)) & 63u;
        const wmask others = hit & ~(1ull << near_lane);
        if (__builtin_amdgcn_inverse_ballot_w64(others)) stack[sp + (int)mbcnt64(others)] = make_uint2(FFX_QREF, key);
        sp += wpop(others);
      }
      nxt = __builtin_amdgcn_readlane((int)FFX_QREF, (int)near_lane);
      descend = true;
      FFX_TSTOP(tw, ANY ? 10 : 2);
    }
    if (!descend && go) {
      // ---- pop: skip entries the rays can no longer reach; an empty stack ends the walk
      go = false;
      while (sp > 0) {
        FFX_STAT(ANY ? 14 : 10);
        --sp;
        const uint2 e = stack[sp];
        const uint32_t ref = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.x), etn = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y) & ~63u;
        if (etn <= hb) { nxt = (int32_t)ref; go = true; break; }
      }
      FFX_TSTOP(tw, ANY ? 11 : 3);
    }
    if (--budget < 0) { completed = false; go = false; } // (a walk that ends on its last allowed step is repeated by the caller: harmless)
    cur = nxt;
  } while (go);
  return completed;
}

#undef FFX_QREF
// wide walk of a packet whose rays share their origin `o` (the apex the records `recs` were prepared for).
// Packets the interval test is bad at go to the binary walk instead (its box tests are per ray): packets whose
// rays disagree on a direction sign, packets whose directions spread more than FFX_WIDE_FAT of their length
// (the samples of a pixel on a depth discontinuity, seen from an emitter: a fan whose bounding wedge
// contains hundreds of boxes no ray comes near — colon, 1024^2: 15.9 ms with every packet on the wide walk,
// 4.2 ms on the binary walk), and walks that exceed FFX_WIDE_MAX_WORK.  Results are identical either way.
template <bool ANY>
__device__ __forceinline__ void traverse_wide(const WideScene &ws, const BvhNode *__restrict__ nodes, const TriApex *__restrict__ recs, const v3 &o, const v3 &d,
                                              const float &tmin, const float &tmax, const bool &act, Hit &h, bool &found, uint2 *__restrict__ stack) {
  FFX_TSTART(ts);
  const wmask active = wballot(act);
  if (active == 0ull) {
    h.t = -INFINITY; h.prim = -1; h.shape = -1; h.slot = -1; found = false;
    return;
  }
  // unit of the box test: tmax maps to 0.999 (traverse_packet_any)
  const float scale = 0.999f * __builtin_amdgcn_rcpf(tmax);
  const v3 id = V3(safe_rcp_dir(d.x) * scale, safe_rcp_dir(d.y) * scale, safe_rcp_dir(d.z) * scale);
  const uint32_t oct = (__float_as_uint(id.x) >> 31) | ((__float_as_uint(id.y) >> 31) << 1) | ((__float_as_uint(id.z) >> 31) << 2);
  const v3 aid = V3(fabsf(id.x), fabsf(id.y), fabsf(id.z));
  const float sw = scale * 1.0000002f;
  // the packet's octant: that of its first active ray
  const uint32_t oct0 = (uint32_t)__builtin_amdgcn_readlane((int)oct, wff1(active));
  const wmask dis = active & __builtin_amdgcn_uicmp(oct, oct0, 33);
  bool done = false;
  if (dis == 0ull) {
    float spread;
    const WidePk pk = make_widepk(o, aid, active, oct0, spread);
    FFX_TSTOP(ts, ANY ? 12 : 4);
    if (spread <= FFX_WIDE_FAT) {
      wmask occ;
      switch (oct0) { // wave-uniform
        case 0: done = traverse_wide_oct<ANY, 0>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 1: done = traverse_wide_oct<ANY, 1>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 2: done = traverse_wide_oct<ANY, 2>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 3: done = traverse_wide_oct<ANY, 3>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 4: done = traverse_wide_oct<ANY, 4>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 5: done = traverse_wide_oct<ANY, 5>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        case 6: done = traverse_wide_oct<ANY, 6>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
        default: done = traverse_wide_oct<ANY, 7>(ws, recs, pk, d, tmin, tmax, sw, active, h, occ, stack); break;
      }
      found = __builtin_amdgcn_inverse_ballot_w64(occ);
    }
  }
  if (!done) {
    FFX_STAT(ANY ? 30 : 26);
    traverse_packet<ANY>(nodes, recs, o, d, tmin, tmax, act, h, found); // binary walk, per-ray box tests
  }
}

// dispatch: WIDE — the 64-wide walk (default); otherwise the binary walks: the octant loop if the packet's
// active rays agree on their direction signs, else the generic loop.  All packet walks are APEX walks (their
// rays share the origin `o` whose records `arecs` were written by k_apex_records).
template <bool ANY, bool WIDE>
__device__ __forceinline__ void traverse_packet_any(const BvhNode *__restrict__ nodes, const TriApex *__restrict__ arecs, const WideScene &ws, uint2 *__restrict__ stack,
                                                    const v3 &o, const v3 &d, const float &tmin, const float &tmax, const bool &active, Hit &h, bool &found) {
  if constexpr (WIDE) {
    traverse_wide<ANY>(ws, nodes, arecs, o, d, tmin, tmax, active, h, found, stack);
    return;
  }
  const wmask am = wballot(active);
  if (am == 0ull) { // nothing to trace
    h.t = -INFINITY; h.prim = -1; h.shape = -1; h.slot = -1; found = false;
    return;
  }
  // unit of the box test: tmax maps to 0.999, so an entry distance beyond the ray's range — which the
  // clamp turns into exactly 1 — stays above the scaled hit distance and the box is rejected
  const float scale = 0.999f * __builtin_amdgcn_rcpf(tmax);
  const RayOct rb = make_rayoct(o, d, scale);
  // octant from the reciprocals actually used (a clamped -0.0 component counts as negative)
  const uint32_t oct = (__float_as_uint(rb.id.x) >> 31) | ((__float_as_uint(rb.id.y) >> 31) << 1) | ((__float_as_uint(rb.id.z) >> 31) << 2);
  const uint32_t oct0 = (uint32_t)__builtin_amdgcn_readlane((int)oct, __builtin_ctzll(am)); // octant of the first active lane
  const bool uniform = (am & __builtin_amdgcn_uicmp(oct, oct0, 33)) == 0ull;
  if (uniform) {
    switch (oct0) { // wave-uniform
      case 0: traverse_packet_oct<ANY, 0>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 1: traverse_packet_oct<ANY, 1>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 2: traverse_packet_oct<ANY, 2>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 3: traverse_packet_oct<ANY, 3>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 4: traverse_packet_oct<ANY, 4>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 5: traverse_packet_oct<ANY, 5>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      case 6: traverse_packet_oct<ANY, 6>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
      default: traverse_packet_oct<ANY, 7>(nodes, arecs, rb, scale, d, tmin, tmax, am, h, found); break;
    }
  } else {
    traverse_packet<ANY>(nodes, arecs, o, d, tmin, tmax, active, h, found);
  }
}

// ------------------------------------------------------------------------------------------ tile bins instead of a tree walk
// (ffx_common.h BinEntry / BinGrid, ffx_bins.hip.)  The rays of a packet leave one apex and cover a rectangle of that apex's image
// plane: one pixel for the primary rays, the (tiny) bounding box of the samples' image points for a packet of shadow rays.  Every
// triangle such a ray can hit is listed in the tile(s) the rectangle touches.  A step loads 64 entries — one per lane, coalesced —
// and tests each against the rectangle: its padded box, then the rectangle's most-inside corner against the three edge functions,
//     max over the rectangle of (n.x x + n.y y + c) = n.x cx + |n.x| hx + n.y cy + |n.y| hy + c      (centre c*, half extents h*)
// four fma per edge with the rectangle as scalar operands, no selects.  The survivors — the triangles whose projection really
// overlaps the pixel, 1 - 3 of them — get the exact apex test of the tree walks (same arithmetic, same acceptance rule, closest hit
// with the primitive-id tie-break: the result does not depend on the order, and is the tree walk's bit for bit).
// No stack, no descent, no packet constants: where the 64-wide walk took 4.2 dependent steps and 100 VALU of set-up per pixel
// this is ~1.3 steps.  tx0..ty1: the tiles the rectangle touches (at most four: the caller falls back to the tree otherwise).
// BOX (bins_primary<..., RECT>): the caller hands the box bounds over — bx0..by1, the values rcx -+ rhx, rcy -+ rhy it read from the film's tables,
// already scalar — instead of having them formed and made uniform here.
// SL (the table-fed plain instances): a tile's two list bounds are read through the constant address space — the bins are the pre-pass's, no wave of
// a render writes them — so that their uniform address makes them scalar loads, not two vector loads and a wait for the vector memory counter.
#define FFX_CONST_AS __attribute__((address_space(4)))
template <bool ANY, bool OFF32 = false, bool BOX = false, bool SL = false>
__device__ __forceinline__ void traverse_bins(const char *__restrict__ bbase, const int nx, const int tx0, const int ty0, const int tx1, const int ty1, const float rcx,
                                              const float rcy, const float rhx, const float rhy, const TriApex *__restrict__ recs, const v3 d, const float tmin,
                                              const float tmax, const wmask active, Hit &h, wmask &occluded, const float bx0 = 0.f, const float bx1 = 0.f,
                                              const float by0 = 0.f, const float by1 = 0.f) {
  h.t = msel(active, tmax, -INFINITY);
  h.prim = -1;
  h.shape = -1;
  h.slot = -1;
  occluded = 0ull;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t *starts = reinterpret_cast<const uint32_t *>(bbase + 64); // ffx_bin_off_starts()
  const char *ents = bbase + ffx_bin_off_entries();
  const char *rbase = reinterpret_cast<const char *>(recs);
  // the rectangle's bounds for the box test — wave-uniform like centre and half extents: kept in SGPRs (they feed the step as scalar
  // operands; as VGPRs they would be eight more registers live across the exact tests)
  auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
  const float rx0 = BOX ? bx0 : uni(rcx - rhx), rx1 = BOX ? bx1 : uni(rcx + rhx), ry0 = BOX ? by0 : uni(rcy - rhy), ry1 = BOX ? by1 : uni(rcy + rhy);
  FFX_STAT(ANY ? 40 : 32);
  const float tmax_up = tmax * 1.0000038f; // tmax (1 + 2^-18)
  bool go = true;
  for (int ty = ty0; ty <= ty1 && go; ++ty) {
    for (int tx = tx0; tx <= tx1 && go; ++tx) {
      const uint32_t tile = (uint32_t)(ty * nx + tx);
      uint32_t beg, end;
      if constexpr (SL) {
        const FFX_CONST_AS uint32_t *sc = (const FFX_CONST_AS uint32_t *)(uintptr_t)starts;
        beg = sc[tile]; end = sc[tile + 1];
      } else {
        beg = starts[tile]; end = starts[tile + 1]; // (uniform address: scalar loads)
      }
      for (uint32_t b0 = beg; b0 < end && go; b0 += 64u) {
        FFX_STAT(ANY ? 41 : 33);
        const uint32_t idx = b0 + lane;
        const uint32_t idc = idx < end ? idx : end - 1u; // lanes beyond the list re-read its last entry and are masked out
        const float4 *e4 = OFF32 ? &at32<float4>(ents, idc << 6) : reinterpret_cast<const float4 *>(ents + ((size_t)idc << 6));
        const float4 A = e4[0], B = e4[1], C = e4[2], D = e4[3];
        wmask m = m_ult(idx, end) & m_le(A.x, rx1) & m_ge(A.z, rx0) & m_le(A.y, ry1) & m_ge(A.w, ry0);
        m &= m_ge(fmaf(B.x, rcx, fmaf(fabsf(B.x), rhx, fmaf(B.y, rcy, fmaf(fabsf(B.y), rhy, B.z)))), 0.f);
        m &= m_ge(fmaf(B.w, rcx, fmaf(fabsf(B.w), rhx, fmaf(C.x, rcy, fmaf(fabsf(C.x), rhy, C.y)))), 0.f);
        m &= m_ge(fmaf(C.z, rcx, fmaf(fabsf(C.z), rhx, fmaf(C.w, rcy, fmaf(fabsf(C.w), rhy, D.x)))), 0.f);
        const int slot_v = __float_as_int(D.y);
        while (m != 0ull) {
          const uint32_t j = (uint32_t)wff1(m);
          asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(j));
          FFX_STAT(ANY ? 42 : 34);
          const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane(slot_v, (int)j);
          const uint32_t roff = slot * 48u;
          const v8i r8 = *reinterpret_cast<const v8i *>(rbase + roff);
          const v4i r4 = *reinterpret_cast<const v4i *>(rbase + roff + 32);
          asm volatile("" ::"s"(r8), "s"(r4));
          const int prim = r4.z;
          // apex test, staged with wave-uniform early-outs (identical arithmetic to traverse_wide_oct / traverse_packet_oct)
          const v3 Av = V3(__int_as_float(r8.s0), __int_as_float(r8.s1), __int_as_float(r8.s2));
          const v3 Bv = V3(__int_as_float(r8.s3), __int_as_float(r8.s4), __int_as_float(r8.s5));
          const v3 Cv = V3(__int_as_float(r8.s6), __int_as_float(r8.s7), __int_as_float(r4.x));
          const float T = __int_as_float(r4.y);
          const float det = vdot(d, Av);
          const wmask neg = m_lt(det, 0.f);
          const float detA = fabsf(det);
          const wmask alive = ANY ? (active & ~occluded) : active;
          if (ANY) {
            // t = +-T / |det| must lie below tmax.  Most candidates of a shadow packet are the triangles of the surface the rays END on
            // (t = 1 up to rounding, beyond tmax = 1 - 10 eps): T and det alone settle them — |T| >= tmax (1 + 2^-18) |det| implies
            // fl(|T| / |det|) >= tmax — before either barycentric is formed (8 VALU instead of the 36 of a test that passes both)
            const float Ts = msel(neg, -T, T);
            if ((alive & m_lt(Ts, detA * tmax_up)) == 0ull) continue;
            FFX_STAT(46);
          }
          const float U = vdot(d, Bv);
          const float Us = msel(neg, -U, U);
          const wmask p1 = alive & m_gt(detA, 0.f) & m_ge(Us, 0.f) & m_le(Us, detA);
          if (p1 == 0ull) continue;
          FFX_STAT(ANY ? 43 : 35);
          const float Vv = vdot(d, Cv);
          const float Vs = msel(neg, -Vv, Vv);
          const wmask p2 = p1 & m_ge(Vs, 0.f) & m_le(Us + Vs, detA);
          if (p2 == 0ull) continue;
          const float t = msel(neg, -T, T) / detA;
          const wmask hitm = p2 & m_gt(t, tmin);
          if (ANY) {
            const wmask occ = hitm & m_lt(t, tmax);
            occluded |= occ;
            msel_into(h.t, occ, -INFINITY);
            if (occ != 0ull && (active & ~occluded) == 0ull) { go = false; m = 0ull; } // every ray of the packet is decided
          } else {
            const wmask better = hitm & (m_lt(t, h.t) | (m_eq(t, h.t) & m_ult((uint32_t)prim, (uint32_t)h.prim)));
            msel_into(h.t, better, t);
            msel_into(h.prim, better, prim);
            msel_into(h.slot, better, (int)slot);
          }
        }
      }
    }
  }
}

// the bins of apex `a` are usable for this launch and this pose?  (grid enabled by the host; lists complete: written by k_bin_scan)
// (SL: the header word through the constant address space, as traverse_bins<..., SL> reads the list bounds)
template <bool SL = false>
__device__ __forceinline__ bool bins_ready(const BinsK &bk, const int a) {
  if (!bk.g[a].on) return false;
  if constexpr (SL) return ((const FFX_CONST_AS BinHdr *)(uintptr_t)bk.base[a])->ok != 0u;
  else return reinterpret_cast<const BinHdr *>(bk.base[a])->ok != 0u; // (uniform address: a scalar load)
}

// primary rays of pixel (px, py): its own tile, its own square of the image plane.  The square is taken a half pad short at the far
// side: a sample position of exactly px + 1 (rounding of px + jitter) still lies within the entries' padding, and the pixels of a
// tile's last column do not drag the next tile's list in.
// RECT (the plain-scene instances; the launch made the film's tables, rect_tables): centre, box bounds and tile of the pixel's column and row are
// two 16-byte scalar loads from the tables (ffx_rect.h: the values the arithmetic below gives, bit for bit — they depend on the column or row, the
// film and the tile side alone), the half extents two kernel arguments; nothing is formed on the vector ALU and carried back.
typedef float v4f __attribute__((ext_vector_type(4)));
template <bool OFF32 = false, bool RECT = false, bool SL = false>
__device__ __forceinline__ bool bins_primary(const BinsK &bk, const int px, const int py, const TriApex *__restrict__ recs, const v3 d, const float tmin, const float tmax,
                                             const wmask active, Hit &h) {
  if (!bins_ready<SL>(bk, 0)) return false;
  if (active == 0ull) { h.t = -INFINITY; h.prim = -1; h.shape = -1; h.slot = -1; return true; } // nothing to trace
  if constexpr (RECT) {
    // (px < W, py < H: the kernel walks live pixels only.  Constant address space: written once, by the host, before the launch — a uniform index
    // is then a scalar load whatever the kernel itself stores elsewhere)
    typedef const __attribute__((address_space(4))) v4f *ctab;
    const RectK &rk = kernarg_rect();
    const ctab tab = (ctab)(uintptr_t)rk.tab;
    const v4f ex = tab[(uint32_t)px], ey = tab[rk.row0 + (uint32_t)py];
    const int stx = __float_as_int(ex.w), sty = __float_as_int(ey.w);
    if (stx >= bk.g[0].nx || sty >= bk.g[0].ny) return false;
    wmask occ;
    traverse_bins<false, OFF32, true, SL>(bk.base[0], bk.g[0].nx, stx, sty, stx, sty, ex.x, ey.x, rk.hx, rk.hy, recs, d, tmin, tmax, active, h, occ, ex.y, ex.z, ey.y, ey.z);
    return true;
  }
  const float its_x = bk.cam_inv_ts_x, its_y = bk.cam_inv_ts_y; // 1 / tile side: a power of two
  const float x0 = (float)px * its_x, y0 = (float)py * its_y;
  const int tx = (int)x0, ty = (int)y0;
  const float hx = 0.5f * its_x - 0.25f * FFX_BIN_PAD, hy = 0.5f * its_y - 0.25f * FFX_BIN_PAD;
  const float cx = x0 + hx, cy = y0 + hy;
  // (uniform values computed on the vector ALU: say so, so that they feed the step as scalar operands)
  const int stx = __builtin_amdgcn_readfirstlane(tx), sty = __builtin_amdgcn_readfirstlane(ty);
  const float scx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cx))), scy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cy)));
  const float shx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hx))), shy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hy)));
  if (stx >= bk.g[0].nx || sty >= bk.g[0].ny) return false;
  wmask occ;
  traverse_bins<false, OFF32, false, SL>(bk.base[0], bk.g[0].nx, stx, sty, stx, sty, scx, scy, shx, shy, recs, d, tmin, tmax, active, h, occ);
  return true;
}

// primary rays of a compact block of bw x bh pixels (K7's packets at fewer than 64 samples per pixel: 4x4 pixels at 1 spp ... one pixel):
// the block is aligned to its own size and at most 4 pixels wide, so it lies inside ONE tile of >= 4 pixels; its rectangle is the block
__device__ __forceinline__ bool bins_block(const BinsK &bk, const int bx0, const int by0, const int bw, const int bh, const TriApex *__restrict__ recs, const v3 d,
                                           const float tmin, const float tmax, const wmask active, Hit &h) {
  if (!bins_ready(bk, 0)) return false;
  if (active == 0ull) { h.t = -INFINITY; h.prim = -1; h.shape = -1; h.slot = -1; return true; }
  const float its_x = bk.cam_inv_ts_x, its_y = bk.cam_inv_ts_y; // 1 / tile side: a power of two
  if ((float)bw * its_x > 1.0f || (float)bh * its_y > 1.0f) return false; // (tiles smaller than the block: FFX_BIN_TILE experiments)
  const float x0 = (float)bx0 * its_x, y0 = (float)by0 * its_y;
  const int tx = (int)x0, ty = (int)y0;
  const float hx = 0.5f * (float)bw * its_x - 0.25f * FFX_BIN_PAD, hy = 0.5f * (float)bh * its_y - 0.25f * FFX_BIN_PAD;
  const float cx = x0 + hx, cy = y0 + hy;
  const int stx = __builtin_amdgcn_readfirstlane(tx), sty = __builtin_amdgcn_readfirstlane(ty);
  const float scx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cx))), scy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cy)));
  const float shx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hx))), shy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hy)));
  if (stx >= bk.g[0].nx || sty >= bk.g[0].ny) return false;
  wmask occ;
  traverse_bins<false>(bk.base[0], bk.g[0].nx, stx, sty, stx, sty, scx, scy, shx, shy, recs, d, tmin, tmax, active, h, occ);
  return true;
}

// four wave-wide reductions of non-negative floats at once — two minima, two maxima — in interleaved DPP chains (wave_reduce3_nn's
// scheme: the three instructions between a DPP write and the next read of the same register are the wait states the hazard needs)
__device__ __forceinline__ void wave_reduce_minmax4(uint32_t &mn0, uint32_t &mn1, uint32_t &mx0, uint32_t &mx1) {
#define FFX_R4_STEP(CTRL, MASK)                                                   \
  "v_min_u32_dpp %0, %0, %0 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"       \
  "v_min_u32_dpp %1, %1, %1 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"       \
  "v_max_u32_dpp %2, %2, %2 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"       \
  "v_max_u32_dpp %3, %3, %3 " CTRL " row_mask:" MASK " bank_mask:0xf\n\t"
  asm("s_nop 1\n\t" FFX_R4_STEP("quad_perm:[1,0,3,2]", "0xf") FFX_R4_STEP("quad_perm:[2,3,0,1]", "0xf") FFX_R4_STEP("row_half_mirror", "0xf")
          FFX_R4_STEP("row_mirror", "0xf") FFX_R4_STEP("row_bcast:15", "0xa") FFX_R4_STEP("row_bcast:31", "0xc")
      : "+v"(mn0), "+v"(mn1), "+v"(mx0), "+v"(mx1));
#undef FFX_R4_STEP
  mn0 = (uint32_t)__builtin_amdgcn_readlane((int)mn0, 63);
  mn1 = (uint32_t)__builtin_amdgcn_readlane((int)mn1, 63);
  mx0 = (uint32_t)__builtin_amdgcn_readlane((int)mx0, 63);
  mx1 = (uint32_t)__builtin_amdgcn_readlane((int)mx1, 63);
}

// shadow rays from emitter apex `a` (1 projector, 2 spot) to the lifted surface points: direction sdir = Po - E per lane.  Their image
// points on the emitter's grid are (M sdir).xy / (M sdir).z; the packet's rectangle is their bounding box (the samples of one pixel:
// a pixel's footprint as the emitter sees it).  A packet that leaves the grid or spreads over more than four tiles (the two sides of
// a depth discontinuity, far apart as seen from the emitter) takes the tree walk.
// GF (the table-fed plain instances): the grid's size as the floats the host converted once (RectK.gxf / gyf, read through kernarg_rect), not a conversion per call
template <bool OFF32 = false, bool GF = false, bool SL = false>
__device__ __forceinline__ bool bins_shadow(const BinsK &bk, const int a, const TriApex *__restrict__ recs, const v3 sdir, const wmask active, wmask &occluded) {
  if (!bins_ready<SL>(bk, a)) return false;
  const float *M = bk.g[a].M;
  const float Z = fmaf(M[6], sdir.x, fmaf(M[7], sdir.y, M[8] * sdir.z));
  const float iz = __builtin_amdgcn_rcpf(Z);
  const float fx = fmaf(M[0], sdir.x, fmaf(M[1], sdir.y, M[2] * sdir.z)) * iz, fy = fmaf(M[3], sdir.x, fmaf(M[4], sdir.y, M[5] * sdir.z)) * iz;
  float gx, gy;
  if constexpr (GF) { gx = kernarg_rect().gxf[a]; gy = kernarg_rect().gyf[a]; }
  else { gx = (float)bk.g[a].nx; gy = (float)bk.g[a].ny; }
  // inside the grid (NaN fails): everything else is the tree's business.  0 <= f < g as ONE unsigned comparison of the floats' bits: non-negative floats
  // order like their bits, negative ones (and NaN) have larger bits than any grid size (-0.0 counts as outside: the tree gives the same answer)
  const wmask inside = m_gt(Z, 0.f) & m_ult(__float_as_uint(fx), __float_as_uint(gx)) & m_ult(__float_as_uint(fy), __float_as_uint(gy));
  if ((active & ~inside) != 0ull) return false;
  // (round 6) the grid's ENVELOPE (ffx_common.h FFX_ENV_SUB, k_bin_env): the cell of each sample's image point holds a plane N . (X - E) = 1 in
  // front of every triangle the tile lists over that cell, pulled forward past the ignored tail of a shadow ray.  N . sdir <= 1: the segment
  // ends in front of it, no listed triangle can be hit within the counted part — and only listed triangles can be hit at all.  A packet all of
  // whose samples pass skips the stage (most do: the emitter stands next to the camera); NaN cells (no proof offered) fail the comparison.
  auto env_built = [&]() { // (SL: the header word as a scalar load, as bins_ready<SL> reads its neighbour)
    if constexpr (SL) return ((const FFX_CONST_AS BinHdr *)(uintptr_t)bk.base[a])->env != 0u;
    else return reinterpret_cast<const BinHdr *>(bk.base[a])->env != 0u;
  };
  if (((bk.env_on >> (a - 1)) & 1) && env_built()) { // (the header: THIS pose's pre-pass built it)
    const int nxf = bk.g[a].nx * FFX_ENV_SUB;
    const uint32_t last = (uint32_t)(nxf * bk.g[a].ny * FFX_ENV_SUB) - 1u;
    const uint32_t ci = (uint32_t)((int)(fy * (float)FFX_ENV_SUB) * nxf + (int)(fx * (float)FFX_ENV_SUB));
    const float4 Nc = OFF32 ? at32<float4>(bk.base[a] + bk.env_off, (ci < last ? ci : last) << 4) : reinterpret_cast<const float4 *>(bk.base[a] + bk.env_off)[ci < last ? ci : last]; // (lanes that are not active may hold anything)
    const float v = fmaf(Nc.x, sdir.x, fmaf(Nc.y, sdir.y, Nc.z * sdir.z));
    if ((active & ~m_le(v, 1.0f)) == 0ull) { occluded = 0ull; FFX_STAT(a == 1 ? 37 : 47); return true; }
  }
  uint32_t mnx = msel(active, __float_as_uint(fx), 0x7f800000u), mny = msel(active, __float_as_uint(fy), 0x7f800000u);
  uint32_t mxx = msel(active, __float_as_uint(fx), 0u), mxy = msel(active, __float_as_uint(fy), 0u);
  wave_reduce_minmax4(mnx, mny, mxx, mxy);
  const float x0 = __uint_as_float(mnx), y0 = __uint_as_float(mny), x1 = __uint_as_float(mxx), y1 = __uint_as_float(mxy);
  const int tx0 = (int)x0, ty0 = (int)y0, tx1 = (int)x1, ty1 = (int)y1; // (non-negative: truncation is floor)
  const int stx0 = __builtin_amdgcn_readfirstlane(tx0), sty0 = __builtin_amdgcn_readfirstlane(ty0);
  const int stx1 = __builtin_amdgcn_readfirstlane(tx1), sty1 = __builtin_amdgcn_readfirstlane(ty1);
  if ((stx1 - stx0 + 1) * (sty1 - sty0 + 1) > 4) return false;
  const float cx = 0.5f * (x0 + x1), cy = 0.5f * (y0 + y1), hx = 0.5f * (x1 - x0) + 1e-5f * gx, hy = 0.5f * (y1 - y0) + 1e-5f * gy; // (+ the rounding of the centre form)
  const float scx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cx))), scy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cy)));
  const float shx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hx))), shy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hy)));
  Hit hs;
  traverse_bins<true, OFF32, false, SL>(bk.base[a], bk.g[a].nx, stx0, sty0, stx1, sty1, scx, scy, shx, shy, recs, sdir, 0.f, 1.0f - SHADOW_EPS, active, hs, occluded);
  return true;
}

// per-sample shading state between the three packet walks
struct ShadePre {
  bool ok, need_p, need_s;
  v3 P, ng, Po;
  float pfac, u, v, sfac;
  float pfac_b, sfac_b; // material rows only
};

// packet version of shade_sample, one sample per lane: every lane of the wave reaches every walk
// The scene constants (ShadeK, ~100 dwords) are the first kernel argument of the render kernels.  Read
// through `c` the compiler loads them all up front and, out of SGPRs, parks them in VGPR lanes
// (v_writelane / v_readlane: ~480 spill instructions on the VALU, the unit that bounds these kernels).
// kernarg_shade() hands out the same constants through a pointer the compiler cannot see through, so
// each phase re-reads what it needs with scalar loads from the kernarg segment (no VALU work at all).

// whether any of the four texels of the bilinear footprint at (u, v) is non-zero (same texel arithmetic as the footprint phase)
// (OFF32: one channel, the four texels at 32-bit offsets — at32)
template <bool OFF32 = false>
__device__ __forceinline__ bool tex_footprint_lit(const float *__restrict__ tex, int tw, int th, int tc, float u, float v) {
  const float fx = fmaf(u, (float)tw, -0.5f), fy = fmaf(v, (float)th, -0.5f);
  const int ix0 = (int)floorf(fx), iy0 = (int)floorf(fy);
  const int x0 = clampi(ix0, 0, tw - 1), x1 = clampi(ix0 + 1, 0, tw - 1), y0 = clampi(iy0, 0, th - 1), y1 = clampi(iy0 + 1, 0, th - 1);
  float m = 0.f;
  if constexpr (OFF32) {
    const uint32_t r0 = __umul24((uint32_t)y0, (uint32_t)tw), r1 = __umul24((uint32_t)y1, (uint32_t)tw);
    m = fmaxf(m, fmaxf(fmaxf(fabsf(at32<float>(tex, (r0 + (uint32_t)x0) << 2)), fabsf(at32<float>(tex, (r0 + (uint32_t)x1) << 2))),
                       fmaxf(fabsf(at32<float>(tex, (r1 + (uint32_t)x0) << 2)), fabsf(at32<float>(tex, (r1 + (uint32_t)x1) << 2)))));
    return m > 0.f;
  }
  for (int ch = 0; ch < tc; ++ch)
    m = fmaxf(m, fmaxf(fmaxf(fabsf(tex[((size_t)y0 * tw + x0) * tc + ch]), fabsf(tex[((size_t)y0 * tw + x1) * tc + ch])),
                       fmaxf(fabsf(tex[((size_t)y1 * tw + x0) * tc + ch]), fabsf(tex[((size_t)y1 * tw + x1) * tc + ch]))));
  return m > 0.f; // (NaN texels: fmaxf drops them — as before, a NaN next to zeros reads as dark)
}

// MATM: 0 = [S,3] Lambert albedos, 1 = material rows, 2 = material rows some of which take their base colour from a texture
// px, py (wave-uniform): the pixel the packet's primary rays belong to — the tile bins are tried first, the tree walks serve
// what they cannot.  (The body's one-element arrays and single-trip loops: see as1.)
// PLAIN (k_render_fwd_pk<..., PLAIN>, MATM == 1): what the host proved about the scene before the launch (plain_scene) is a constant here — no record is
// flagged smooth, the spot's frame is rigid, the projector's texture has one channel, every row is a principled row with a pre-row and no optional
// lobe.  The tests and their arms are not compiled; the arithmetic that remains is the generic instance's, operation for operation.
// RECT (the plain forward and the plain forward + adjoint): the film's rectangle tables are at hand (rect_tables); the cache-writing plain forward keeps
// the per-pixel arithmetic and the parent's machine code (not measured with the tables; left for a change of its own).
template <bool WIDE, int MATM = 0, bool PLAIN = false, bool RECT = false>
__device__ __forceinline__ void shade_sample_pk(const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs,
                                                uint32_t astride, const WideScene &ws, uint2 *__restrict__ stack, const bool &active_, const v3 &o_,
                                                const v3 &d_, const float &nt_, const float &ft_, SampleTerms &st_,
                                                const float4 *__restrict__ nrec, const float4 *__restrict__ gn, const int px, const int py,
                                                const float *__restrict__ tex_probe = nullptr, const int blk_w = 1, const int blk_h = 1) {
  constexpr bool MAT = MATM != 0, TEX = MATM == 2;
  static_assert(!PLAIN || MATM == 1, "the plain-scene instance renders principled rows without textured base colours");
  const bool (&active)[1] = as1(active_);
  const v3 (&o)[1] = as1(o_), (&d)[1] = as1(d_);
  const float (&nt)[1] = as1(nt_), (&ft)[1] = as1(ft_);
  SampleTerms (&st)[1] = as1(st_);
  Hit h[1];
  bool fnd[1];
  FFX_TSTART(tp);
  bool binned = false;
  // (blk_w x blk_h > 1: the packet's primary rays belong to a compact block of pixels whose first is (px, py) — k_render_fwd_blk, renders at
  // fewer than 64 samples per pixel; the default arguments are constants of every other caller)
  if (blk_w * blk_h == 1) binned = bins_primary<PLAIN && FFX_K8_OFF32, RECT, RECT && FFX_K8_RECT_SL>(kernarg_shade().bins, px, py, arecs, d[0], nt[0], ft[0], wballot(active[0]), h[0]);
  else binned = bins_block(kernarg_shade().bins, px, py, blk_w, blk_h, arecs, d[0], nt[0], ft[0], wballot(active[0]), h[0]);
  if (!binned) {
    FFX_STAT(36);
    traverse_packet_any<false, WIDE>(nodes, arecs, ws, stack, o[0], d[0], nt[0], ft[0], active[0], h[0], fnd[0]); // apex 0: the camera
  }
#ifdef FFX_BINCHECK // self-check build: every binned walk is repeated on the tree and compared lane by lane (tools/bincheck.py)
  if (binned) {
    Hit h2[1];
    traverse_packet_any<false, WIDE>(nodes, arecs, ws, stack, o[0], d[0], nt[0], ft[0], active[0], h2[0], fnd[0]);
    const bool bad = active[0] && (h2[0].prim != h[0].prim || (h2[0].prim >= 0 && h2[0].t != h[0].t));
    const wmask bm = wballot(bad);
    if (bm != 0ull && (threadIdx.x & 63) == (unsigned)wff1(bm)) {
      atomicAdd(&g_ffx_chk[0], 1ull);
      if (atomicAdd(&g_ffx_chk[1], 1ull) == 0ull) { g_ffx_chk[2] = (unsigned long long)px | ((unsigned long long)py << 16) | ((unsigned long long)(threadIdx.x & 63) << 32); g_ffx_chk[3] = (unsigned long long)(uint32_t)h[0].prim | ((unsigned long long)(uint32_t)h2[0].prim << 32); g_ffx_chk[4] = (unsigned long long)(uint32_t)h[0].slot | ((unsigned long long)(uint32_t)h2[0].slot << 32); g_ffx_chk[5] = (unsigned long long)__float_as_uint(h[0].t) | ((unsigned long long)__float_as_uint(h2[0].t) << 32); }
    }
    h[0] = h2[0];
  }
#endif
  FFX_TSTOP(tp, 22);
  const ShadeK &c = kernarg_shade(); // phase: light terms at the hit point
  ShadePre pre[1];
  bool any_p = false, any_s = false;
#pragma unroll
  for (int r = 0; r < 1; ++r) {
    ShadePre &q = pre[r];
    // shading normal of this sample (ffx_smooth): equal to the geometric one unless the hit record is flagged.  It takes the
    // geometric normal's place in q.ng once the geometric side tests below are done (one normal stays live across the walks).
    v3 ns = V3(0.f, 0.f, 1.f);
    bool smooth = false;
    st[r].hit = h[r].prim >= 0;
    st[r].has_proj = 0;
    st[r].proj_fac = 0.f; st[r].proj_fac_b = 0.f;
    st[r].spot[0] = st[r].spot[1] = st[r].spot[2] = 0.f;
    st[r].spot_b[0] = st[r].spot_b[1] = st[r].spot_b[2] = 0.f;
    st[r].shape = -1; // read from the hit's triangle record below (the octant loops do not carry it)
    q.P = V3(0.f, 0.f, 0.f);
    q.ng = V3(0.f, 0.f, 1.f);
    q.Po = V3(0.f, 0.f, 0.f);
    q.ok = st[r].hit != 0;
    if (q.ok) {
      const float4 *r4 = reinterpret_cast<const float4 *>(recs + h[r].slot);
      // the unit geometric normal comes from the update (ffx_bvh_info.off_gn: IEEE, the oracle's bits) — re-deriving it from the
      // record cost 22 VALU per sample (cross, dot, sqrt, reciprocal, scale) — with the shape id and the smooth flag in its fourth
      // word: the record itself is only touched by samples that interpolate normals or look up a base-colour texture
      const float4 gq = (PLAIN && FFX_K8_OFF32) ? at32<float4>(gn, (uint32_t)h[r].slot << 4) : gn[h[r].slot];
      const int gbits = __float_as_int(gq.w); // 0: degenerate triangle; else (shape + 1) | smooth << 30
      st[r].shape = (gbits & FFX_GN_SHAPE_MASK) - 1;
      q.P = V3(fmaf(h[r].t, d[r].x, o[r].x), fmaf(h[r].t, d[r].y, o[r].y), fmaf(h[r].t, d[r].z, o[r].z));
      v3 ng = V3(gq.x, gq.y, gq.z);
      q.ok = (gbits & FFX_GN_SHAPE_MASK) != 0;
      if (!q.ok) st[r].shape = 0;
      if (q.ok) {
        if (vdot(ng, d[r]) > 0.f) ng = V3(-ng.x, -ng.y, -ng.z);
        q.ng = ng;
        float pmax = fmaxf(fabsf(q.P.x), fmaxf(fabsf(q.P.y), fabsf(q.P.z)));
        float off = (1.0f + pmax) * RAY_EPS;
        q.Po = V3(fmaf(off, ng.x, q.P.x), fmaf(off, ng.y, q.P.y), fmaf(off, ng.z, q.P.z));
        ns = ng;
        if constexpr (!PLAIN) smooth = (gbits & FFX_GN_SMOOTH_BIT) != 0;
        if (!PLAIN && wballot(smooth) != 0ull) { // (wave-uniform: scenes without flagged records never enter)
          const float4 ra = r4[0], rb = r4[1], rc = r4[2];
          const v3 ni = interpolated_normal<true>(nrec, smooth ? h[r].slot : 0, ra, rb, rc, o[r], d[r], ng);
          if (smooth) ns = ni;
        }
      }
    }
    const bool any_smooth = !PLAIN && wballot(smooth) != 0ull;
    // ---- projector terms
    q.need_p = false;
    q.pfac = 0.f; q.u = 0.f; q.v = 0.f;
    q.pfac_b = 0.f; q.sfac_b = 0.f;
    // material rows (MAT): pi f cos = base_color * bA + bB per emitter (material_eval); Lambert: bA = cos_s, bB = 0
    // (MAT: the BSDF is evaluated AFTER the shadow walks, for the samples the emitters reach — there the walk's registers
    // are free; before the walks only the geometric factors are formed, and P, ng stay live across them.  Parking P and ng
    // in LDS across the walks reaches 8 waves per SIMD instead of 7 but measured the same: the BSDF's own arithmetic, not
    // occupancy, is what the material rows cost — K8 0.57 ms against 0.48 ms for a diffuse scene)
    if (c.proj_on && q.ok) {
      v3 pl = xf_point(c.p_w2l, q.P);
      if (pl.z > 0.f) {
        const float *m = c.p_c2s;
        float qx = fmaf(m[0], pl.x, fmaf(m[1], pl.y, fmaf(m[2], pl.z, m[3])));
        float qy = fmaf(m[4], pl.x, fmaf(m[5], pl.y, fmaf(m[6], pl.z, m[7])));
        float qw = fmaf(m[12], pl.x, fmaf(m[13], pl.y, fmaf(m[14], pl.z, m[15])));
        const float iqw = rcp_nr(qw);
        q.u = qx * iqw;
        q.v = qy * iqw;
        if (q.u >= 0.f && q.u <= 1.f && q.v >= 0.f && q.v <= 1.f) {
          v3 ppos = V3(c.p_pos[0], c.p_pos[1], c.p_pos[2]);
          v3 wi = vsub(ppos, q.P);
          float d2 = vdot(wi, wi);
          const float idist = rsqrt_nr(d2);
          wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
          float cos_s = vdot(ns, wi);
          float cos_p = -vdot(V3(c.p_axis[0], c.p_axis[1], c.p_axis[2]), wi);
          bool lit = cos_s > 0.f && cos_p > 0.f;
          if (any_smooth) lit = lit && (!smooth || vdot(q.ng, wi) > 0.f); // the emitter on the viewer's GEOMETRIC side too
          if constexpr (MAT) {
            // (material rows: the texture probe — see below — comes first, it saves the BSDF of a dark footprint too)
            if (tex_probe && lit) lit = tex_footprint_lit<PLAIN && FFX_K8_OFF32>(tex_probe, c.tw, c.th, PLAIN ? 1 : c.tc, q.u, q.v);
          }
          if (lit) {
            q.need_p = true;
            if constexpr (MAT) {
              q.pfac = div_nr(c.p_scale, pl.z * pl.z * cos_p); // x (bA, bB) after the walks
            } else {
              q.pfac = div_nr(c.p_scale, pl.z * pl.z * cos_p) * cos_s;
            }
          }
        }
      }
    }
    // ---- spot terms
    q.need_s = false;
    q.sfac = 0.f;
    if (c.spot_on && q.ok) {
      v3 spos = V3(c.s_pos[0], c.s_pos[1], c.s_pos[2]);
      v3 wi = vsub(spos, q.P);
      float d2 = vdot(wi, wi);
      const float idist = rsqrt_nr(d2);
      wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
      float cos_s = vdot(ns, wi);
      bool front = cos_s > 0.f;
      if (any_smooth) front = front && (!smooth || vdot(q.ng, wi) > 0.f);
      if (front) {
        float cos_t;
        if (PLAIN || c.s_rigid) { // (the spot's world-to-local is a rotation — the usual case: |ll| = |wi| = 1, and ll.z is one row of it)
          cos_t = -fmaf(c.s_w2l[8], wi.x, fmaf(c.s_w2l[9], wi.y, c.s_w2l[10] * wi.z));
        } else {
          v3 ll = xf_dir(c.s_w2l, V3(-wi.x, -wi.y, -wi.z));
          float ln = sqrt_nr(vdot(ll, ll));
          cos_t = div_nr(ll.z, ln);
        }
        float fall = 0.f;
        if (cos_t >= c.cos_beam) fall = 1.f;
        else if (cos_t > c.cos_cut) fall = (c.cutoff - acosf(cos_t)) * c.inv_trans;
        if (fall > 0.f) {
          q.need_s = true;
          if constexpr (MAT) {
            q.sfac = div_nr(fall, d2) * 0.3183098861837907f; // x (bA, bB) after the walks
          } else {
            q.sfac = div_nr(fall * cos_s, d2) * 0.3183098861837907f;
          }
        }
      }
    }
    q.ng = ns; // from here on (BSDF after the walks) only the shading normal is needed
    // A plain forward render (no adjoint cache) does not need the projector's shadow ray where the projector shines
    // nothing: if the four texels of the sample's bilinear footprint are all exactly zero — most of a dot pattern is —
    // its contribution is zero whatever the walk finds.  (The cache-writing forward keeps every walk: the ADJOINT of a
    // dark texel is not zero.)  Same texel arithmetic as the footprint phase below.
    if constexpr (!MAT) {
      if (tex_probe && q.need_p) q.need_p = tex_footprint_lit(tex_probe, c.tw, c.th, c.tc, q.u, q.v);
    }
    any_p |= q.need_p;
    any_s |= q.need_s;
  }
  // ---- shadow walks (wave-uniform decisions).  A shadow ray is traced FROM the emitter — the apex its
  // triangle records were prepared for — to the lifted surface point: o = emitter, d = Po - emitter,
  // occluded iff some triangle is hit at 0 < t < 1 - eps.  No normalisation, and the packet's rays share
  // their origin exactly.
  bool occ_p[1], occ_s[1];
  occ_p[0] = occ_s[0] = false;
  FFX_TSTOP(tp, 18);
  const bool walk_p = c.shadows && wballot(any_p) != 0ull, walk_s = c.shadows && wballot(any_s) != 0ull;
  if (walk_p) {
    const v3 ppos = V3(c.p_pos[0], c.p_pos[1], c.p_pos[2]);
    v3 so[1], sdir[1];
    float s0[1], s1[1];
    bool act[1];
    Hit hs[1];
#pragma unroll
    for (int r = 0; r < 1; ++r) { so[r] = ppos; sdir[r] = vsub(pre[r].Po, ppos); s0[r] = 0.f; s1[r] = 1.0f - SHADOW_EPS; act[r] = pre[r].need_p; }
    const TriApex *arecs_p = reinterpret_cast<const TriApex *>(reinterpret_cast<const char *>(arecs) + astride);
    bool binned_p = false;
    wmask occm;
    binned_p = bins_shadow<PLAIN && FFX_K8_OFF32, RECT && FFX_K8_RECT_GF, RECT && FFX_K8_RECT_SL>(kernarg_shade().bins, 1, arecs_p, sdir[0], wballot(act[0]), occm);
    if (binned_p) occ_p[0] = __builtin_amdgcn_inverse_ballot_w64(occm);
    if (!binned_p) {
      FFX_STAT(44);
      traverse_packet_any<true, WIDE>(nodes, arecs_p, ws, stack, so[0], sdir[0], s0[0], s1[0], act[0], hs[0], occ_p[0]);
    }
#ifdef FFX_BINCHECK
    if (binned_p) {
      bool occ2[1];
      traverse_packet_any<true, WIDE>(nodes, arecs_p, ws, stack, so[0], sdir[0], s0[0], s1[0], act[0], hs[0], occ2[0]);
      const wmask bm = wballot(act[0] && occ2[0] != occ_p[0]);
      if (bm != 0ull && (threadIdx.x & 63) == (unsigned)wff1(bm)) {
        atomicAdd(&g_ffx_chk[8], 1ull);
        if (atomicAdd(&g_ffx_chk[9], 1ull) == 0ull) { g_ffx_chk[10] = (unsigned long long)px | ((unsigned long long)py << 16) | ((unsigned long long)(threadIdx.x & 63) << 32) | ((unsigned long long)occ2[0] << 40); g_ffx_chk[11] = (unsigned long long)(uint32_t)hs[0].slot; }
      }
      occ_p[0] = occ2[0];
    }
#endif
  }
  FFX_TSTOP(tp, 19);
  if (walk_s) {
    const v3 spos = V3(c.s_pos[0], c.s_pos[1], c.s_pos[2]);
    v3 so[1], sdir[1];
    float s0[1], s1[1];
    bool act[1];
    Hit hs[1];
#pragma unroll
    for (int r = 0; r < 1; ++r) { so[r] = spos; sdir[r] = vsub(pre[r].Po, spos); s0[r] = 0.f; s1[r] = 1.0f - SHADOW_EPS; act[r] = pre[r].need_s; }
    const TriApex *arecs_s = reinterpret_cast<const TriApex *>(reinterpret_cast<const char *>(arecs) + 2u * astride);
    bool binned_s = false;
    wmask occm;
    binned_s = bins_shadow<PLAIN && FFX_K8_OFF32, RECT && FFX_K8_RECT_GF, RECT && FFX_K8_RECT_SL>(kernarg_shade().bins, 2, arecs_s, sdir[0], wballot(act[0]), occm);
    if (binned_s) occ_s[0] = __builtin_amdgcn_inverse_ballot_w64(occm);
    if (!binned_s) {
      FFX_STAT(45);
      traverse_packet_any<true, WIDE>(nodes, arecs_s, ws, stack, so[0], sdir[0], s0[0], s1[0], act[0], hs[0], occ_s[0]);
    }
#ifdef FFX_BINCHECK
    if (binned_s) {
      bool occ2[1];
      traverse_packet_any<true, WIDE>(nodes, arecs_s, ws, stack, so[0], sdir[0], s0[0], s1[0], act[0], hs[0], occ2[0]);
      const wmask bm = wballot(act[0] && occ2[0] != occ_s[0]);
      if (bm != 0ull && (threadIdx.x & 63) == (unsigned)wff1(bm)) {
        atomicAdd(&g_ffx_chk[16], 1ull);
        if (atomicAdd(&g_ffx_chk[17], 1ull) == 0ull) { g_ffx_chk[18] = (unsigned long long)px | ((unsigned long long)py << 16) | ((unsigned long long)(threadIdx.x & 63) << 32) | ((unsigned long long)occ2[0] << 40); g_ffx_chk[19] = (unsigned long long)(uint32_t)hs[0].slot; }
      }
      occ_s[0] = occ2[0];
    }
#endif
  }
  FFX_TSTOP(tp, 20);
  const ShadeK &c2 = kernarg_shade(); // phase: texture footprint and light intensities
#pragma unroll
  for (int r = 0; r < 1; ++r) {
    ShadePre &q = pre[r];
    if constexpr (MAT) {
      // BSDF of the samples an emitter reaches: pi f cos = base_color * bA + bB (material_eval); Lambert rows: bA = cos_s
      const bool lit_p = q.need_p && !occ_p[r], lit_s = q.need_s && !occ_s[r];
      if constexpr (TEX) { st[r].base[0] = st[r].base[1] = st[r].base[2] = 0.f; }
      if (lit_p || lit_s) {
        const float *mrow = (PLAIN && FFX_K8_OFF32) ? &at32<float>(c2.mat_h, __umul24((uint32_t)st[r].shape, FFX_MAT_STRIDE * 4u)) : mat_table(c2) + (size_t)FFX_MAT_STRIDE * st[r].shape;
        const bool mat_on = PLAIN || mrow[FFX_MAT_MODEL] != 0.f;
        // (wave-uniform: the rows travel with the call and the host derived their constants — other tables take the on-the-fly form)
        const float *prow = (PLAIN && FFX_K8_OFF32) ? &at32<float>(c2.mat_pre, __umul24((uint32_t)st[r].shape, FFX_PRE_FLOATS * 4u))
                            : (PLAIN || c2.mat_pre_on) ? c2.mat_pre + FFX_PRE_FLOATS * st[r].shape : nullptr;
        const v3 wv = V3(-d[r].x, -d[r].y, -d[r].z);
        if constexpr (TEX) { // base colour of this sample: the row's, or its texture at the hit (only lit samples need one)
          st[r].base[0] = mrow[0]; st[r].base[1] = mrow[1]; st[r].base[2] = mrow[2];
          const int tix = (int)mrow[FFX_MAT_BASE_TEX];
          if (tix > 0 && tix <= c2.n_base_tex) {
            const float4 *r4 = reinterpret_cast<const float4 *>(recs + h[r].slot);
            float bu, bv;
            hit_barycentrics<true>(r4[0], r4[1], r4[2], o[r], d[r], bu, bv);
            base_tex_sample(c2, tix - 1, h[r].slot, bu, bv, st[r].base);
          }
        }
        // one emitter after the other: directions -> cosines (MatGeo) -> lobes
        if (lit_p) emitter_terms<TEX, PLAIN>(mrow, prow, mat_on, q.P, q.ng, wv, st[r].base, c2.p_pos, q.pfac, q.pfac_b);
        if (lit_s) emitter_terms<TEX, PLAIN>(mrow, prow, mat_on, q.P, q.ng, wv, st[r].base, c2.s_pos, q.sfac, q.sfac_b);
      }
    }
    if (q.need_p && !occ_p[r]) {
      st[r].proj_fac = q.pfac;
      if constexpr (MAT) st[r].proj_fac_b = q.pfac_b;
      sample_footprint(st[r], q.u, q.v, c2.tw, c2.th);
    }
    if (q.need_s && !occ_s[r]) {
      st[r].spot[0] = c2.s_int[0] * q.sfac;
      st[r].spot[1] = c2.s_int[1] * q.sfac;
      st[r].spot[2] = c2.s_int[2] * q.sfac;
      if constexpr (MAT) {
        st[r].spot_b[0] = c2.s_int[0] * q.sfac_b;
        st[r].spot_b[1] = c2.s_int[1] * q.sfac_b;
        st[r].spot_b[2] = c2.s_int[2] * q.sfac_b;
      }
    }
  }
  FFX_TSTOP(tp, 21);
}

// Packet kernels.  A wavefront owns one 2x2-pixel tile (65,536 work items at 512x512): tile costs vary
// by an order of magnitude (rays along the tube vs. rays that leave it), so fine-grained, independent
// waves let the hardware dispatcher keep every SIMD busy to the end.  The 64 lanes are the 64 samples
// of a pixel and the tile is walked as four single pixels: one ray per lane (two pixels per lane were measured slower and
// removed; the two tile kernels keep R = 1 in their template heads and their [R] arrays, see there).  All 64 rays of a packet are within a one-pixel frustum, so the
// union of their paths is practically one ray's path.
#define PK_BLOCK 64 // one independent wave per workgroup: the finest grain for the dispatcher (2 / 4 waves measured +1 % / +8 % time)

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// K7 on the packet traversal.  A wavefront owns a compact block of bw x bh pixels with spp_w samples
// each (bw * bh * spp_w = 64): 8x8 pixels at 1 spp ... one pixel at >= 64 spp (then it loops over the
// pixel's samples 64 at a time).  Sample index and jitter are those of k_trace_primary.
template <bool WIDE>
__global__ void __launch_bounds__(PK_BLOCK) __attribute__((amdgpu_waves_per_eu(FFX_PK1_WAVES, FFX_PK1_WAVES)))
    k_trace_primary_pk(CamK cam, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs, WideScene ws, int spp,
                       int jitter, uint32_t seed_key, int bw_log2,
                       int bh_log2, int blocks_x, int n_blocks, float *__restrict__ t_out, int32_t *__restrict__ shape_out, int32_t *__restrict__ prim_out, BinsK bins) {
  __shared__ uint2 s_wstack[WIDE ? FFX_WSTACK : 1];
  // (wave-uniform by construction; readfirstlane tells the compiler, which otherwise carries everything derived from it in VGPRs)
  const int blk = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (blk >= n_blocks) return; // whole wave
  const int lane = threadIdx.x & 63;
  const int ppw_log2 = bw_log2 + bh_log2; // pixels per wave (log2)
  const int spp_w = 64 >> ppw_log2;       // samples of one pixel handled per pass
  const int pl = lane >> (6 - ppw_log2);  // pixel of the block (0 when the wave is a single pixel)
  const int sl = lane & (spp_w - 1);      // sample slot within the pass
  const int x = ((blk % blocks_x) << bw_log2) + (pl & ((1 << bw_log2) - 1));
  const int y = ((blk / blocks_x) << bh_log2) + (pl >> bw_log2);
  const bool in_img = x < cam.W && y < cam.H;
  const uint32_t pix = (uint32_t)y * (uint32_t)cam.W + (uint32_t)x;
  const int passes = (spp + spp_w - 1) / spp_w;
  for (int pass = 0; pass < passes; ++pass) {
    const int sidx = pass * spp_w + sl;
    const bool active = in_img && sidx < spp;
    const uint32_t idx = pix * (uint32_t)spp + (uint32_t)sidx;
    float jx = 0.f, jy = 0.f;
    if (jitter) sample_jitter(seed_key, idx, jx, jy);
    v3 o, d;
    float nt, ft;
    cam_ray(cam, ((float)x + jx) * cam.inv_w, ((float)y + jy) * cam.inv_h, o, d, nt, ft);
    Hit h;
    bool fnd;
    // round 4: the block's candidates from the camera's tile bins (as K8's primary rays) — the tree walk when there are none
    // (no bins area, a grid that is off or overflowed)
    bool binned = false;
    if (bins.g[0].on)
      binned = bins_block(bins, (blk % blocks_x) << bw_log2, (blk / blocks_x) << bh_log2, 1 << bw_log2, 1 << bh_log2, arecs, d, nt, ft, wballot(active), h);
    if (!binned) traverse_packet_any<false, WIDE>(nodes, arecs, ws, s_wstack, o, d, nt, ft, active, h, fnd);
    if (active) {
      const bool hit = h.prim >= 0;
      t_out[idx] = hit ? (h.t - nt) : 0.f;
      if (shape_out) shape_out[idx] = hit ? recs[h.slot].shape : -1;
      if (prim_out) prim_out[idx] = h.prim;
    }
  }
}

// tile index -> pixel.  tiles_x carries the enumeration: bits 0..23 the number of 2x2-pixel tiles per
// image row, bits 24..27 tb: tiles are enumerated in square blocks of 2^tb x 2^tb tiles (row-major
// inside a block, blocks row-major over the image; tb = 0: plain row-major), so that consecutive work
// items — which the dispatcher hands to neighbouring wave slots — are compact 2-D patches of the image.
template <int R>
__device__ __forceinline__ void packet_pixels(int tile, int tiles_x_tb, int sub, int (&px)[R], int (&py)[R]) {
  const int tb = (tiles_x_tb >> 24) & 15, tiles_x = tiles_x_tb & 0xffffff;
  const int bt1 = (1 << tb) - 1, blocks_x = (tiles_x + bt1) >> tb;
  const int blk = tile >> (2 * tb), within = tile & ((1 << (2 * tb)) - 1);
  // row / column of the block: an UNSIGNED division through a float reciprocal with one correction step (exact for
  // the < 2^22 blocks of any film) — the compiler's signed integer division and modulo were ~50 scalar instructions
  // per wave, a tenth of a one-pixel wave's scalar work
  uint32_t by_ = (uint32_t)((float)blk * __builtin_amdgcn_rcpf((float)blocks_x));
  by_ = __builtin_amdgcn_readfirstlane((int)by_);
  int rem = blk - (int)by_ * blocks_x;
  if (rem < 0) { --by_; rem += blocks_x; }
  if (rem >= blocks_x) { ++by_; rem -= blocks_x; }
  const int tx = (rem << tb) + (within & bt1), ty = ((int)by_ << tb) + (within >> tb);
  const int bx = tx * 2, by = ty * 2;
#pragma unroll
  for (int r = 0; r < R; ++r) { px[r] = bx + (sub & 1); py[r] = by + (sub >> 1); }
}

// ---- adjoint cache (store instead of re-trace): what K9 needs of a pixel, written by K8.
// The render is linear in the texture and the 64 samples of a pixel land on a handful of neighbouring texels
// (measured: 87 % of the lit pixels within 4x4 texels, 99.5 % within 5x5), nearly always on ONE shape, so the
// adjoint of a pixel is  gtex[T] += (gimg[p] . albedo[shape] (. colour)) / spp * W[T]  with the per-pixel
// FOOTPRINT  W[T] = sum over its samples of fac * bilinear weight — 25 floats instead of 64 records of 16 B.
//   [0, 64)                        CacheHdr
//   64 + 8 * pixel                 CachePix: window origin, shape, lit flag — a DENSE array, so that the adjoint reads
//                                  2 MB of it instead of touching every pixel's footprint
//   off_foot + 112 * pixel         CacheFoot: the 5x5 footprint (written and read for lit pixels only)
//   off_arena + 24 * i             CacheStray: single samples that do not fit (outside the window: depth discontinuities,
//                                  grazing surfaces; a second shape in the pixel; later 64-sample passes of a pixel that
//                                  drift), allocated with one atomic per affected wave
// 37.7 MB at 512x512x64 (one 16-byte record per sample was 268 MB), of which K8 writes and K9 reads ~10 MB.
struct CacheHdr { uint32_t n_stray, cap_stray, dropped, pad[13]; };
struct __attribute__((aligned(8))) CachePix { int16_t x0, y0; uint16_t shape, lit; };
static_assert(sizeof(CachePix) == 8, "cache pixel header must be 8 bytes");
struct __attribute__((aligned(16))) CacheFoot { float w[25]; uint32_t pad[3]; };
static_assert(sizeof(CacheFoot) == 112, "cache footprint must be 112 bytes");
__host__ __device__ inline size_t cache_off_foot(size_t n_pix) { return (64 + 8 * n_pix + 127) & ~(size_t)127; }
__host__ __device__ inline size_t cache_off_arena(size_t n_pix) { return (cache_off_foot(n_pix) + sizeof(CacheFoot) * n_pix + 127) & ~(size_t)127; }
struct CacheStray { uint32_t pix, xy_shape; float ax, ay, fac; float fac_b; /* material rows only (else not written) */ }; // xy_shape = x0 | y0 << 12 ... see stray_pack
static_assert(sizeof(CacheStray) == 24, "stray record must be 24 bytes");
__host__ __device__ inline size_t cache_stray_capacity(int w, int h, int spp) {
  const size_t n = (size_t)w * h * spp / 64;
  return n < 4096 ? 4096 : n;
}
// material rows: a second footprint per pixel (the part of the BSDF that does not scale with base_color), behind the arena
__host__ __device__ inline size_t cache_off_foot_b(size_t n_pix, size_t cap_stray) {
  return (cache_off_arena(n_pix) + sizeof(CacheStray) * cap_stray + 127) & ~(size_t)127;
}

// ---- adjoint cache of a FILTERED render (ffx_render_fwd_cache_filtered, include/ffx.h).  A sample spreads over the 25 pixels of its
// window with weights of its own (the jitter), so a pixel's samples do not fold into one texture footprint as under the box film — its
// adjoint is a 25 x 25 matrix (window pixel x texel).  Kept instead: one 16-byte record PER SAMPLE of the pixels that have a lit sample
// {(ubx + 1) | (uby + 1) << 12 | shape << 24, ax, ay, fac} (+ fac_b in a second array with material rows) — one coalesced 1 KB store per
// wave and lit pass.  Round 6: the records live in an ARENA of 64-sample blocks (rounds 4-5: a dense [pixel][sample] array, 20 B x pixels x
// spp of address space — 5.4 GB at 1024 x 1024 x 256 — for the ~4 % of the pixels that hold a lit sample): the first lit pass of a pixel
// takes one block for itself and for every later pass with ONE atomic of its wave (on one of eight counters — sub-arenas —, neighbouring
// pixels on different ones; an arena with a block for every pass of every pixel hands each pixel its own, without atomics), the pixel's
// header holds the first block and that pass;
// capacity = rfc_cap_blocks; a pixel that finds the arena full is counted in `dropped` (sticky, as the
// box film's arena: ffx_render_cache_status, the NaN poison of the adjoint, ffx_adam_args.guard) and keeps no records.
//   [0, 64)                CacheHdr {-, capacity, dropped pixels, -, blocks taken from each of the eight sub-arenas (may exceed their share)}
//   64 + 8 * pixel         CachePix {x0 | y0 << 16 = first block, shape = first lit pass, lit = bit mask of the passes that hold records}
//   rfc_off_wsum           float per pixel
//   rfc_off_recs           uint4 per sample slot of the arena's blocks
//   rfc_off_facb           float per sample slot (material rows)
__host__ __device__ inline size_t rfc_cap_blocks(size_t n_pix, size_t spp, bool all = false) {
  // every pass of every pixel up to 2^18 blocks (335 MB with material rows: 512 x 512 x 64 spp keeps a block per pixel and cannot overflow,
  // whatever the texture), a QUARTER of them beyond: 1024 x 1024 x 256 — 1.05 M blocks, 1.34 GB instead of 5.4 GB.  (A tenth, 0.54 GB, was
  // tried first: BASELINE configs[4]'s own 1 024-point pattern lights 17 % of the film — 178 k pixels x 4 passes — and 73 k of them found no block.)
  // `all` (ffx_scene_desc.shadows & FFX_SHADOWS_CACHE_DENSE: the caller's answer to an overflow): a block for every pass of every pixel
  const size_t dense = n_pix * ((spp + 63) / 64), part = dense / 4, keep = (size_t)1 << 18;
  const size_t n = part > keep ? part : keep;
  return (all || n >= dense) ? dense : n;
}
__host__ __device__ inline size_t rfc_off_wsum(size_t n_pix) { return (64 + 8 * n_pix + 127) & ~(size_t)127; }
__host__ __device__ inline size_t rfc_off_recs(size_t n_pix) { return (rfc_off_wsum(n_pix) + 4 * n_pix + 127) & ~(size_t)127; }
__host__ __device__ inline size_t rfc_off_facb(size_t n_pix, size_t spp, bool all) { return (rfc_off_recs(n_pix) + 16 * 64 * rfc_cap_blocks(n_pix, spp, all) + 127) & ~(size_t)127; }
__host__ __device__ inline size_t rfc_bytes(size_t n_pix, size_t spp, bool mat, bool all) { return rfc_off_facb(n_pix, spp, all) + (mat ? ((4 * 64 * rfc_cap_blocks(n_pix, spp, all) + 127) & ~(size_t)127) : 0); }
static inline bool rfc_all(const ffx_scene_desc *sd) { return (sd->shadows & FFX_SHADOWS_CACHE_DENSE) != 0; }


// ---- reconstruction filter that spreads a sample over its 5x5-pixel window (include/ffx.h, ffx_scene_desc.rfilter) -------------------------
// A wave holds the 64 samples of ONE pixel, one per lane; what the film needs from it are 25 x (r, g, b, weight) sums over those samples —
// 100 cross-lane reductions (7 instructions each as DPP chains: ~700 at the 4-cycle rate, +65 % on the kernel).  Instead the lanes change
// roles through LDS: every lane parks its five weights per axis, its radiance and its "I am a sample" flag in 14 rows of 64 floats; then
// lane l becomes window entry l % 32 (25 of them) for the samples of half l / 32 and runs over its 32 samples with 16-byte LDS reads of the
// six rows it needs (its x weight, its y weight, the four channels): per four samples 6 reads, 4 multiplies and 16 fused multiply-adds,
// all in the 2-cycle class; the two halves meet in one cross-lane add per channel.  The rows alias the wide walk's stack (never live at the
// same time); the row pitch of 68 floats puts the rows a read touches into different banks.  The oracle sums in the same order (the two
// halves of every 64 samples apart, then together).  Measured (tools/rftime.py, 512^2 x 64 spp): see DESIGN 5.1.
// Tried and dropped: (1) lane = (entry, channel) over all 64 samples in two rounds — twice the LDS reads (96 x 1 KB per pixel: the CU's LDS
// port, shared by its four SIMDs, was then busy 80 % of the kernel's time) and 256 instead of 160 instructions: the kernel 0.386 -> 0.487 ms;
// (2) the same sums on the matrix pipe — v_mfma_f32_16x16x4_f32 with rows = channel (4 of 16 used), columns = window entry, K = samples
// (lanes ARE the K index: no role change, bit-identical k-ordered sums) — 32 instructions x 32 cycles of a pipe whose issue time adds to
// the VALU's here: 0.545 ms.
#define FFX_RF_ROW 68
#define FFX_RF_FLOATS (14 * FFX_RF_ROW)
static_assert(FFX_RF_ROW % 4 == 0, "rf_fold reads the rows as float4: the row pitch must keep them 16-byte aligned");
__device__ __forceinline__ void rf_weights(const RfC &c, float j, float (&w)[5]) {
  if (c.rec) { // (wave-uniform)
    const float x0 = -1.5f - j; // centre of window pixel 0 minus the sample position; pixel a: x0 + a
    const float e0 = __builtin_amdgcn_exp2f(c.aL * (x0 * x0)), r = __builtin_amdgcn_exp2f(c.aL2 * x0);
    const float e1 = e0 * r * c.k[0], e2 = e1 * r * c.k[1], e3 = e2 * r * c.k[2], e4 = e3 * r * c.k[3];
    w[0] = fmaxf(e0 - c.bias, 0.f); w[1] = fmaxf(e1 - c.bias, 0.f); w[2] = fmaxf(e2 - c.bias, 0.f); w[3] = fmaxf(e3 - c.bias, 0.f); w[4] = fmaxf(e4 - c.bias, 0.f);
    return;
  }
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const float x = ((float)(a - 2) + 0.5f) - j;
    w[a] = fmaxf(__expf(c.alpha * (x * x)) - c.bias, 0.f);
  }
}
static void rf_constants(float stddev, RfC &c) { // [EXT Mitsuba src/rfilters/gaussian.cpp] radius 4 stddev
  c.alpha = -1.0f / (2.0f * stddev * stddev);
  c.bias = expf(c.alpha * (4.0f * stddev) * (4.0f * stddev));
  c.aL = c.alpha * 1.4426950408889634f;
  c.aL2 = 2.0f * c.aL;
  for (int n = 0; n < 4; ++n) c.k[n] = (float)exp((double)c.alpha * (2 * n + 1));
  c.rec = c.alpha >= -8.0f ? 1 : 0;
}
// acc[ch] of lane l += sum over the samples 32 (l / 32) .. + 31 of this pass of  gx[a] gy[b] L[ch]  for window entry n = 5 b + a = l % 32 (< 25)
__device__ __forceinline__ void rf_fold(float *__restrict__ s_rf, int lane, const float (&gx)[5], const float (&gy)[5], float l0, float l1, float l2, float l3,
                                        float (&acc)[4]) {
  int lz = lane;
  asm volatile("" : "+v"(lz)); // (keeps the row addresses out of long-lived registers, as for s_foot)
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    s_rf[a * FFX_RF_ROW + lz] = gx[a];
    s_rf[(5 + a) * FFX_RF_ROW + lz] = gy[a];
  }
  s_rf[10 * FFX_RF_ROW + lz] = l0;
  s_rf[11 * FFX_RF_ROW + lz] = l1;
  s_rf[12 * FFX_RF_ROW + lz] = l2;
  s_rf[13 * FFX_RF_ROW + lz] = l3;
  __builtin_amdgcn_wave_barrier();
  const int n = min(lz & 31, 24), half = lz >> 5;
  const int b = (n * 13) >> 6, a = n - 5 * b; // n / 5, n % 5 for n < 25
  const float4 *rx = reinterpret_cast<const float4 *>(s_rf + a * FFX_RF_ROW) + 8 * half;
  const float4 *ry = reinterpret_cast<const float4 *>(s_rf + (5 + b) * FFX_RF_ROW) + 8 * half;
  const float4 *r0 = reinterpret_cast<const float4 *>(s_rf + 10 * FFX_RF_ROW) + 8 * half;
  float t0 = acc[0], t1 = acc[1], t2 = acc[2], t3 = acc[3];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 X = rx[k], Y = ry[k];
    const float4 L0 = r0[k], L1 = r0[k + FFX_RF_ROW / 4], L2 = r0[k + 2 * (FFX_RF_ROW / 4)], L3 = r0[k + 3 * (FFX_RF_ROW / 4)];
    const float w0 = X.x * Y.x, w1 = X.y * Y.y, w2 = X.z * Y.z, w3 = X.w * Y.w;
    t0 = __builtin_fmaf(w0, L0.x, t0); t1 = __builtin_fmaf(w0, L1.x, t1); t2 = __builtin_fmaf(w0, L2.x, t2); t3 = __builtin_fmaf(w0, L3.x, t3);
    t0 = __builtin_fmaf(w1, L0.y, t0); t1 = __builtin_fmaf(w1, L1.y, t1); t2 = __builtin_fmaf(w1, L2.y, t2); t3 = __builtin_fmaf(w1, L3.y, t3);
    t0 = __builtin_fmaf(w2, L0.z, t0); t1 = __builtin_fmaf(w2, L1.z, t1); t2 = __builtin_fmaf(w2, L2.z, t2); t3 = __builtin_fmaf(w2, L3.z, t3);
    t0 = __builtin_fmaf(w3, L0.w, t0); t1 = __builtin_fmaf(w3, L1.w, t1); t2 = __builtin_fmaf(w3, L2.w, t2); t3 = __builtin_fmaf(w3, L3.w, t3);
  }
  acc[0] = t0; acc[1] = t1; acc[2] = t2; acc[3] = t3;
  __builtin_amdgcn_wave_barrier();
}
// a pixel's 25 outgoing sums -> scratch [pixel][25][4]: lane n < 25 adds its two halves (samples 0..31 in lanes 0..31, 32..63 in lanes 32..63)
__device__ __forceinline__ void rf_store(float *__restrict__ part, uint32_t pix, int lane, const float (&acc)[4]) {
  const float h0 = __shfl_down(acc[0], 32), h1 = __shfl_down(acc[1], 32), h2 = __shfl_down(acc[2], 32), h3 = __shfl_down(acc[3], 32);
  if (lane < 25) reinterpret_cast<float4 *>(part)[(size_t)pix * 25 + lane] = make_float4(acc[0] + h0, acc[1] + h1, acc[2] + h2, acc[3] + h3);
}

// rf_fold + rf_store for a wave that holds SEVERAL pixels (k_render_fwd_blk<..., RF>: 2^ppw_log2 pixels x spp_w = 64 >> ppw_log2 sample slots, pixel q in
// lanes [q spp_w, (q + 1) spp_w)): the same 14 rows of 64 floats; then work item (pixel q, window entry n) runs over ITS pixel's slots in order — the
// fma chain rf_fold runs over a half's 32 samples, where the slots beyond the sample count add exact zeros and the second half is empty: the same bits
// as the pixel-per-wave kernel's sums.  50 items per round (two pixels x 25 entries), 2^ppw_log2 / 2 rounds: 160 multiply-adds per lane as in rf_fold,
// for 2^ppw_log2 pixels instead of one.
__device__ __forceinline__ void rf_fold_blk(float *__restrict__ s_rf, int lane, const float (&gx)[5], const float (&gy)[5], float l0, float l1, float l2, float l3,
                                            int ppw_log2, int bw_log2, int bx0, int by0, int W, int H, float *__restrict__ part) {
  int lz = lane;
  asm volatile("" : "+v"(lz));
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    s_rf[a * FFX_RF_ROW + lz] = gx[a];
    s_rf[(5 + a) * FFX_RF_ROW + lz] = gy[a];
  }
  s_rf[10 * FFX_RF_ROW + lz] = l0;
  s_rf[11 * FFX_RF_ROW + lz] = l1;
  s_rf[12 * FFX_RF_ROW + lz] = l2;
  s_rf[13 * FFX_RF_ROW + lz] = l3;
  __builtin_amdgcn_wave_barrier();
  const int spp_w = 64 >> ppw_log2, groups = spp_w >> 2; // float4 groups of a pixel's slots (spp_w >= 8: the block never exceeds 8 pixels)
  const int item = lz < 50 ? lz : 49, ql = item >= 25 ? 1 : 0, n = item - 25 * ql;
  const int b = (n * 13) >> 6, a = n - 5 * b; // n / 5, n % 5 for n < 25
  const int n_pix = 1 << ppw_log2;
  for (int q0 = 0; q0 < n_pix; q0 += 2) {
    const int q = q0 + ql; // (a block of one pixel does not get here: the host sends >= 2 pixels per wave, or the pixel-per-wave kernel)
    const float4 *rx = reinterpret_cast<const float4 *>(s_rf + a * FFX_RF_ROW) + q * groups;
    const float4 *ry = reinterpret_cast<const float4 *>(s_rf + (5 + b) * FFX_RF_ROW) + q * groups;
    const float4 *r0 = reinterpret_cast<const float4 *>(s_rf + 10 * FFX_RF_ROW) + q * groups;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    for (int k = 0; k < groups; ++k) {
      const float4 X = rx[k], Y = ry[k];
      const float4 L0 = r0[k], L1 = r0[k + FFX_RF_ROW / 4], L2 = r0[k + 2 * (FFX_RF_ROW / 4)], L3 = r0[k + 3 * (FFX_RF_ROW / 4)];
      const float w0 = X.x * Y.x, w1 = X.y * Y.y, w2 = X.z * Y.z, w3 = X.w * Y.w;
      t0 = __builtin_fmaf(w0, L0.x, t0); t1 = __builtin_fmaf(w0, L1.x, t1); t2 = __builtin_fmaf(w0, L2.x, t2); t3 = __builtin_fmaf(w0, L3.x, t3);
      t0 = __builtin_fmaf(w1, L0.y, t0); t1 = __builtin_fmaf(w1, L1.y, t1); t2 = __builtin_fmaf(w1, L2.y, t2); t3 = __builtin_fmaf(w1, L3.y, t3);
      t0 = __builtin_fmaf(w2, L0.z, t0); t1 = __builtin_fmaf(w2, L1.z, t1); t2 = __builtin_fmaf(w2, L2.z, t2); t3 = __builtin_fmaf(w2, L3.z, t3);
      t0 = __builtin_fmaf(w3, L0.w, t0); t1 = __builtin_fmaf(w3, L1.w, t1); t2 = __builtin_fmaf(w3, L2.w, t2); t3 = __builtin_fmaf(w3, L3.w, t3);
    }
    const int x = bx0 + (q & ((1 << bw_log2) - 1)), y = by0 + (q >> bw_log2);
    // (rf_store adds the second half's sums — here an empty half: + 0.f keeps the bits and turns a -0.f into the +0.f the other kernel stores)
    if (lz < 50 && q < n_pix && x < W && y < H)
      reinterpret_cast<float4 *>(part)[((size_t)y * W + x) * 25 + n] = make_float4(t0 + 0.f, t1 + 0.f, t2 + 0.f, t3 + 0.f);
  }
  __builtin_amdgcn_wave_barrier();
}

// the weights alone (the adjoint's first launch): one wave per pixel, the jitter decides everything
__global__ void __launch_bounds__(64) k_rf_weights(RfC rfc, int n_pix, int spp, uint32_t seed_key, float *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_rf[FFX_RF_FLOATS]; // (rf_fold reads it in 16-byte units)
  const int pix = blockIdx.x, lane = threadIdx.x;
  if (pix >= n_pix) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < (spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    float jx, jy, gx[5], gy[5];
    sample_jitter(seed_key, (uint32_t)pix * (uint32_t)spp + (uint32_t)s, jx, jy);
    rf_weights(rfc, jx, gx);
    rf_weights(rfc, jy, gy);
    rf_fold(s_rf, lane, gx, gy, 0.f, 0.f, 0.f, s < spp ? 1.f : 0.f, acc);
  }
  rf_store(part, (uint32_t)pix, lane, acc);
}

// second launch of either direction: a pixel's 25 incoming sums.  Forward: img = (r, g, b) / weight.  Adjoint (gimg != NULL):
// G = gimg / weight as float4 per pixel.  Window entry n = (a, b) of source pixel (x - (a - 2), y - (b - 2)) is what that pixel's
// samples sent HERE; summed in window order like the oracle.  A wave owns 64 pixels of one film row; for each window row b it stages the
// 80-byte (b, 0..4) segments of the 68 source records it needs through LDS — five lanes per segment, every byte of the scratch area read
// once — and lane x then picks entry a from record x + 4 - a.  (Read straight from memory a lane's 25 loads were 400 bytes apart from its
// neighbours': 0.061 ms for 105 MB, the vector L1 thrashing.)
#define FFX_RFG_WAVES 1 // (one-wave workgroups: the gather of one render runs beside the next render's kernel on the other stream — with four waves and 22 KB of LDS
                        //  per workgroup it waited for room on one compute unit: 1 742 -> 1 913 filtered renders/s; the waves never cooperated anyway)
// k_rf_gather's staging and 25 additions for the two gathers beside it (k_lights_gather, k_aov_gather): pixel (x0 + lane, y)'s sums into r, g, b, w;
// seg: the wave's 68 x 5 segment table in LDS
__device__ __forceinline__ void rf_window_sums(const float4 *__restrict__ part, int W, int H, int x0, int y, int lane, float4 *seg, float &r, float &g, float &b,
                                               float &w) {
  r = g = b = w = 0.f;
  for (int wb = 0; wb < 5; ++wb) {
    const int qy = y - (wb - 2);
    if (qy < 0 || qy >= H) continue; // (wave-uniform)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int e = lane + 64 * k; // element (record e / 5, entry e % 5) of the 68 x 5 segment table
      if (e < 340) {
        const int rec = e / 5, wa = e - 5 * rec;
        const int qx = x0 - 2 + rec;
        seg[e] = (qx >= 0 && qx < W) ? part[((size_t)qy * W + qx) * 25 + (wb * 5 + wa)] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int wa = 0; wa < 5; ++wa) {
      const float4 v = seg[(lane + 4 - wa) * 5 + wa];
      r += v.x; g += v.y; b += v.z; w += v.w;
    }
  }
}
__global__ void __launch_bounds__(64 * FFX_RFG_WAVES) k_rf_gather(const float4 *__restrict__ part, int W, int H, int fp16, void *__restrict__ img,
                                                                   const float *__restrict__ gimg, float4 *__restrict__ G, float *__restrict__ wsum_out = nullptr) {
  __shared__ float4 s_seg[FFX_RFG_WAVES][68 * 5];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = blockIdx.x * 64, y = blockIdx.y * FFX_RFG_WAVES + wv;
  if (y >= H) return; // (wave-uniform; the waves of a workgroup never synchronise)
  float4 *seg = s_seg[wv];
  // (rf_window_sums, stated here: through the shared piece the benchmark's gaussian gradient steps measured 0.35 % slower, outside the parent's spread)
  float r = 0.f, g = 0.f, b = 0.f, w = 0.f;
  for (int wb = 0; wb < 5; ++wb) {
    const int qy = y - (wb - 2);
    if (qy < 0 || qy >= H) continue; // (wave-uniform)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int e = lane + 64 * k; // element (record e / 5, entry e % 5) of the 68 x 5 segment table
      if (e < 340) {
        const int rec = e / 5, wa = e - 5 * rec;
        const int qx = x0 - 2 + rec;
        seg[e] = (qx >= 0 && qx < W) ? part[((size_t)qy * W + qx) * 25 + (wb * 5 + wa)] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int wa = 0; wa < 5; ++wa) {
      const float4 v = seg[(lane + 4 - wa) * 5 + wa];
      r += v.x; g += v.y; b += v.z; w += v.w;
    }
  }
  const int x = x0 + lane;
  if (x >= W) return;
  const size_t pix = (size_t)y * W + x;
  if (gimg) {
    const bool ok = w > 0.f;
    G[pix] = make_float4(ok ? gimg[pix * 3] / w : 0.f, ok ? gimg[pix * 3 + 1] / w : 0.f, ok ? gimg[pix * 3 + 2] / w : 0.f, 0.f);
    return;
  }
  const float v0 = w > 0.f ? r / w : 0.f, v1 = w > 0.f ? g / w : 0.f, v2 = w > 0.f ? b / w : 0.f;
  if (wsum_out) wsum_out[pix] = w; // (ffx_render_fwd_cache_filtered: the weight this pixel received, for the cached adjoint's G = gimg / weight)
  if (fp16 & 1) {
    _Float16 *p = (_Float16 *)img + pix * 3;
    p[0] = (_Float16)v0; p[1] = (_Float16)v1; p[2] = (_Float16)v2;
  } else {
    float *p = (float *)img + pix * 3;
    p[0] = v0; p[1] = v1; p[2] = v2;
  }
}

// lane n < 25: G of window pixel n = (a, b) of pixel (px, py), i.e. pixel (px + a - 2, py + b - 2); zero outside the film and in lanes >= 25
__device__ __forceinline__ float4 rf_window_g(const float4 *__restrict__ G, int px, int py, int W, int H, int lane, bool live) {
  const int b = (lane * 13) >> 6, a = lane - 5 * b;
  const int tx = px + a - 2, ty = py + b - 2;
  if (!live || lane >= 25 || tx < 0 || tx >= W || ty < 0 || ty >= H) return make_float4(0.f, 0.f, 0.f, 0.f);
  return G[(size_t)ty * W + tx];
}
// the adjoint weight of a sample with jitter (jx, jy): box: g; RF: lanes 0..24 hold G of the pixel's window (rf_window_g) and q is the sum over the
// window of filter weight x G — window order n = 0..24, w = gx[n % 5] * gy[n / 5], one fused multiply-add per channel and n
template <bool RF>
__device__ __forceinline__ void sample_adjoint(const RfC &rf, float jx, float jy, const float (&g)[3], float (&q)[3]) {
  q[0] = g[0]; q[1] = g[1]; q[2] = g[2];
  if (RF) { // (all lanes: the readlanes need the whole wave)
    float gx[5], gy[5];
    rf_weights(rf, jx, gx);
    rf_weights(rf, jy, gy);
    q[0] = q[1] = q[2] = 0.f;
#pragma unroll
    for (int n = 0; n < 25; ++n) {
      const float w = gx[n % 5] * gy[n / 5];
      q[0] = __builtin_fmaf(w, __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(g[0]), n)), q[0]);
      q[1] = __builtin_fmaf(w, __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(g[1]), n)), q[1]);
      q[2] = __builtin_fmaf(w, __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(g[2]), n)), q[2]);
    }
  }
}

#ifndef FFX_PK_MAT_WAVES
#define FFX_PK_MAT_WAVES 7 // material rows: 75 VGPRs (72 at this setting without spills; 8 waves spill 4)
#endif
// RF (ffx_render_fwd_filtered): instead of the pixel's mean, the wave leaves the 25 x 4 sums its samples send to its 5x5 window in `cache`
// (here: the scratch area, [pixel][25][4] floats; no adjoint cache in this mode) — see rf_fold above.
// RFC (ffx_render_fwd_cache_filtered; RF && !ADJ): additionally the per-sample records of the filtered film's adjoint cache (rfc_off_* above);
// its base travels in `adj_gtex`, the record areas' offsets (128-byte units) in cache_foot_off / cache_foot_b_off.
// R (rays per lane) is 1 and stays in the template head: the benchmark and the committed profiles read ADJ and RF by their position
// in the instance name as the profiler prints it, k_render_fwd_pk<1, true, 1, false, false, false>.  (Its [R] arrays and loops: see as1.)
// PLAIN (last, so the generic instances keep their printed names): the instance for a scene about which the host proved, before the launch, what the
// generic one tests per sample (plain_scene below): principled rows that travel inline with their pre-rows, no optional lobe in any row, no smooth
// record, a rigid spot, a one-channel projector texture, an f32 box film in one pass.  Same arithmetic, same order, same bits; FFX_K8_PLAIN=0 keeps
// the generic instance.
// CACHE (behind PLAIN for the same reason; PLAIN only): whether the launch writes the adjoint cache is a fact of the instance too — the launcher knows
// it when it picks.  The plain forward (!ADJ, !CACHE) holds no footprint fold, no stray-record allocation, no header write and no footprint store
// (as a run-time `cache != nullptr` that dead arm kept scalars live through the whole kernel: 12 SGPR spills, 4 without it); the cache-writing plain
// forward (!ADJ, CACHE) is the L1-loss step's render.  The generic instances keep the run-time test.
// (rk, the last parameter: read in place through kernarg_rect, which is defined behind the kernel from the kernel's own parameter types)
template <int R, bool WIDE, int MATM, bool ADJ = false, bool RF = false, bool RFC = false, bool PLAIN = false, bool CACHE = false>
__global__ void __launch_bounds__(PK_BLOCK) __attribute__((amdgpu_waves_per_eu(MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES, MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES)))
    k_render_fwd_pk(ShadeK c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs, uint32_t astride,
                    WideScene ws, const float *__restrict__ albedo, const float *__restrict__ tex, int spp, uint32_t seed_key, int tiles_x, int n_tiles, int remap,
                    int fp16, void *__restrict__ img, char *__restrict__ cache, int ppw, float inv_spp_arg, uint32_t cache_foot_off, uint32_t cache_arena_off,
                    uint32_t cache_foot_b_off, const float4 *__restrict__ nrec, const float4 *__restrict__ gn, uint32_t cap_stray,
                    const float *__restrict__ adj_gimg, float *__restrict__ adj_gtex, float *__restrict__ adj_dot, RectK rk) {
  constexpr bool MAT = MATM != 0, TEX = MATM == 2;
  constexpr int MS = MAT ? FFX_MAT_STRIDE : 3; // floats per material row
  // adj_gtex (ffx_render_fwd_adjoint): the adjoint of a loss whose gradient gimg does not depend on the image (a loss linear in it) needs
  // no second pass — the pixel's footprint is scattered into gtex where it is formed instead of being stored for K9, stray samples at
  // once: no cache, no arena that could overflow, no launch behind the render.  `fold`: the footprint bookkeeping runs for either mode.
  // (ADJ is a template parameter: as a run-time mode its three pointers and the epilogue cost the plain forward a dozen scalar spills)
  // RF && ADJ (ffx_render_fwd_adjoint_filtered): adj_gimg is then G = gimg / weight as float4 per pixel (k_rf_gather) and every lit sample
  // enters the pixel's footprint with ITS OWN gradient — sum over its window of w_n G[pixel + n], times albedo and colour — already applied;
  // the epilogue scatters the footprint as it is.  1-channel textures only (the host refuses the other).
  // CACHE_ARM: the instance can write the box film's adjoint cache; has_cache: this launch does (PLAIN: a constant of the instance)
  constexpr bool CACHE_ARM = !ADJ && !RF && (!PLAIN || CACHE), FOLD_CT = RF ? ADJ : (ADJ || CACHE);
  const bool has_cache = PLAIN ? CACHE : cache != nullptr;
  const bool fold = (RF || PLAIN) ? FOLD_CT : (ADJ || has_cache);
  constexpr int WSTACK_N = WIDE ? FFX_WSTACK : 1, RF_N = (FFX_RF_FLOATS * 4 + 7) / 8;
  __shared__ __attribute__((aligned(16))) uint2 s_wstack[RF ? (WSTACK_N > RF_N ? WSTACK_N : RF_N) : WSTACK_N]; // (RF: the filter's rows alias the walk's stack and are read in 16-byte units)
  __shared__ float s_foot[32]; // the pixel's 5x5 texture footprint (adjoint cache)
  __shared__ float s_foot_b[MAT ? 32 : 1]; // material rows: the footprint of the base_color-independent part
  static_assert(R == 1, "one ray per lane: the adjoint cache is written one pixel at a time");
  static_assert(!RFC || (RF && !ADJ), "RFC: the filtered forward that writes the per-sample adjoint records");
  static_assert(!PLAIN || (MATM == 1 && !RF && !RFC), "PLAIN: principled rows, box film");
  static_assert(!CACHE || (PLAIN && !ADJ), "CACHE: the plain-scene forward that writes the adjoint cache");
  FFX_TINIT();
  FFX_TSTART(twave);
  FFX_TSTART(tpro);
  // The per-pixel radiance sums are live across all three walks of every pass but touched once per pass:
  // they are parked in LDS (which these kernels do not otherwise use) instead of holding 3R VGPRs that
  // the allocator would spill to scratch at 8 waves per SIMD.  Each lane only ever reads its own slots.
  __shared__ float s_acc[R][RF ? 4 : 3][PK_BLOCK];
  // each wave of the workgroup owns its own tile; the waves never synchronise
  // a wave walks `ppw` (1, 2 or 4) of its tile's four pixels; 4 / ppw waves share a tile
  const int wv = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x, remap) * (blockDim.x >> 6) + (threadIdx.x >> 6)); // wave-uniform: say so
  const int wpt_log2 = ppw == 1 ? 2 : (ppw == 2 ? 1 : 0); // waves per tile = 4 / ppw, a power of two: shifts, not divisions
  const int tile = wv >> wpt_log2, sub0 = (wv & ((1 << wpt_log2) - 1)) * ppw;
  const int lane = threadIdx.x & 63;
  const int W = c.cam.W, H = c.cam.H; // (the only direct use of the by-value copy)
  const int passes = PLAIN ? 1 : (spp + 63) >> 6;
  // (wave-uniform, used once per pixel: kept in an SGPR — as a VGPR it was live across the whole kernel and spilled)
  const float inv_spp_u = inv_spp_arg; // 1 / spp from the host (a kernel argument is scalar by construction; the division here was ten vector instructions per wave)
  if constexpr (CACHE_ARM) {
    if (has_cache && wv == 0 && lane == 0) reinterpret_cast<CacheHdr *>(cache)->cap_stray = cap_stray; // (read back by K9 and ffx_render_cache_status; no wave of this launch reads it)
  }
  if constexpr (RFC) { // (the arena's counters were cleared in front of this launch — launch_apex / FFX_RENDER_CACHE_ZEROED; nobody here reads the capacity word)
    if (wv == 0 && lane == 0) reinterpret_cast<CacheHdr *>(adj_gtex)->cap_stray = cap_stray;
  }
  FFX_TSTOP(tpro, 25);
  // UNI (the plain-scene instances, next to their rectangle tables): the tile's origin — a division through a float reciprocal and its way back into
  // scalar registers — is found once per wave instead of once per pixel, and the wave-uniform `live` is branched on as the scalar it is
  constexpr bool RECT_I = PLAIN && !CACHE && FFX_K8_RECTTAB, UNI = RECT_I && FFX_K8_RECT_UNI; // (RECT_I: the instance reads the film's tables)
  int bx0[R], by0[R];
  if constexpr (UNI) packet_pixels<R>(tile, tiles_x, 0, bx0, by0); // (sub 0: the tile's first pixel)
  for (int sub = sub0; sub < sub0 + ppw; ++sub) {
    int px[R], py[R];
    if constexpr (UNI) { px[0] = bx0[0] + (sub & 1); py[0] = by0[0] + (sub >> 1); }
    else packet_pixels<R>(tile, tiles_x, sub, px, py);
    bool live[R], any_live = false;
    uint32_t pix[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live[r] = tile < n_tiles && px[r] < W && py[r] < H;
      any_live |= live[r];
      pix[r] = (uint32_t)py[r] * (uint32_t)W + (uint32_t)px[r];
    }
    if constexpr (UNI) {
      if (!any_live) continue;
    } else {
      if (wballot(any_live) == 0ull) continue;
    }
    // adjoint cache: window origin (wave-uniform) and shape of this pixel's footprint, -1 until a sample is lit
    int fox = -1, foy = -1, fshape = -1;
    float fin0 = 0.f, fin1 = 0.f, fin2 = 0.f; // the pixel's value as stored (ffx_render_fwd_adjoint: <gimg, img>)
    float rfacc[4] = {0.f, 0.f, 0.f, 0.f}; // RF: this lane's window entry (lane % 32, samples of half lane / 32), four channels, summed over the passes
    uint32_t rfc_mask = 0u; // RFC: the passes of this pixel that hold a lit sample (wave-uniform)
    uint32_t rfc_first = 0u; // ... the arena block of the first of them (the later passes follow it), and that pass; rfc_drop: the arena was full
    int rfc_first_pass = -1;
    bool rfc_drop = false;
    for (int pass = 0; pass < passes; ++pass) {
      const int s = pass * 64 + lane;
      bool active[R];
      v3 o[R], d[R];
      float nt[R], ft[R];
      FFX_TSTART(tk);
      const CamK &cam = kernarg_shade().cam; // phase: ray generation
#pragma unroll
      for (int r = 0; r < R; ++r) {
        active[r] = live[r] && s < spp;
        uint32_t idx = pix[r] * (uint32_t)spp + (uint32_t)s;
        float jx, jy;
        sample_jitter(seed_key, idx, jx, jy);
        cam_ray<PLAIN && FFX_K8_BAND>(cam, ((float)px[r] + jx) * cam.inv_w, ((float)py[r] + jy) * cam.inv_h, o[r], d[r], nt[r], ft[r]);
      }
      FFX_TSTOP(tk, 16);
      SampleTerms st[R];
      // (fp16 carries the call's flags: bit 0 fp16 film, bit 1 FFX_RENDER_SPARSE_ADJOINT — then the cache-writing forward may
      // skip dark footprints too: the caller only wants gradients of texels whose value is not zero)
      shade_sample_pk<WIDE, MATM, PLAIN, RECT_I>(nodes, recs, arecs, astride, ws, s_wstack, active[0], o[0], d[0], nt[0], ft[0], st[0], nrec, gn, px[0], py[0], ((fold || RFC) && !(fp16 & 2)) ? nullptr : tex);
      FFX_TSTOP(tk, 17);
      if constexpr (RFC) {
        // ---- the filtered film's adjoint cache: this pass's 64 records, if any of its samples is lit (one 1 KB store per wave)
        const bool lit = active[0] && st[0].hit && st[0].has_proj;
        if (wballot(lit) != 0ull && !rfc_drop) {
          char *rfc = reinterpret_cast<char *>(adj_gtex);
          if (rfc_first_pass < 0) { // the pixel's first lit pass: blocks for it and for every pass behind it
            const uint32_t want = (uint32_t)(passes - pass);
            if (cap_stray >= (uint32_t)W * (uint32_t)H * (uint32_t)passes) {
              // the arena holds a block for every pass of every pixel (up to 2^18 blocks: 512 x 512 x 64 spp): the pixel's own — nothing to take,
              // nothing that can run out
              rfc_first = pix[0] * (uint32_t)passes + (uint32_t)pass;
              rfc_first_pass = pass;
            } else {
              // one atomic of the wave — on ONE of eight counters, picked so that neighbouring pixels take different ones: the lit pixels of a
              // laser dot are rendered together, and same-address atomics from eight XCDs serialise at ~90 ns each (one counter: 178 k of them
              // on configs[4], twice the kernel's own time; at 512 x 512 x 64 the filtered gradient step lost 8 %)
              const uint32_t sub = ((uint32_t)px[0] + 3u * (uint32_t)py[0]) & 7u, sub_cap = cap_stray >> 3;
              uint32_t b0 = 0u;
              if (lane == 0) b0 = atomicAdd(&reinterpret_cast<CacheHdr *>(rfc)->pad[1 + sub], want);
              b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
              if (b0 + want > sub_cap) {
                rfc_drop = true; // (sub-arena full: this pixel keeps no records — counted, the adjoint is poisoned, the caller re-traces)
                if (lane == 0) atomicAdd(&reinterpret_cast<CacheHdr *>(rfc)->dropped, 1u);
              } else {
                rfc_first = sub * sub_cap + b0;
                rfc_first_pass = pass;
              }
            }
          }
        }
        if (wballot(lit) != 0ull && !rfc_drop) {
          rfc_mask |= 1u << pass;
          if (s < spp) {
            char *rfc = reinterpret_cast<char *>(adj_gtex);
            const size_t si = (size_t)(rfc_first + (uint32_t)(pass - rfc_first_pass)) * 64u + (size_t)(s & 63);
            uint4 rec = make_uint4(0u, 0u, 0u, 0u);
            if (lit) rec = make_uint4((uint32_t)(st[0].ubx + 1) | ((uint32_t)(st[0].uby + 1) << 12) | ((uint32_t)st[0].shape << 24), __float_as_uint(st[0].wx1),
                                      __float_as_uint(st[0].wy1), __float_as_uint(st[0].proj_fac));
            reinterpret_cast<uint4 *>(rfc + ((size_t)cache_foot_off << 7))[si] = rec;
            if constexpr (MAT) reinterpret_cast<float *>(rfc + ((size_t)cache_foot_b_off << 7))[si] = lit ? st[0].proj_fac_b : 0.f;
          }
        }
      }
      if (fold) {
        // ---- adjoint cache: fold this pass's lit samples into the pixel's footprint
        const bool lit = active[0] && st[0].hit && st[0].has_proj;
        const wmask litm = wballot(lit);
        if (litm != 0ull) {
          if (fox < 0) { // first lit samples of the pixel: the window starts at their smallest tap
            // (the footprint is cleared HERE, not at the start of every pixel: 96 % of the pixels of a dot pattern's render never get here.
            // Index laundered: the compiler otherwise keeps &s_foot[lane] in a VGPR across the whole kernel — and, at the 64-VGPR budget,
            // spills it: 256 B of scratch traffic per wave for an address that costs two instructions)
            int lz = lane;
            asm volatile("" : "+v"(lz));
            if (lz < 32) s_foot[lz] = 0.f;
            if constexpr (MAT) { if (lz < 32) s_foot_b[lz] = 0.f; }
            __builtin_amdgcn_wave_barrier();
            fox = (int)wave_reduce_nn<false>(lit ? (uint32_t)st[0].ix0 : 0xffffffffu);
            foy = (int)wave_reduce_nn<false>(lit ? (uint32_t)st[0].iy0 : 0xffffffffu);
            fshape = __builtin_amdgcn_readlane(st[0].shape, wff1(litm));
          }
          const bool in_win = lit && st[0].ix0 >= fox && st[0].ix1 <= fox + 4 && st[0].iy0 >= foy && st[0].iy1 <= foy + 4 && st[0].shape == fshape;
          float rf_pf = 0.f; // RF && ADJ: proj_fac (and proj_fac_b) of this sample with its filtered gradient, albedo and colour applied
          if constexpr (RF && ADJ) {
            const ShadeK &cr = kernarg_shade();
            const float4 gw = rf_window_g(reinterpret_cast<const float4 *>(adj_gimg), px[0], py[0], W, H, lane, live[0]);
            const float gwin[3] = {gw.x, gw.y, gw.z};
            float jx, jy, a[3];
            sample_jitter(seed_key, pix[0] * (uint32_t)spp + (uint32_t)s, jx, jy);
            sample_adjoint<true>(cr.rf, jx, jy, gwin, a);
            if (lit) rf_pf = tap_value_1ch(a, mat_table(cr) + MS * st[0].shape, cr.p_color, st[0].proj_fac, MAT ? st[0].proj_fac_b : 0.f, 1.0f); // (the weight inside G normalises)
          }
          if (in_win) {
            const float pf = (RF && ADJ) ? rf_pf : st[0].proj_fac;
            const int bx0 = st[0].ix0 - fox, bx1 = st[0].ix1 - fox, by0 = (st[0].iy0 - foy) * 5, by1 = (st[0].iy1 - foy) * 5;
            atomicAdd(&s_foot[by0 + bx0], pf * st[0].wy0 * st[0].wx0);
            atomicAdd(&s_foot[by0 + bx1], pf * st[0].wy0 * st[0].wx1);
            atomicAdd(&s_foot[by1 + bx0], pf * st[0].wy1 * st[0].wx0);
            atomicAdd(&s_foot[by1 + bx1], pf * st[0].wy1 * st[0].wx1);
            if constexpr (MAT && !(RF && ADJ)) {
              const float pb = st[0].proj_fac_b;
              if (pb != 0.f) {
                atomicAdd(&s_foot_b[by0 + bx0], pb * st[0].wy0 * st[0].wx0);
                atomicAdd(&s_foot_b[by0 + bx1], pb * st[0].wy0 * st[0].wx1);
                atomicAdd(&s_foot_b[by1 + bx0], pb * st[0].wy1 * st[0].wx0);
                atomicAdd(&s_foot_b[by1 + bx1], pb * st[0].wy1 * st[0].wx1);
              }
            }
          }
          const wmask straym = wballot(lit && !in_win);
          // fused adjoint: the four taps of a sample that does not fit the footprint, at once.  sample_scatter's values (tap_value_1ch / tap_value_3ch, times
          // wy, times wx, zero values skipped), written out: as a call, with the texel offsets scaled by a run-time tc, the ADJ instances spill other scalars
          if (ADJ && straym != 0ull) {
            if constexpr (RF) {
              if (lit && !in_win && rf_pf != 0.f) {
                const ShadeK &ca = kernarg_shade();
                atomicAdd(adj_gtex + (size_t)st[0].iy0 * ca.tw + st[0].ix0, rf_pf * st[0].wy0 * st[0].wx0);
                atomicAdd(adj_gtex + (size_t)st[0].iy0 * ca.tw + st[0].ix1, rf_pf * st[0].wy0 * st[0].wx1);
                atomicAdd(adj_gtex + (size_t)st[0].iy1 * ca.tw + st[0].ix0, rf_pf * st[0].wy1 * st[0].wx0);
                atomicAdd(adj_gtex + (size_t)st[0].iy1 * ca.tw + st[0].ix1, rf_pf * st[0].wy1 * st[0].wx1);
              }
            } else
            if (lit && !in_win) {
              const ShadeK &ca = kernarg_shade();
              const float g0 = adj_gimg[(size_t)pix[0] * 3], g1 = adj_gimg[(size_t)pix[0] * 3 + 1], g2 = adj_gimg[(size_t)pix[0] * 3 + 2];
              const float *alb = mat_table(ca) + MS * st[0].shape;
              const float pf = st[0].proj_fac, pb = MAT ? st[0].proj_fac_b : 0.f;
              const float wx0 = st[0].wx0, wx1 = st[0].wx1, wy0 = st[0].wy0, wy1 = st[0].wy1;
              if (PLAIN || ca.tc == 1) {
                float wsv = (g0 * alb[0] * ca.p_color[0] + g1 * alb[1] * ca.p_color[1] + g2 * alb[2] * ca.p_color[2]) * pf * inv_spp_u;
                if (pb != 0.f) wsv += (g0 * ca.p_color[0] + g1 * ca.p_color[1] + g2 * ca.p_color[2]) * pb * inv_spp_u;
                if constexpr (PLAIN && FFX_K8_OFF32) { // (gtex has the texture's shape: the same 32-bit texel offsets)
                  if (wsv != 0.f) {
                    const uint32_t r0 = __umul24((uint32_t)st[0].iy0, (uint32_t)ca.tw), r1 = __umul24((uint32_t)st[0].iy1, (uint32_t)ca.tw);
                    atomicAdd(const_cast<float *>(&at32<float>(adj_gtex, (r0 + (uint32_t)st[0].ix0) << 2)), wsv * wy0 * wx0);
                    atomicAdd(const_cast<float *>(&at32<float>(adj_gtex, (r0 + (uint32_t)st[0].ix1) << 2)), wsv * wy0 * wx1);
                    atomicAdd(const_cast<float *>(&at32<float>(adj_gtex, (r1 + (uint32_t)st[0].ix0) << 2)), wsv * wy1 * wx0);
                    atomicAdd(const_cast<float *>(&at32<float>(adj_gtex, (r1 + (uint32_t)st[0].ix1) << 2)), wsv * wy1 * wx1);
                  }
                } else
                if (wsv != 0.f) {
                  atomicAdd(adj_gtex + (size_t)st[0].iy0 * ca.tw + st[0].ix0, wsv * wy0 * wx0);
                  atomicAdd(adj_gtex + (size_t)st[0].iy0 * ca.tw + st[0].ix1, wsv * wy0 * wx1);
                  atomicAdd(adj_gtex + (size_t)st[0].iy1 * ca.tw + st[0].ix0, wsv * wy1 * wx0);
                  atomicAdd(adj_gtex + (size_t)st[0].iy1 * ca.tw + st[0].ix1, wsv * wy1 * wx1);
                }
              } else {
                const size_t o00 = ((size_t)st[0].iy0 * ca.tw + st[0].ix0) * 3, o01 = ((size_t)st[0].iy0 * ca.tw + st[0].ix1) * 3;
                const size_t o10 = ((size_t)st[0].iy1 * ca.tw + st[0].ix0) * 3, o11 = ((size_t)st[0].iy1 * ca.tw + st[0].ix1) * 3;
                const float gg[3] = {g0, g1, g2};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                  float wsv = gg[ch] * alb[ch] * pf * inv_spp_u;
                  if (pb != 0.f) wsv += gg[ch] * pb * inv_spp_u;
                  if (wsv == 0.f) continue;
                  atomicAdd(adj_gtex + o00 + ch, wsv * wy0 * wx0);
                  atomicAdd(adj_gtex + o01 + ch, wsv * wy0 * wx1);
                  atomicAdd(adj_gtex + o10 + ch, wsv * wy1 * wx0);
                  atomicAdd(adj_gtex + o11 + ch, wsv * wy1 * wx1);
                }
              }
            }
          } else if constexpr (CACHE_ARM) {
            if (straym != 0ull) { // single samples that do not fit the footprint: one allocation per wave
              CacheHdr *hdr = reinterpret_cast<CacheHdr *>(cache);
              const uint32_t n = (uint32_t)wpop(straym);
              uint32_t base = 0;
              if (lane == 0) base = atomicAdd(&hdr->n_stray, n);
              base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
              const uint32_t cap = cap_stray; // (a kernel argument: the header may have been cleared as a whole by the caller, FFX_RENDER_CACHE_ZEROED)
              if (base + n <= cap) {
                if (lit && !in_win) {
                  CacheStray *rec = reinterpret_cast<CacheStray *>(cache + ((size_t)cache_arena_off << 7)) + base + mbcnt64(straym);
                  rec->pix = pix[0];
                  rec->xy_shape = (uint32_t)(st[0].ubx + 1) | ((uint32_t)(st[0].uby + 1) << 12) | ((uint32_t)st[0].shape << 24);
                  rec->ax = st[0].wx1;
                  rec->ay = st[0].wy1;
                  rec->fac = st[0].proj_fac;
                  if constexpr (MAT) rec->fac_b = st[0].proj_fac_b;
                }
              } else if (lane == 0) {
                atomicAdd(&hdr->dropped, n); // arena exhausted (never seen: it holds 1/64 of all samples, strays are ~0.1 %)
              }
            }
          }
        }
      }
      const ShadeK &ct = kernarg_shade(); // phase: texture gather and accumulation
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float L[3] = {0.f, 0.f, 0.f}; // this pass's contribution of the lane's sample
        // (a textured row: the sample's own base colour; zero where nothing lit it, and then its terms are zero too)
        if constexpr (PLAIN && FFX_K8_OFF32) {
          if (st[r].hit) sample_colour<true, true>(ct, st[r], tex, &at32<float>(ct.mat_h, __umul24((uint32_t)st[r].shape, MS * 4u)), MAT, L);
        } else
        if (st[r].hit) sample_colour<PLAIN>(ct, st[r], tex, TEX ? st[r].base : mat_table(ct) + MS * st[r].shape, MAT, L);
        float c0 = L[0], c1 = L[1], c2 = L[2];
        if constexpr (RF) {
          // the lane's sample -> its 25 window entries (weights from the jitter, re-derived: two hashes instead of two live registers)
          // (re-derived: two hashes instead of two live registers — parking the jitter in LDS instead was tried in round 5: the film's fold keeps
          // the CU's LDS port busy as it is, filtered render 0.531 -> 0.559 ms)
          float jx, jy, gx[5], gy[5];
          sample_jitter(seed_key, pix[r] * (uint32_t)spp + (uint32_t)s, jx, jy);
          rf_weights(ct.rf, jx, gx);
          rf_weights(ct.rf, jy, gy);
          if (pass > 0) { rfacc[0] = s_acc[r][0][threadIdx.x]; rfacc[1] = s_acc[r][1][threadIdx.x]; rfacc[2] = s_acc[r][2][threadIdx.x]; rfacc[3] = s_acc[r][3][threadIdx.x]; }
          rf_fold(reinterpret_cast<float *>(s_wstack), lane, gx, gy, c0, c1, c2, active[r] ? 1.f : 0.f, rfacc); // (the weight channel: every sample drawn counts)
          if (pass + 1 < passes) { s_acc[r][0][threadIdx.x] = rfacc[0]; s_acc[r][1][threadIdx.x] = rfacc[1]; s_acc[r][2][threadIdx.x] = rfacc[2]; s_acc[r][3][threadIdx.x] = rfacc[3]; }
          else if (live[r]) rf_store(reinterpret_cast<float *>(cache), pix[r], lane, rfacc);
          continue;
        }
        // running sums of a pixel that needs several 64-sample passes are parked in LDS between the passes; the
        // usual single pass never touches it (it had cost 15 LDS operations per pixel)
        if (pass > 0) { c0 += s_acc[r][0][threadIdx.x]; c1 += s_acc[r][1][threadIdx.x]; c2 += s_acc[r][2][threadIdx.x]; }
        if (pass + 1 < passes) {
          s_acc[r][0][threadIdx.x] = c0; s_acc[r][1][threadIdx.x] = c1; s_acc[r][2][threadIdx.x] = c2;
        } else {
          // last pass: combine the 64 lanes in a fixed order (deterministic, no atomics) — the three channel sums in
          // interleaved DPP chains (FFX_R3_ALL, see wave_reduce3_nn: butterfly inside the rows, row_bcast to lane 63)
          asm(FFX_R3_ALL("v_add_f32_dpp") : "+v"(c0), "+v"(c1), "+v"(c2));
          const float a0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(c0), 63));
          const float a1 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(c1), 63));
          const float a2 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(c2), 63));
          if (lane == 0 && live[r]) {
            size_t o = (size_t)pix[r] * 3;
            if (!PLAIN && (fp16 & 1)) {
              _Float16 *p = (_Float16 *)img;
              p[o] = (_Float16)vmul_s(a0, inv_spp_u);
              p[o + 1] = (_Float16)vmul_s(a1, inv_spp_u);
              p[o + 2] = (_Float16)vmul_s(a2, inv_spp_u);
            } else {
              float *p = (float *)img;
              p[o] = vmul_s(a0, inv_spp_u);
              p[o + 1] = vmul_s(a1, inv_spp_u);
              p[o + 2] = vmul_s(a2, inv_spp_u);
            }
          }
          if (ADJ && adj_dot) { // (wave-uniform values: the same in every lane)
            const bool half_film = !PLAIN && (fp16 & 1);
            fin0 = half_film ? (float)(_Float16)vmul_s(a0, inv_spp_u) : vmul_s(a0, inv_spp_u);
            fin1 = half_film ? (float)(_Float16)vmul_s(a1, inv_spp_u) : vmul_s(a1, inv_spp_u);
            fin2 = half_film ? (float)(_Float16)vmul_s(a2, inv_spp_u) : vmul_s(a2, inv_spp_u);
          }
        }
      }
      FFX_TSTOP(tk, 23);
    }
    if constexpr (RFC) { // the pixel's header: which of its passes hold records
      if (live[0] && lane == 0) {
        CachePix hp;
        hp.x0 = (int16_t)(rfc_first & 0xffffu); hp.y0 = (int16_t)(rfc_first >> 16); hp.shape = (uint16_t)(rfc_first_pass < 0 ? 0 : rfc_first_pass); hp.lit = (uint16_t)rfc_mask;
        reinterpret_cast<CachePix *>(reinterpret_cast<char *>(adj_gtex) + 64)[pix[0]] = hp;
      }
    }
    if (ADJ && RF && live[0]) { // filtered fused adjoint: the footprint already carries every sample's own gradient
      __builtin_amdgcn_wave_barrier();
      const ShadeK &ca = kernarg_shade();
      int lw = lane;
      asm volatile("" : "+v"(lw));
      if (fox >= 0 && lw < 25) {
        const float w = s_foot[lw];
        const int ey = (lw * 13) >> 6, ex = lw - 5 * ey;
        if (w != 0.f) atomicAdd(adj_gtex + (size_t)(foy + ey) * ca.tw + (fox + ex), w);
      }
    }
    if (ADJ && !RF && live[0] && (fox >= 0 || adj_dot)) { // fused adjoint: the pixel's footprint x (gimg . albedo . colour) / spp goes straight into gtex
      __builtin_amdgcn_wave_barrier();
      const ShadeK &ca = kernarg_shade();
      const float g[3] = {adj_gimg[(size_t)pix[0] * 3], adj_gimg[(size_t)pix[0] * 3 + 1], adj_gimg[(size_t)pix[0] * 3 + 2]};
      if (fox >= 0) {
        int lw = lane;
        asm volatile("" : "+v"(lw));
        if (lw < 25) {
          const float *alb = (PLAIN && FFX_K8_OFF32) ? ca.mat_h + MS * fshape : mat_table(ca) + MS * fshape; // (fshape: wave-uniform)
          const float w = s_foot[lw];
          float wb = 0.f;
          if constexpr (MAT) wb = s_foot_b[lw];
          const int ey = (lw * 13) >> 6, ex = lw - 5 * ey; // lw / 5, lw % 5 for lw < 25
          const int tx = fox + ex, ty = foy + ey;
          if (w != 0.f || wb != 0.f) {
            if (PLAIN || ca.tc == 1) {
              const float val = foot_value_1ch(g_alb_colour(g, alb, ca.p_color) * inv_spp_u, g_colour(g, ca.p_color) * inv_spp_u, w, wb);
              if constexpr (PLAIN && FFX_K8_OFF32) {
                if (val != 0.f) atomicAdd(const_cast<float *>(&at32<float>(adj_gtex, (__umul24((uint32_t)ty, (uint32_t)ca.tw) + (uint32_t)tx) << 2)), val);
              } else
              if (val != 0.f) atomicAdd(adj_gtex + (size_t)ty * ca.tw + tx, val);
            } else {
              float *t = adj_gtex + ((size_t)ty * ca.tw + tx) * 3;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch)
                if (g[ch] != 0.f) atomicAdd(t + ch, foot_value_3ch(g[ch], alb[ch], inv_spp_u, w, wb));
            }
          }
        }
      }
      if (adj_dot && lane == 0) { // <gimg, img> of this pixel into one of FFX_ADJOINT_DOT_SLOTS partial sums (256 cache lines: a quarter of a
        const float dd = g[0] * fin0 + g[1] * fin1 + g[2] * fin2; // million atomics over the launch meet ~1000 times per line, not on one address)
        if (dd != 0.f) atomicAdd(adj_dot + (pix[0] & (FFX_ADJOINT_DOT_SLOTS - 1)), dd);
      }
    }
    if constexpr (CACHE_ARM) {
      if (has_cache && live[0]) { // the pixel's slot: header always, the footprint only if something was lit
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
          CachePix hp;
          hp.x0 = (int16_t)fox; hp.y0 = (int16_t)foy;
          hp.shape = (uint16_t)(fshape < 0 ? 0 : fshape);
          hp.lit = fox >= 0 ? 1 : 0;
          reinterpret_cast<CachePix *>(cache + 64)[pix[0]] = hp; // one 8-byte store
        }
        int lw = lane;
        asm volatile("" : "+v"(lw));
        if (fox >= 0 && lw < 25) reinterpret_cast<CacheFoot *>(cache + ((size_t)cache_foot_off << 7))[pix[0]].w[lw] = s_foot[lw];
        if constexpr (MAT) {
          if (fox >= 0 && lw < 25) reinterpret_cast<CacheFoot *>(cache + ((size_t)cache_foot_b_off << 7))[pix[0]].w[lw] = s_foot_b[lw];
        }
      }
    }
  }
  FFX_TSTOP(twave, 24);
  FFX_TFLUSH();
}

// ---- K8 at fewer than 64 samples per pixel (round 5): the plain forward, box film.  k_render_fwd_pk gives every pixel a wave of its own
// whatever the sample count — at 1 spp one lane of 64 works and the launch costs what it costs at 64 (0.37 ms at 512^2: the dataset loop of
// main.py:138-160 draws its spp from 1..100).  Here a wave owns a compact block of bw x bh pixels with spp_w sample slots each, as
// k_trace_primary_pk does (same layout, same caps: thinner packets mean fewer exact tests per walk and enough waves to fill the GPU); the
// block's primary rays take the block's rectangle to the camera's tile bins (bins_block), shadow packets their samples' bounding box as always.
// Shading is shade_sample_pk's, per sample; a pixel's sum runs over its own spp_w lanes (xor butterfly inside the group).  No adjoint cache,
// no fused adjoint, no reconstruction filter: those keep a pixel per wave.
// RF (ffx_render_fwd_filtered below 33 spp): instead of the pixels' means the wave leaves every pixel's 25 x 4 outgoing sums in the scratch area
// (`img`: [pixel][25][4] floats), as k_render_fwd_pk<..., RF> does — rf_fold_blk below.
template <bool WIDE, int MATM, bool RF = false>
__global__ void __launch_bounds__(PK_BLOCK) __attribute__((amdgpu_waves_per_eu(MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES, MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES)))
    k_render_fwd_blk(ShadeK c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs, uint32_t astride, WideScene ws,
                     const float *__restrict__ albedo, const float *__restrict__ tex, int spp, uint32_t seed_key, int bw_log2, int bh_log2, int blocks_x, int n_blocks,
                     int fp16, void *__restrict__ img, float inv_spp_arg, const float4 *__restrict__ nrec, const float4 *__restrict__ gn) {
  constexpr bool MAT = MATM != 0, TEX = MATM == 2;
  constexpr int MS = MAT ? FFX_MAT_STRIDE : 3;
  constexpr int WSTACK_N = WIDE ? FFX_WSTACK : 1, RF_N = (FFX_RF_FLOATS * 4 + 7) / 8;
  __shared__ __attribute__((aligned(16))) uint2 s_wstack[RF ? (WSTACK_N > RF_N ? WSTACK_N : RF_N) : WSTACK_N]; // (RF: the filter's rows alias the walk's stack)
  const int blk = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (blk >= n_blocks) return; // whole wave
  const int lane = threadIdx.x & 63;
  const int ppw_log2 = bw_log2 + bh_log2;
  const int spp_w = 64 >> ppw_log2;      // sample slots per pixel (>= spp: the host chooses the block so)
  const int pl = lane >> (6 - ppw_log2); // pixel of the block
  const int sl = lane & (spp_w - 1);     // sample slot
  // blocks are enumerated in patches of 8 x 8 blocks (row-major inside a patch, patches row-major over the film: n_blocks counts whole patches), so that
  // the waves the dispatcher starts together work on neighbouring tiles' lists
  const int patches_x = (blocks_x + 7) >> 3, patch = blk >> 6, within = blk & 63;
  const int pby = patch / patches_x, pbx = patch - pby * patches_x;
  const int bxi = (pbx << 3) + (within & 7), byi = (pby << 3) + (within >> 3);
  const int bx0 = bxi << bw_log2, by0 = byi << bh_log2;
  if (bx0 >= c.cam.W || by0 >= c.cam.H) return; // (a patch that overhangs the film)
  const int x = bx0 + (pl & ((1 << bw_log2) - 1)), y = by0 + (pl >> bw_log2);
  const int W = c.cam.W, H = c.cam.H; // (the only direct use of the by-value copy)
  const bool in_img = x < W && y < H;
  const uint32_t pix = (uint32_t)y * (uint32_t)W + (uint32_t)x;
  const bool active = in_img && sl < spp;
  v3 o, d;
  float nt, ft;
  {
    const CamK &cam = kernarg_shade().cam;
    float jx, jy;
    sample_jitter(seed_key, pix * (uint32_t)spp + (uint32_t)sl, jx, jy);
    cam_ray(cam, ((float)x + jx) * cam.inv_w, ((float)y + jy) * cam.inv_h, o, d, nt, ft);
  }
  SampleTerms st;
  shade_sample_pk<WIDE, MATM>(nodes, recs, arecs, astride, ws, s_wstack, active, o, d, nt, ft, st, nrec, gn, bx0, by0, tex, 1 << bw_log2, 1 << bh_log2);
  const ShadeK &ct = kernarg_shade();
  float L[3] = {0.f, 0.f, 0.f};
  if (st.hit) sample_colour(ct, st, tex, TEX ? st.base : mat_table(ct) + MS * st.shape, MAT, L);
  float c0 = L[0], c1 = L[1], c2 = L[2];
  if constexpr (RF) {
    float jx, jy, gx[5], gy[5];
    sample_jitter(seed_key, pix * (uint32_t)spp + (uint32_t)sl, jx, jy);
    rf_weights(ct.rf, jx, gx);
    rf_weights(ct.rf, jy, gy);
    rf_fold_blk(reinterpret_cast<float *>(s_wstack), lane, gx, gy, c0, c1, c2, active ? 1.f : 0.f, ppw_log2, bw_log2, bx0, by0, W, H, reinterpret_cast<float *>(img));
    return;
  }
  // the pixel's samples sit in spp_w neighbouring lanes: a butterfly inside the group, nearest partners first — the tree of k_render_fwd_pk's DPP
  // chain (pairs, quads, half rows, rows, rows of rows; its lanes beyond the sample count add zeros), so the two kernels store the same bits
  for (int m = 1; m < spp_w; m <<= 1) {
    c0 += __shfl_xor(c0, m, 64);
    c1 += __shfl_xor(c1, m, 64);
    c2 += __shfl_xor(c2, m, 64);
  }
  if (in_img && sl == 0) {
    const size_t o3 = (size_t)pix * 3;
    if (fp16 & 1) {
      _Float16 *p = (_Float16 *)img;
      p[o3] = (_Float16)(c0 * inv_spp_arg);
      p[o3 + 1] = (_Float16)(c1 * inv_spp_arg);
      p[o3 + 2] = (_Float16)(c2 * inv_spp_arg);
    } else {
      float *p = (float *)img;
      p[o3] = c0 * inv_spp_arg;
      p[o3 + 1] = c1 * inv_spp_arg;
      p[o3 + 2] = c2 * inv_spp_arg;
    }
  }
}


// Deterministic accumulation (ffx_render_bwd_det, include/ffx.h): float atomics make gtex depend on the order in which the samples' taps arrive
// (reassociation: ~1e-7 relative, different from run to run).  INTEGER additions commute: mode 1 finds the largest |tap value| of the launch
// (atomicMax on the float's bits — order-independent), the host derives a power-of-two scale from it, mode 2 adds llrint(value * scale) to a
// 64-bit fixed-point accumulator per texel (global_atomic_add_x2) and k_det_finish converts back — bitwise the same gtex whatever the
// dispatch order, the number of XCDs or the rank count, at a resolution of 2^-(62 - b) of the largest tap, b = bits of the launch's tap count: 2^-36 at 512 x 512 x 64 spp (float32 carries 2^-24).
struct DetK { int mode; float scale; unsigned long long *fix; unsigned int *vmax; };
// one of the two passes alone (ffx_render_bwd_det_part, ABI 9): part 1 = the largest tap into *vmax (atomicMax: accumulates over calls), part 2 = the
// fixed-point sums at the caller's scale 2^scale_log2 into fix[] (accumulate over calls — over the scene samples of a step, over ranks)
struct DetPart { int part; int scale_log2; unsigned long long *fix; unsigned int *vmax; };
// the scale of a deterministic accumulation: vmax < 2^e, |sum| <= n_taps x vmax < 2^(b + e) with b = bits of the tap count; 2^(62 - b - e) keeps
// every sum below 2^62 and one unit at 2^-(62 - b) of the largest tap.  INT_MIN: nothing lit (vmax = 0) or a non-finite tap
static int det_scale_log2(uint32_t vmax_bits, unsigned long long n_taps) {
  float vmax;
  memcpy(&vmax, &vmax_bits, 4);
  if (!(vmax > 0.f) || !(vmax < 3.0e38f)) return INT_MIN;
  int e;
  frexpf(vmax, &e);
  int b = 0;
  for (unsigned long long ns = n_taps > 0 ? n_taps : 1; ns > 0; ns >>= 1) ++b;
  const int sh = 62 - b - e;
  return sh > 126 ? 126 : (sh < -126 ? -126 : sh);
}
__device__ __forceinline__ void det_emit(const DetK &det, float *__restrict__ gtex, size_t t, float v) {
  if (det.mode == 0) { atomicAdd(gtex + t, v); return; }
  if (det.mode == 1) { if (v != 0.f) atomicMax(det.vmax, __float_as_uint(fabsf(v))); return; }
  if (v != 0.f) atomicAdd(det.fix + t, (unsigned long long)__double2ll_rn((double)v * (double)det.scale));
}
__global__ void __launch_bounds__(256) k_det_finish(const unsigned long long *__restrict__ fix, float inv_scale, long n, float *__restrict__ gtex) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) gtex[t] += (float)((double)(long long)fix[t] * (double)inv_scale); // (gtex is ACCUMULATED into, as by every adjoint)
}
// RF (ffx_render_bwd_filtered): `gimg` is then G = gimg / weight as float4 per pixel (k_rf_gather) and a sample's radiance receives
// sum over its 5x5 window of  w_n G[pixel + n]  — the transpose of the filter — in place of gimg[pixel] / spp.
// (R = 1 stays in the template head as in k_render_fwd_pk: the instance names k_render_bwd_pk<1, ...> are what profiles and tools key on)
template <int R, bool WIDE, int MATM, bool RF = false>
__global__ void __launch_bounds__(PK_BLOCK) __attribute__((amdgpu_waves_per_eu(MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES, MATM ? FFX_PK_MAT_WAVES : FFX_PK1_WAVES)))
    k_render_bwd_pk(ShadeK c, const BvhNode *__restrict__ nodes, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs, uint32_t astride,
                    WideScene ws, const float *__restrict__ albedo, int spp, uint32_t seed_key, int tiles_x, int n_tiles, int remap,
                    const float *__restrict__ gimg, float *__restrict__ gtex, const float4 *__restrict__ nrec, const float4 *__restrict__ gn, DetK det) {
  constexpr bool MAT = MATM != 0, TEX = MATM == 2;
  __shared__ uint2 s_wstack[WIDE ? FFX_WSTACK : 1];
  const int tile = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x, remap) * (blockDim.x >> 6) + (threadIdx.x >> 6)); // wave-uniform: say so
  const int lane = threadIdx.x & 63;
  const int W = c.cam.W, H = c.cam.H; // (the only direct use of the by-value copy; see kernarg_shade)
  const float inv_spp = RF ? 1.0f : 1.0f / (float)spp; // (RF: the normalisation is the weight inside G)
  const int passes = (spp + 63) >> 6;
  static_assert(R == 1, "one ray per lane");
  for (int sub = 0; sub < 4; ++sub) { // the tile's four pixels
    int px[R], py[R];
    packet_pixels<R>(tile, tiles_x, sub, px, py);
    bool live[R], any_live = false;
    uint32_t pix[R];
    float g[R][3];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live[r] = tile < n_tiles && px[r] < W && py[r] < H;
      pix[r] = live[r] ? (uint32_t)py[r] * (uint32_t)W + (uint32_t)px[r] : 0u;
      g[r][0] = g[r][1] = g[r][2] = 0.f;
      if constexpr (RF) {
        // lane n < 25 looks at window pixel n: the pixel is skipped when no pixel of its window carries a gradient
        const float4 gw = rf_window_g(reinterpret_cast<const float4 *>(gimg), px[r], py[r], W, H, lane, live[r]);
        live[r] = wballot(gw.x != 0.f || gw.y != 0.f || gw.z != 0.f) != 0ull;
      } else {
      if (live[r]) { g[r][0] = gimg[(size_t)pix[r] * 3]; g[r][1] = gimg[(size_t)pix[r] * 3 + 1]; g[r][2] = gimg[(size_t)pix[r] * 3 + 2]; }
      live[r] = live[r] && !(g[r][0] == 0.f && g[r][1] == 0.f && g[r][2] == 0.f);
      }
      any_live |= live[r];
    }
    if (wballot(any_live) == 0ull) continue; // wave-uniform
    for (int pass = 0; pass < passes; ++pass) {
      const int s = pass * 64 + lane;
      bool active[R];
      v3 o[R], d[R];
      float nt[R], ft[R];
      const CamK &cam = kernarg_shade().cam; // phase: ray generation
#pragma unroll
      for (int r = 0; r < R; ++r) {
        active[r] = live[r] && s < spp;
        uint32_t idx = pix[r] * (uint32_t)spp + (uint32_t)s;
        float jx, jy;
        sample_jitter(seed_key, idx, jx, jy);
        cam_ray(cam, ((float)px[r] + jx) * cam.inv_w, ((float)py[r] + jy) * cam.inv_h, o[r], d[r], nt[r], ft[r]);
      }
      SampleTerms st[R];
      shade_sample_pk<WIDE, MATM>(nodes, recs, arecs, astride, ws, s_wstack, active[0], o[0], d[0], nt[0], ft[0], st[0], nrec, gn, px[0], py[0]);
      const ShadeK &ct = kernarg_shade(); // phase: scatter into the texture gradient
      const int tc = ct.tc;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if constexpr (RF) {
          // every lane's sample gathers its own gradient through the filter's weights: window pixel n's G sits in lane n (re-read: cached),
          // broadcast with readlane and weighted per lane — window order, fused multiply-adds, as the oracle
          const float4 gw = rf_window_g(reinterpret_cast<const float4 *>(gimg), px[r], py[r], W, H, lane, live[r]);
          const float gwin[3] = {gw.x, gw.y, gw.z};
          float jx, jy;
          sample_jitter(seed_key, pix[r] * (uint32_t)spp + (uint32_t)s, jx, jy);
          sample_adjoint<true>(ct.rf, jx, jy, gwin, g[r]);
        }
        if (!st[r].hit || !st[r].has_proj) continue;
        const float *alb = TEX ? st[r].base : mat_table(ct) + (MAT ? FFX_MAT_STRIDE : 3) * st[r].shape;
        sample_scatter(sample_taps(st[r], ct.tw, tc), tc, g[r], alb, ct.p_color, st[r].proj_fac, MAT ? st[r].proj_fac_b : 0.f, inv_spp, false,
                       [&](size_t o, int ch, float v) { det_emit(det, gtex, o + ch, v); });
      }
    }
  }
}

// K9 from the adjoint cache.  Part 1: 32 lanes per pixel slot — lane e < 25 scatters footprint weight e scaled by
// the pixel's  gimg . albedo[shape] (. colour) / spp  with one global float atomic (a lit pixel touches ~16
// texels: ~0.8 M atomics per 512x512 render instead of 4 x 16.8 M sample taps).  Part 2 (the blocks past the
// pixel slots): one lane per stray sample record, four taps each.
struct BwdP { int tw, th, tc, spp; float color[3]; float inv_spp; int W, H; int ms; size_t off_foot_b; // ms: floats per material row (3 / FFX_MAT_STRIDE)
              const void *img; int img_fp16; float *dot_out; int dot_slots; // optional: sum(dot_out[0 .. dot_slots)) += <gimg, img> (the value of a linear loss whose gradient gimg is)
              const float *l1_tgt; float l1_gs, l1_vs; // optional (ffx_render_bwd_cached_l1): gimg = the gradient of l1_vs * sum |img - l1_tgt|, formed per pixel
              const float *mats; int mat_inline; float mat_h[FFX_MAX_MAT_H]; }; // the material table: the caller's device array or (ffx_scene_desc.mat_h) this kernel argument
__device__ __forceinline__ const float *mat_table(const BwdP &k) { return k.mat_inline ? k.mat_h : k.mats; }
// the loss gradient at a pixel: the caller's gimg, or (l1_tgt) the L1 loss's own — sign(img - target) * weight / n, the arithmetic of k_l1_partial
// (ffx_l1_value_grad) — with the pixel's |img - target| for the loss value
__device__ __forceinline__ void k9_g(const BwdP &p, const float *__restrict__ gimg, long pixel, float &g0, float &g1, float &g2, float *absum = nullptr) {
  if (p.l1_tgt) {
    const float *q = (const float *)p.img + pixel * 3, *t = p.l1_tgt + pixel * 3;
    const float d0 = q[0] - t[0], d1 = q[1] - t[1], d2 = q[2] - t[2];
    g0 = d0 > 0.f ? p.l1_gs : (d0 < 0.f ? -p.l1_gs : 0.f);
    g1 = d1 > 0.f ? p.l1_gs : (d1 < 0.f ? -p.l1_gs : 0.f);
    g2 = d2 > 0.f ? p.l1_gs : (d2 < 0.f ? -p.l1_gs : 0.f);
    if (absum) *absum = (fabsf(d0) + fabsf(d1)) + fabsf(d2);
    return;
  }
  g0 = gimg[pixel * 3]; g1 = gimg[pixel * 3 + 1]; g2 = gimg[pixel * 3 + 2];
}
// <g, img> of a pixel with gradient g, for either film format
__device__ __forceinline__ float k9_pixel_dot(const BwdP &p, long pixel, float g0, float g1, float g2) {
  if (p.img_fp16) {
    const _Float16 *q = (const _Float16 *)p.img + pixel * 3;
    return g0 * (float)q[0] + g1 * (float)q[1] + g2 * (float)q[2];
  }
  const float *q = (const float *)p.img + pixel * 3;
  return g0 * q[0] + g1 * q[1] + g2 * q[2];
}

// the stray records of the adjoint cache: thread i replays record i (four bilinear taps each)
__device__ __forceinline__ void k9_stray(const char *__restrict__ cache, long n_pix, uint32_t i, const BwdP &p, const float *__restrict__ gimg,
                                         const float *__restrict__ albedo, float *__restrict__ gtex) {
  const CacheHdr *hdr = reinterpret_cast<const CacheHdr *>(cache);
  // the forward pass ran out of stray records: the gradient of `dropped` samples is missing.  A wrong gradient must not
  // look like a right one: poison gtex (NaN) — ffx_render_cache_status tells the host why, which then re-traces
  // (functional._Render.backward) or raises (optim.PatternOptimizer)
  if (i == 0 && hdr->dropped != 0u) atomicAdd(gtex, __uint_as_float(0x7fc00000u));
  const uint32_t n = min(hdr->n_stray, hdr->cap_stray);
  if (i >= n) return;
  const CacheStray rec = reinterpret_cast<const CacheStray *>(cache + cache_off_arena((size_t)n_pix))[i];
  const long pixel = rec.pix;
  // (sample_scatter's values with zero values skipped, written out: as a call it changes the register count of k_render_bwd_cached_tiled16, whose tail this is)
  float g0, g1, g2;
  k9_g(p, gimg, pixel, g0, g1, g2);
  const int ix0 = (int)(rec.xy_shape & 0xfffu) - 1, iy0 = (int)((rec.xy_shape >> 12) & 0xfffu) - 1, shape = (int)(rec.xy_shape >> 24);
  const int x0 = clampi(ix0, 0, p.tw - 1), x1 = clampi(ix0 + 1, 0, p.tw - 1), y0 = clampi(iy0, 0, p.th - 1), y1 = clampi(iy0 + 1, 0, p.th - 1);
  const float wx0 = 1.0f - rec.ax, wx1 = rec.ax, wy0 = 1.0f - rec.ay, wy1 = rec.ay;
  const float *alb = albedo + p.ms * shape;
  const float fac_b = p.ms == 3 ? 0.f : rec.fac_b;
  if (p.tc == 1) {
    float ws = (g0 * alb[0] * p.color[0] + g1 * alb[1] * p.color[1] + g2 * alb[2] * p.color[2]) * rec.fac * p.inv_spp;
    if (fac_b != 0.f) ws += (g0 * p.color[0] + g1 * p.color[1] + g2 * p.color[2]) * fac_b * p.inv_spp;
    if (ws == 0.f) return;
    atomicAdd(gtex + (size_t)y0 * p.tw + x0, ws * wy0 * wx0);
    atomicAdd(gtex + (size_t)y0 * p.tw + x1, ws * wy0 * wx1);
    atomicAdd(gtex + (size_t)y1 * p.tw + x0, ws * wy1 * wx0);
    atomicAdd(gtex + (size_t)y1 * p.tw + x1, ws * wy1 * wx1);
  } else {
    const size_t o00 = ((size_t)y0 * p.tw + x0) * 3, o01 = ((size_t)y0 * p.tw + x1) * 3;
    const size_t o10 = ((size_t)y1 * p.tw + x0) * 3, o11 = ((size_t)y1 * p.tw + x1) * 3;
    const float gg[3] = {g0, g1, g2};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float ws = gg[ch] * alb[ch] * rec.fac * p.inv_spp;
      if (fac_b != 0.f) ws += gg[ch] * fac_b * p.inv_spp;
      if (ws == 0.f) continue;
      atomicAdd(gtex + o00 + ch, ws * wy0 * wx0);
      atomicAdd(gtex + o01 + ch, ws * wy0 * wx1);
      atomicAdd(gtex + o10 + ch, ws * wy1 * wx0);
      atomicAdd(gtex + o11 + ch, ws * wy1 * wx1);
    }
  }
}

// K9 for 1-channel textures, tiled: a workgroup owns a 16x16-pixel block of the image.  Neighbouring pixels land on neighbouring texels, so their
// 5x5 footprints overlap heavily: one global float atomic per footprint element was bound by contention (~900 k of them into a 500^2 texture).
// Here the block's footprints are summed in a 48x48-texel LDS tile anchored at the smallest window origin of its lit pixels, and every touched
// texel gets ONE global atomic; footprint elements that fall outside the tile (a block on a depth discontinuity) go to memory directly.
// Summation order inside a block is not fixed (LDS float atomics) — like the global atomics it replaces.
// Most of K9's time is not the scatter but finding out that there is nothing to scatter: 96 % of the pixels of a dot pattern's render are unlit.
// Every lane owns a pixel in pass 1 — header, <gimg, img>, a ballot — and a workgroup without a lit pixel ends after ONE round of
// independent loads; the lit pixels are compacted into a list that pass 2 walks 8 at a time (32 lanes per pixel, 25 footprint weights).
#define K9_TILE16 48
__global__ void __launch_bounds__(256)
    k_render_bwd_cached_tiled16(BwdP p_by_value, const char *__restrict__ cache, int blocks_x, int tile_blocks, const float *__restrict__ gimg,
                                float *__restrict__ gtex) {
  __shared__ float s_tile[K9_TILE16 * K9_TILE16];
  __shared__ int s_ox, s_oy, s_n;
  // the lit pixels of the block, compacted: pixel (lane of pass 1), window origin, and the two per-pixel factors of its footprints
  __shared__ unsigned short s_px[256];
  __shared__ int s_xy[256];
  __shared__ float s_ws[256], s_wsb[256];
  const BwdP &p = kernarg_first<BwdP>();
  const float *albedo = mat_table(p);
  const long n_pix = (long)p.W * p.H;
  if ((int)blockIdx.x >= tile_blocks) { // the tail of the grid replays the stray records
    k9_stray(cache, n_pix, (uint32_t)((int)blockIdx.x - tile_blocks) * 256u + threadIdx.x, p, gimg, albedo, gtex);
    return;
  }
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const CachePix *hdrs = reinterpret_cast<const CachePix *>(cache + 64);
  const CacheFoot *foots = reinterpret_cast<const CacheFoot *>(cache + cache_off_foot((size_t)n_pix));
  const CacheFoot *foots_b = reinterpret_cast<const CacheFoot *>(cache + p.off_foot_b);
  if (threadIdx.x == 0) { s_ox = 0x7fffffff; s_oy = 0x7fffffff; s_n = 0; }
  __syncthreads();
  // pass 1: one lane per pixel of the 16x16 block
  {
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = bx * 16 + lx, y = by * 16 + ly;
    const bool in = x < p.W && y < p.H;
    const long pixel = (long)y * p.W + x;
    CachePix hp;
    hp.lit = 0;
    if (in) hp = hdrs[pixel];
    const bool lit = in && hp.lit;
    float g[3] = {0.f, 0.f, 0.f}, l1_abs = 0.f;
    if (in && (p.dot_out || lit)) k9_g(p, gimg, pixel, g[0], g[1], g[2], &l1_abs);
    if (p.l1_tgt) { // the L1 loss's value: this wave's 4 rows of |img - target|, one add into the block's own slot (summed by the gradient launch)
      const float d = wave_sum64(l1_abs);
      if ((threadIdx.x & 63) == 0 && d != 0.f) atomicAdd(p.dot_out + (int)blockIdx.x % p.dot_slots, d * p.l1_vs);
    }
    const wmask lm = wballot(lit);
    if (lm != 0ull) { // (per wave) origin of the tile and the wave's share of the list
      int base = 0;
      if ((threadIdx.x & 63) == 0) base = atomicAdd(&s_n, wpop(lm));
      base = __builtin_amdgcn_readfirstlane(base);
      if (lit) {
        atomicMin(&s_ox, (int)hp.x0);
        atomicMin(&s_oy, (int)hp.y0);
        const float *alb = albedo + p.ms * (int)hp.shape;
        const int k = base + (int)mbcnt64(lm);
        s_px[k] = (unsigned short)threadIdx.x;
        s_xy[k] = (int)hp.x0 | ((int)hp.y0 << 16);
        s_ws[k] = g_alb_colour(g, alb, p.color) * p.inv_spp;
        s_wsb[k] = g_colour(g, p.color) * p.inv_spp;
      }
    }
    if (p.dot_out && !p.l1_tgt) { // <gimg, img> of this wave's 4 rows: one add into the block's own slot (ffx_render_dot_slots)
      const float d = wave_sum64(in ? k9_pixel_dot(p, pixel, g[0], g[1], g[2]) : 0.f);
      if ((threadIdx.x & 63) == 0 && d != 0.f) atomicAdd(p.dot_out + (int)blockIdx.x % p.dot_slots, d);
    }
  }
  __syncthreads();
  const int n_lit = s_n;
  if (n_lit == 0) return; // (uniform: nothing lit in this block)
  for (int i = threadIdx.x; i < K9_TILE16 * K9_TILE16; i += 256) s_tile[i] = 0.f;
  __syncthreads();
  const int ox = s_ox, oy = s_oy;
  // pass 2: 32 lanes per lit pixel (25 footprint weights), 8 pixels side by side and four of those rounds in flight (the block of a
  // laser dot holds ~140 lit pixels: walked one round at a time its dependent loads were the tail of the whole launch)
  const int e = threadIdx.x & 31;
  const bool has_b = p.ms != 3;
  for (int it0 = threadIdx.x >> 5; it0 < n_lit; it0 += 32) {
    float w[4], wb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + 8 * u;
      w[u] = 0.f; wb[u] = 0.f;
      if (it < n_lit && e < 25) {
        const int pl = (int)s_px[it];
        const long pixel = (long)(by * 16 + (pl >> 4)) * p.W + (bx * 16 + (pl & 15));
        w[u] = foots[pixel].w[e];
        if (has_b) wb[u] = foots_b[pixel].w[e];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + 8 * u;
      if (it >= n_lit || (w[u] == 0.f && wb[u] == 0.f)) continue;
      float val = s_ws[it] * w[u]; // (foot_value_1ch, written out: s_wsb[it] is read only where wb != 0)
      if (wb[u] != 0.f) val += s_wsb[it] * wb[u];
      if (val == 0.f) continue;
      const int xy = s_xy[it];
      const int tx = (xy & 0xffff) + e % 5, ty = (xy >> 16) + e / 5;
      const int lx = tx - ox, ly = ty - oy;
      if (lx < K9_TILE16 && ly < K9_TILE16) atomicAdd(&s_tile[ly * K9_TILE16 + lx], val); // (lx, ly >= 0 by construction)
      else atomicAdd(gtex + (size_t)ty * p.tw + tx, val);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K9_TILE16 * K9_TILE16; i += 256) {
    const float v = s_tile[i];
    if (v != 0.f) atomicAdd(gtex + (size_t)(oy + i / K9_TILE16) * p.tw + (ox + i % K9_TILE16), v);
  }
}

__global__ void __launch_bounds__(256)
    k_render_bwd_cached(BwdP p_by_value, const char *__restrict__ cache, long n_pix, int slot_blocks, const float *__restrict__ gimg, float *__restrict__ gtex) {
  const BwdP &p = kernarg_first<BwdP>();
  const float *albedo = mat_table(p);
  if ((int)blockIdx.x < slot_blocks) {
    const long pixel = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int e = threadIdx.x & 31;
    if (p.dot_out) { // <gimg, img> of the block's 8 pixels: lanes 0..7 of wave 0, one atomic
      __shared__ float s_d[8];
      if (e == 0) s_d[threadIdx.x >> 5] = pixel < n_pix ? k9_pixel_dot(p, pixel, gimg[pixel * 3], gimg[pixel * 3 + 1], gimg[pixel * 3 + 2]) : 0.f;
      __syncthreads();
      if (threadIdx.x == 0) {
        const float d = ((s_d[0] + s_d[1]) + (s_d[2] + s_d[3])) + ((s_d[4] + s_d[5]) + (s_d[6] + s_d[7]));
        if (d != 0.f) atomicAdd(p.dot_out + (int)blockIdx.x % p.dot_slots, d);
      }
    }
    if (pixel >= n_pix) return;
    const CachePix hp = reinterpret_cast<const CachePix *>(cache + 64)[pixel];
    if (!hp.lit || e >= 25) return;
    const float w = reinterpret_cast<const CacheFoot *>(cache + cache_off_foot((size_t)n_pix))[pixel].w[e];
    const float wb = p.ms == 3 ? 0.f : reinterpret_cast<const CacheFoot *>(cache + p.off_foot_b)[pixel].w[e];
    if (w == 0.f && wb == 0.f) return;
    const float g[3] = {gimg[pixel * 3], gimg[pixel * 3 + 1], gimg[pixel * 3 + 2]};
    const float *alb = albedo + p.ms * (int)hp.shape;
    const int x = (int)hp.x0 + e % 5, y = (int)hp.y0 + e / 5;
    if (p.tc == 1) {
      const float val = foot_value_1ch(g_alb_colour(g, alb, p.color) * p.inv_spp, g_colour(g, p.color) * p.inv_spp, w, wb);
      if (val != 0.f) atomicAdd(gtex + (size_t)y * p.tw + x, val);
    } else {
      float *t = gtex + ((size_t)y * p.tw + x) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        if (g[ch] != 0.f) atomicAdd(t + ch, foot_value_3ch(g[ch], alb[ch], p.inv_spp, w, wb));
    }
    return;
  }
  k9_stray(cache, n_pix, (uint32_t)(blockIdx.x - slot_blocks) * 256u + threadIdx.x, p, gimg, albedo, gtex);
}

// K9 of the filtered film's cache (ffx_render_bwd_cached_filtered; rfc_off_* above).  An ITEM is one lit 64-sample pass of one pixel: the
// lanes take its 64 records (one coalesced 1 KB load), their ten filter weights from the jitter (the forward's hash), the pixel's window of
// G = gimg / weight (lanes 0..24 load a window pixel each, broadcast by v_readlane), the sample's own gradient sum_n w_n G[pixel + n]
// (sample_adjoint); the wave then sums its samples' taps per texel of the pixel's 5x5 texel window
// (25 DPP reductions) and 25 lanes add one value each to gtex — no per-sample atomics (samples outside the window: their four taps directly).
// ~800 VALU instructions per item, and the items of a dot pattern's render sit in ~500 of the film's 4096 8x8-pixel blocks: as ONE workgroup
// per block (first version: 16x16-pixel blocks, then 8x8, four to sixteen waves, an LDS tile per block) a block's ~64 items ran on ONE compute
// unit — 0.16 / 0.09 / 0.065 ms with 250 of 256 CUs idle.  Now every block is served by K9F_SUB independent ONE-WAVE workgroups (the
// dispatcher deals them to different CUs and XCDs): each reads the block's 64 pixel headers itself (512 bytes, L2) and takes every
// K9F_SUB-th lit item.  A block without lit pixels costs its waves one load.  3-channel textures: twelve direct atomics per sample.
struct BwdF { int tw, th, tc, spp; float color[3]; RfC rf; int W, H; int ms, n_shapes; uint32_t seed_key; size_t off_wsum, off_recs, off_facb;
              const float *mats; int mat_inline; float mat_h[FFX_MAX_MAT_H]; };
__device__ __forceinline__ const float *mat_table(const BwdF &k) { return k.mat_inline ? k.mat_h : k.mats; }
#define K9F_BLOCK 8 // pixels per side of a block
#ifndef K9F_SUB
#define K9F_SUB 16 // one-wave workgroups per block (a wave's items are a serial chain of ~1000 instructions each: 4 / 8 / 16 waves per block = 0.102 / 0.055 / 0.035 ms)
#endif
__global__ void __launch_bounds__(64)
    k_render_bwd_cached_filtered(BwdF p_by_value, const char *__restrict__ cache, int blocks_x, const float *__restrict__ gimg, float *__restrict__ gtex) {
  const BwdF &p = kernarg_first<BwdF>();
  const float *albedo = mat_table(p);
  const int blk = (int)blockIdx.x / K9F_SUB, sub = (int)blockIdx.x % K9F_SUB;
  const int bx = blk % blocks_x, by = blk / blocks_x;
  const CachePix *hdrs = reinterpret_cast<const CachePix *>(cache + 64);
  const float *wsum = reinterpret_cast<const float *>(cache + p.off_wsum);
  const uint4 *recs = reinterpret_cast<const uint4 *>(cache + p.off_recs);
  const float *facb = reinterpret_cast<const float *>(cache + p.off_facb);
  const int lane = threadIdx.x;
  uint32_t mask = 0u; // the lane's pixel: its lit passes, the arena block of the first of them, that pass
  uint32_t hfirst = 0u;
  int hpass = 0;
  {
    const int x = bx * K9F_BLOCK + lane % K9F_BLOCK, y = by * K9F_BLOCK + lane / K9F_BLOCK;
    if (x < p.W && y < p.H) {
      const CachePix hp = hdrs[(long)y * p.W + x];
      mask = hp.lit;
      hfirst = (uint32_t)(uint16_t)hp.x0 | ((uint32_t)(uint16_t)hp.y0 << 16);
      hpass = hp.shape;
    }
  }
  // (a forward that found the arena full left pixels without records: the gradient would have holes that look like values — poison it, NaN;
  // ffx_render_cache_status tells the host why, which re-traces (functional._Render.backward) or raises (optim.PatternOptimizer))
  if (blockIdx.x == 0 && lane == 0 && reinterpret_cast<const CacheHdr *>(cache)->dropped != 0u) atomicAdd(gtex, __uint_as_float(0x7fc00000u));
  if (wballot(mask != 0u) == 0ull) return; // (nothing lit in this block: 96 % of a dot pattern's film ends here)
  const int passes = (p.spp + 63) >> 6;
  const bool tiled = p.tc == 1, mat = p.ms != 3;
  // this wave's items: rank r of the block's lit (pass, pixel) pairs in (pass, pixel) order belongs to wave r % K9F_SUB.  State of the walk: the
  // pass, the lit pixels of that pass not yet visited, the rank of the next one — all wave-uniform
  int it_pass = 0, it_rank = 0;
  wmask it_left = wballot((mask & 1u) != 0u);
  auto next_item = [&](int &pl, int &pass) -> bool { // -> this wave's next item, false when the block is exhausted
    for (;;) {
      while (it_left == 0ull) {
        if (++it_pass >= passes) return false;
        it_left = wballot(((mask >> it_pass) & 1u) != 0u);
      }
      const int l = wff1(it_left);
      it_left &= it_left - 1ull;
      if ((it_rank++ % K9F_SUB) == sub) { pl = l; pass = it_pass; return true; }
    }
  };
  // an item's inputs: the lane's record (+ fac_b) and, in lanes 0..24, gimg and the weight of one pixel of the window.  Loaded ONE ITEM AHEAD
  struct Item { uint4 rec; float fb, q0, q1, q2, qw; int px, py; uint32_t sidx; bool ok; };
  auto fetch = [&](Item &o) {
    o.rec = make_uint4(0u, 0u, 0u, 0u); o.fb = 0.f; o.q0 = o.q1 = o.q2 = 0.f; o.qw = 0.f; o.px = o.py = 0; o.sidx = 0u;
    int pl = 0, pass = 0;
    o.ok = next_item(pl, pass);
    if (!o.ok) return;
    o.px = bx * K9F_BLOCK + pl % K9F_BLOCK; o.py = by * K9F_BLOCK + pl / K9F_BLOCK;
    const long pixel = (long)o.py * p.W + o.px;
    const int s = pass * 64 + lane;
    o.sidx = (uint32_t)pixel * (uint32_t)p.spp + (uint32_t)s;
    if (s < p.spp) {
      const uint32_t blk_ = (uint32_t)__builtin_amdgcn_readlane((int)hfirst, pl) + (uint32_t)(pass - __builtin_amdgcn_readlane(hpass, pl));
      o.rec = recs[(size_t)blk_ * 64u + (size_t)lane];
      if (mat) o.fb = facb[(size_t)blk_ * 64u + (size_t)lane];
    }
    const int wb = (lane * 13) >> 6, wa = lane - 5 * wb; // lane / 5, lane % 5 for lane < 25
    const int tx = o.px + wa - 2, ty = o.py + wb - 2;
    if (lane < 25 && tx >= 0 && tx < p.W && ty >= 0 && ty < p.H) {
      const long q = (long)ty * p.W + tx;
      o.qw = wsum[q];
      o.q0 = gimg[q * 3]; o.q1 = gimg[q * 3 + 1]; o.q2 = gimg[q * 3 + 2];
    }
  };
  Item cur, nxt;
  fetch(cur);
  while (cur.ok) { // (wave-uniform loop)
    fetch(nxt);
    const uint4 rec = cur.rec;
    const float fb = cur.fb;
    const float fac = __uint_as_float(rec.w);
    const bool lit = fac != 0.f || fb != 0.f;
    // the pixel's window of G = gimg / weight (lanes 0..24), zero outside the film
    const bool gok = cur.qw > 0.f;
    const float g0 = gok ? cur.q0 / cur.qw : 0.f, g1 = gok ? cur.q1 / cur.qw : 0.f, g2 = gok ? cur.q2 / cur.qw : 0.f;
    const float gwin[3] = {g0, g1, g2};
    float jx, jy, a[3];
    sample_jitter(p.seed_key, cur.sidx, jx, jy);
    sample_adjoint<true>(p.rf, jx, jy, gwin, a);
    const int ubx = (int)(rec.x & 0xfffu) - 1, uby = (int)((rec.x >> 12) & 0xfffu) - 1, shape = (int)(rec.x >> 24);
    const int x0 = clampi(ubx, 0, p.tw - 1), x1 = clampi(ubx + 1, 0, p.tw - 1), y0 = clampi(uby, 0, p.th - 1), y1 = clampi(uby + 1, 0, p.th - 1);
    const float ax = __uint_as_float(rec.y), ay = __uint_as_float(rec.z);
    const float wx0 = 1.0f - ax, wx1 = ax, wy0 = 1.0f - ay, wy1 = ay;
    const float *alb = albedo + p.ms * (lit ? shape : 0);
    if (tiled) {
      float pf = 0.f;
      if (lit) pf = tap_value_1ch(a, alb, p.color, fac, fb, 1.0f); // (the weight inside G normalises)
      const bool on = lit && pf != 0.f;
      if (wballot(on) != 0ull) { // (wave-uniform)
        const int fox = (int)wave_reduce_nn<false>(on ? (uint32_t)x0 : 0xffffffffu), foy = (int)wave_reduce_nn<false>(on ? (uint32_t)y0 : 0xffffffffu);
        const bool in_win = on && x1 - fox <= 4 && y1 - foy <= 4;
        const int cx0 = x0 - fox, cx1 = x1 - fox, cy0 = y0 - foy, cy1 = y1 - foy;
        float cw[5], rw[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          cw[c] = in_win ? ((cx0 == c ? wx0 : 0.f) + (cx1 == c ? wx1 : 0.f)) : 0.f; // (a clamped border tap may name the same texel twice: both weights count)
          rw[c] = in_win ? pf * ((cy0 == c ? wy0 : 0.f) + (cy1 == c ? wy1 : 0.f)) : 0.f;
        }
        float v[27];
#pragma unroll
        for (int n = 0; n < 25; ++n) v[n] = rw[n / 5] * cw[n % 5];
        v[25] = v[26] = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) asm(FFX_R3_ALL("v_add_f32_dpp") : "+v"(v[3 * k]), "+v"(v[3 * k + 1]), "+v"(v[3 * k + 2])); // (the wave's sums in lane 63)
        float mine = 0.f;
#pragma unroll
        for (int n = 0; n < 25; ++n) {
          const float sn = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v[n]), 63));
          if (lane == n) mine = sn;
        }
        if (mine != 0.f) { // (lanes 0..24: one texel each)
          const int ey = (lane * 13) >> 6, ex = lane - 5 * ey;
          atomicAdd(gtex + (size_t)(foy + ey) * p.tw + (fox + ex), mine);
        }
        // a sample outside its pixel's window (depth discontinuities, grazing surfaces: ~0.1 %): its four taps directly
        if (on && !in_win) taps_scatter(make_taps(x0, x1, y0, y1, wx0, wx1, wy0, wy1, p.tw, 1), 0, pf, AtomicInto{gtex});
      }
    } else if (lit) { // 3-channel textures: twelve direct atomics per sample
      sample_scatter(make_taps(x0, x1, y0, y1, wx0, wx1, wy0, wy1, p.tw, 3), 3, a, alb, p.color, fac, fb, 1.0f, true, AtomicInto{gtex});
    }
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------ path integrator
// max_depth > 2 (include/ffx.h FFX_RENDER_PATH): Mitsuba's `path` with cosine-weighted bounces and next-event estimation to the two delta emitters
// at every vertex.  Per-lane kernels: one wave = one pixel, lane l takes samples l, l + 64, ... (the layout rf_fold needs), one lane walks one path
// with shade_sample's arbitrary-ray form.  The adjoint replays the same paths: the texture enters through the emitters' terms only.
// The counter-based stream of the path's random numbers: vertex v (1 = the primary hit), dimension dim (0, 1: the bounce direction, 2: roulette)
__device__ __forceinline__ float path_u(uint32_t path_key, uint32_t idx, int v, int dim) {
  const uint32_t r = hash32(hash32(idx ^ path_key) + (uint32_t)(4 * v + dim));
  return (float)(r >> 8) * (1.0f / 16777216.0f);
}
// cosine-weighted direction about the unit normal n: (sqrt(u0) cos(2 pi u1), sqrt(u0) sin(2 pi u1), sqrt(1 - u0)) in the frame of Duff et al. 2017
__device__ __forceinline__ v3 cosine_dir(v3 n, float u0, float u1) {
  const float sg = copysignf(1.0f, n.z), a = -1.0f / (sg + n.z), b = n.x * n.y * a;
  const v3 s = V3(1.0f + sg * n.x * n.x * a, sg * b, -sg * n.x), t = V3(b, sg + n.y * n.y * a, -n.y);
  const float r = sqrtf(u0), ph = 2.0f * FFX_PI_F * u1, z = sqrtf(fmaxf(1.0f - u0, 0.f));
  const float x = r * cosf(ph), y = r * sinf(ph);
  return V3(fmaf(x, s.x, fmaf(y, t.x, z * n.x)), fmaf(x, s.y, fmaf(y, t.y, z * n.y)), fmaf(x, s.z, fmaf(y, t.z, z * n.z)));
}
// the projector's texture value at a vertex, per colour channel: proj_tex_value's values.  (Its own statement, one loop over the channels: through
// proj_tex_value, which gathers the first channel ahead of the branch as the render kernels always did, the path kernels compile to other machine code.)
__device__ __forceinline__ void path_tex(const ShadeK &c, const SampleTerms &st, const float *__restrict__ tex, float (&tv)[3]) {
  const int tc = c.tc;
  const size_t o00 = ((size_t)st.iy0 * c.tw + st.ix0) * tc, o01 = ((size_t)st.iy0 * c.tw + st.ix1) * tc;
  const size_t o10 = ((size_t)st.iy1 * c.tw + st.ix0) * tc, o11 = ((size_t)st.iy1 * c.tw + st.ix1) * tc;
  if (tc == 1) {
    const float v = st.wy0 * (st.wx0 * tex[o00] + st.wx1 * tex[o01]) + st.wy1 * (st.wx0 * tex[o10] + st.wx1 * tex[o11]);
    tv[0] = v * c.p_color[0]; tv[1] = v * c.p_color[1]; tv[2] = v * c.p_color[2];
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tv[ch] = st.wy0 * (st.wx0 * tex[o00 + ch] + st.wx1 * tex[o01 + ch]) + st.wy1 * (st.wx0 * tex[o10 + ch] + st.wx1 * tex[o11 + ch]);
  }
}
// the bounce at vertex pv towards wo: throughput *= pi f = (base A + B) / cos_o (Lambert rows: base).  pb receives what the derivative of f needs
// (prb): model (0: a Lambert row, f = base), A (the tint parts pi tau / lum included), 1 / cos_o and — TAU only — pi tau
struct PrbBounce { int model; float A, tau, ic; };
template <bool TAU>
__device__ __forceinline__ void path_bounce_weight(const ShadeK &c, const SampleTerms &st, const PathVtx &pv, v3 d, v3 wo, float (&f)[3], PrbBounce &pb) {
  const float *mt = mat_table(c);
  f[0] = st.base[0]; f[1] = st.base[1]; f[2] = st.base[2];
  pb.model = 0; pb.A = 1.f; pb.tau = 0.f; pb.ic = 1.f;
  float A, B, T = 0.f, cos_o;
  if (row_terms<TAU>(c, mt, st.shape, pv.textured, st.base, pv.ns, V3(-d.x, -d.y, -d.z), wo, A, B, T, &cos_o)) {
    const float ic = cos_o > 0.f ? 1.0f / cos_o : 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) f[ch] = (st.base[ch] * A + B) * ic;
    pb.model = 1; pb.A = A; pb.tau = T; pb.ic = ic;
  }
}
struct PathArgs { const BvhNode *nodes; const TriRec *recs; const float4 *nrec; int spp, max_depth, rr_depth; uint32_t seed_key, path_key; };
struct NoBounce {
  template <typename... T> __device__ __forceinline__ void operator()(T &&...) const {}
};
// one path of sample idx whose camera ray is (o, d) in (nt, ft], every caller's by the same arithmetic in the same order.  At every vertex
// visit(v, st, ap, mv, d, beta) sees the emitters' terms and the throughput (ap with APP, mv with MAT: shade_sample's); then the bounce (vertex
// v < max_depth - 1), the roulette (v >= rr_depth: q and the survival test are constants of a replay) and, after a bounce that survived,
// bounce(v, st, pv, ap, d, wo, beta, iq, f, pb) — beta is the throughput in front of the bounce, iq = 1 / q_v, pb.tau is formed with APP only —
// and the secondary ray from the lifted point.  !EMIT: shade_sample's — the main emitters are left out and the visitor is visit(v, st, pv, d, beta).
// AMB (the constant emitter): escaped(beta) is told of every ray of the walk that hit nothing — the camera ray (beta = 1), a bounce ray
// (beta: the throughput behind that bounce) — and the last vertex, where the walk stops, makes its bounce all the same (direction, weight, roulette: the
// numbers (v, 0..2) no other walk draws) as ONE any-hit ray from the lifted point: a bounce that ends in an occlusion test
template <bool APP = false, bool MAT = false, bool EMIT = true, bool AMB = false, typename V, typename B = NoBounce, typename E = NoBounce>
__device__ __forceinline__ void path_walk(const PathArgs &a, uint32_t idx, v3 o, v3 d, float nt, float ft, int *stack, int stride, V &&visit, B &&bounce = B(),
                                          E &&escaped = E()) {
  const ShadeK &c = kernarg_shade();
  SampleTerms st;
  std::conditional_t<EMIT, PathVtx, PathVtxP> pv;
  AppTerms ap;
  MatVtx mv;
  shade_sample<true, APP, MAT, EMIT>(c, a.nodes, a.recs, a.nrec, o, d, nt, ft, st, stack, stride, &pv, &ap, &mv);
  float beta[3] = {1.f, 1.f, 1.f};
  if constexpr (AMB) {
    if (!st.hit) escaped(beta);
  }
  for (int v = 1; st.hit && pv.ok; ++v) {
    if constexpr (EMIT) visit(v, st, ap, mv, d, beta);
    else visit(v, st, pv, d, beta);
    const bool last = v + 1 >= a.max_depth;
    if (!AMB && last) break;
    const v3 wo = cosine_dir(pv.ns, path_u(a.path_key, idx, v, 0), path_u(a.path_key, idx, v, 1));
    if (!(vdot(pv.ng, wo) > 0.f)) break;
    float f[3], nb[3];
    PrbBounce pb;
    path_bounce_weight<APP>(c, st, pv, d, wo, f, pb);
    nb[0] = beta[0] * f[0]; nb[1] = beta[1] * f[1]; nb[2] = beta[2] * f[2];
    const float bmax = fmaxf(nb[0], fmaxf(nb[1], nb[2]));
    if (!(bmax > 0.f)) break;
    float iq = 1.0f;
    if (v >= a.rr_depth) { // Mitsuba's roulette: survive with q = min(max beta, 0.95), then beta /= q
      const float q = fminf(bmax, 0.95f);
      if (path_u(a.path_key, idx, v, 2) >= q) break;
      iq = 1.0f / q;
      nb[0] *= iq; nb[1] *= iq; nb[2] *= iq;
    }
    if constexpr (AMB) {
      if (last) { // the closing ray (every lane that comes this far comes here in the same turn of the loop: max_depth is uniform)
        Hit hc;
        if (!traverse<true, false>(a.nodes, a.recs, pv.Po, wo, 0.f, 3.0e38f, hc, stack, stride)) escaped(nb);
        break;
      }
    }
    bounce(v, st, pv, ap, d, wo, beta, iq, f, pb);
    beta[0] = nb[0]; beta[1] = nb[1]; beta[2] = nb[2];
    o = pv.Po;
    d = wo;
    shade_sample<true, APP, MAT, EMIT>(c, a.nodes, a.recs, a.nrec, o, d, 0.f, 3.0e38f, st, stack, stride, &pv, &ap, &mv);
    if constexpr (AMB) {
      if (!st.hit) escaped(beta);
    }
  }
}
__device__ __forceinline__ float wave_sum_tree(float v) { // (fixed order: the same bits on every run)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// RF: the gaussian film — the pixel's 25 x 4 outgoing sums into `part` ([pixel][25][4], k_rf_gather forms the image); else the pixel's mean into img
template <bool RF>
__global__ void __launch_bounds__(64)
    k_path_fwd(ShadeK c, PathArgs a, const float *__restrict__ tex, int fp16, void *__restrict__ img, float *__restrict__ part) {
  extern __shared__ int s_dyn[];
  __shared__ __attribute__((aligned(16))) float s_rf[RF ? FFX_RF_FLOATS : 4];
  const int lane = threadIdx.x;
  const uint32_t pix = blockIdx.x;
  const int W = c.cam.W, px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
    float jx, jy;
    sample_jitter(a.seed_key, idx, jx, jy);
    float L[3] = {0.f, 0.f, 0.f};
    if (s < a.spp) {
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      path_walk(a, idx, o, d, nt, ft, s_dyn + lane, 64, [&](int, const SampleTerms &st, const AppTerms &, const MatVtx &, v3, const float (&beta)[3]) {
        const ShadeK &k = kernarg_shade();
        float r[3] = {st.spot[0], st.spot[1], st.spot[2]}, b[3] = {st.spot_b[0], st.spot_b[1], st.spot_b[2]};
        if (st.has_proj) {
          float tv[3];
          path_tex(k, st, tex, tv);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) { r[ch] += tv[ch] * st.proj_fac; b[ch] += tv[ch] * st.proj_fac_b; }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) L[ch] += beta[ch] * (k.mat_stride == 3 ? st.base[ch] * r[ch] : st.base[ch] * r[ch] + b[ch]);
      });
    }
    if (RF) {
      float gx[5], gy[5];
      rf_weights(c.rf, jx, gx);
      rf_weights(c.rf, jy, gy);
      rf_fold(s_rf, lane, gx, gy, L[0], L[1], L[2], s < a.spp ? 1.f : 0.f, acc);
    } else {
      acc[0] += L[0]; acc[1] += L[1]; acc[2] += L[2];
    }
  }
  if (RF) {
    rf_store(part, pix, lane, acc);
    return;
  }
  const float inv_spp = 1.0f / (float)a.spp;
  const float m0 = wave_sum_tree(acc[0]) * inv_spp, m1 = wave_sum_tree(acc[1]) * inv_spp, m2 = wave_sum_tree(acc[2]) * inv_spp;
  if (lane == 0) {
    if (fp16 & 1) {
      _Float16 *p = (_Float16 *)img + (size_t)pix * 3;
      p[0] = (_Float16)m0; p[1] = (_Float16)m1; p[2] = (_Float16)m2;
    } else {
      float *p = (float *)img + (size_t)pix * 3;
      p[0] = m0; p[1] = m1; p[2] = m2;
    }
  }
}
// ------------------------------------------------------------------------------------------ extra emitters
// FFX_RENDER_LIGHTS(n) (include/ffx.h): n further delta emitters — point lights and spots — in a pass of its own behind the launches of the main image.
// k_path_fwd's shape (one wave = one pixel, lane l takes samples l, l + 64, ...) and its walk (path_walk<..., !EMIT>: the same hits, bounces and
// roulette, the two main emitters left out); at every vertex the n lights by the formulas of shade_sample's spot.  The pixel's mean is ADDED to img
// (box film: the pixel's own wave, lane 0; gaussian film: the sums through the scratch, k_lights_gather adds).  No atomics.
// The table's records (FFX_LIGHT_FLOATS floats each, read with wave-uniform addresses) are turned into what a vertex needs once per wave, in LDS:
#define FFX_LK_POS 0    // the light's position: to_world's translation
#define FFX_LK_INV 3    // inverse of to_world's 3 x 3, row-major (spots)
#define FFX_LK_INT 12   // intensity
#define FFX_LK_CBEAM 15 // cos(beam_width), cos(cutoff), cutoff in radians, 1 / (cutoff - beam_width)
#define FFX_LK_CCUT 16
#define FFX_LK_CUT 17
#define FFX_LK_ITRANS 18
#define FFX_LK_TYPE 19
#define FFX_LK_FLOATS 20
// DIR (the directional emitter): a record of type FFX_LIGHT_DIRECTIONAL parks wi = -normalize(to_world's 3 x 3 . (0, 0, 1)) in the position's
// three floats — (0, 0, 0) where that is no finite unit vector, which no vertex's cosine test passes — and its irradiance in the intensity's
template <bool DIR = false>
__device__ __forceinline__ void lights_derive(const float *__restrict__ table, int n, int lane, float *__restrict__ s_l) {
  for (int k = 0; k < n; ++k) { // (wave-uniform: every lane forms the same values, lane 0 parks them)
    const float *m = table + (size_t)FFX_LIGHT_FLOATS * k;
    if constexpr (DIR) {
      if (m[21] == (float)FFX_LIGHT_DIRECTIONAL) { // (wave-uniform)
        const float zx = m[2], zy = m[6], zz = m[10];
        const float il = 1.0f / sqrtf(zx * zx + zy * zy + zz * zz);
        v3 wi = V3(-zx * il, -zy * il, -zz * il);
        const float l2 = vdot(wi, wi);
        if (!(l2 > 0.99f && l2 < 1.01f)) wi = V3(0.f, 0.f, 0.f); // (a zero, infinite or NaN axis: lights nothing)
        if (lane == 0) {
          float *o = s_l + FFX_LK_FLOATS * k;
          o[FFX_LK_POS] = wi.x; o[FFX_LK_POS + 1] = wi.y; o[FFX_LK_POS + 2] = wi.z;
          o[FFX_LK_INT] = m[16]; o[FFX_LK_INT + 1] = m[17]; o[FFX_LK_INT + 2] = m[18];
          o[FFX_LK_TYPE] = m[21];
        }
        continue;
      }
    }
    const float a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const float c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const float idet = 1.0f / (a00 * c00 + a01 * c01 + a02 * c02); // (a singular frame: no finite cosine below, the spot lights nothing)
    const float deg = 0.017453292519943295f, cutoff = m[19] * deg, beam = m[20] * deg;
    if (lane == 0) {
      float *o = s_l + FFX_LK_FLOATS * k;
      o[FFX_LK_POS] = m[3]; o[FFX_LK_POS + 1] = m[7]; o[FFX_LK_POS + 2] = m[11];
      o[FFX_LK_INV + 0] = c00 * idet; o[FFX_LK_INV + 1] = (a02 * a21 - a01 * a22) * idet; o[FFX_LK_INV + 2] = (a01 * a12 - a02 * a11) * idet;
      o[FFX_LK_INV + 3] = c01 * idet; o[FFX_LK_INV + 4] = (a00 * a22 - a02 * a20) * idet; o[FFX_LK_INV + 5] = (a02 * a10 - a00 * a12) * idet;
      o[FFX_LK_INV + 6] = c02 * idet; o[FFX_LK_INV + 7] = (a01 * a20 - a00 * a21) * idet; o[FFX_LK_INV + 8] = (a00 * a11 - a01 * a10) * idet;
      o[FFX_LK_INT] = m[16]; o[FFX_LK_INT + 1] = m[17]; o[FFX_LK_INT + 2] = m[18];
      o[FFX_LK_CBEAM] = cosf(beam); o[FFX_LK_CCUT] = cosf(cutoff); o[FFX_LK_CUT] = cutoff; o[FFX_LK_ITRANS] = 1.0f / (cutoff - beam);
      o[FFX_LK_TYPE] = m[21];
    }
  }
  __syncthreads();
}
// lights_at_vertex's last statement, for its directional and its positional arm: record k's term from the arm's factors f, fb without the intensity.  (A
// macro: stated as a lambda or as a function, one addition of every k_lights_bwd instance comes out with its operands commuted — tools/isa_same.py.)
// It reads, by these names, lights_at_vertex's ADJ, c, st, beta, L, q, sums, stride, the loop's k and lk and the arm's f and fb
#define FFX_LIGHT_ADD()                                                                                                     \
  _Pragma("unroll") for (int ch = 0; ch < 3; ++ch) {                                                                        \
    if constexpr (ADJ) {                                                                                                    \
      sums[(3 * k + ch) * stride] += q[ch] * (beta[ch] * (c.mat_stride == 3 ? st.base[ch] * f : st.base[ch] * f + fb));     \
    } else {                                                                                                                \
      const float r = lk[FFX_LK_INT + ch] * f, b = lk[FFX_LK_INT + ch] * fb;                                                \
      L[ch] += beta[ch] * (c.mat_stride == 3 ? st.base[ch] * r : st.base[ch] * r + b);                                      \
    }                                                                                                                       \
  }
// the n lights at one vertex (st, pv: shade_sample<true, ..., !EMIT>'s; d: the ray that found it), weighted by the throughput beta, into L.
// DIR: a directional record (lights_derive<true>'s) has no position, no falloff and no 1 / d^2; its shadow ray leaves the lifted point along wi, the closing
// ray's form (path_walk's AMB), on the lane's own stack.
// ADJ (k_lights_bwd): the same geometry, falloff, shadow ray and row_terms, but record k's term WITHOUT its intensity, times the sample's
// adjoint weight q, is added to the record's three sums sums[(3 k + ch) * stride]; L is not touched
template <bool DIR = false, bool ADJ = false>
__device__ __forceinline__ void lights_at_vertex(const ShadeK &c, const PathArgs &a, const float *__restrict__ s_l, int n, const SampleTerms &st, const PathVtxP &pv, v3 d,
                                                 const float (&beta)[3], int *stack, int stride, float (&L)[3], const float *q = nullptr, float *sums = nullptr) {
  const float *mt = mat_table(c);
  for (int k = 0; k < n; ++k) {
    const float *lk = s_l + FFX_LK_FLOATS * k;
    if constexpr (DIR) {
      if (lk[FFX_LK_TYPE] == (float)FFX_LIGHT_DIRECTIONAL) { // (wave-uniform branch: s_l is read at uniform addresses)
        const v3 wi = V3(lk[FFX_LK_POS], lk[FFX_LK_POS + 1], lk[FFX_LK_POS + 2]);
        const float cos_s = vdot(pv.ns, wi);
        if (!(cos_s > 0.f && vdot(pv.ng, wi) > 0.f)) continue;
        if (c.shadows) {
          Hit hs;
          if (traverse<true, false>(a.nodes, a.recs, pv.Po, wi, 0.f, 3.0e38f, hs, stack, stride)) continue;
        }
        float bA = cos_s, bB = 0.f, bT = 0.f;
        row_terms<false>(c, mt, st.shape, pv.textured, st.base, pv.ns, V3(-d.x, -d.y, -d.z), wi, bA, bB, bT);
        const float f = bA * 0.3183098861837907f, fb = bB * 0.3183098861837907f;
        FFX_LIGHT_ADD();
        continue;
      }
    }
    const v3 lpos = V3(lk[FFX_LK_POS], lk[FFX_LK_POS + 1], lk[FFX_LK_POS + 2]);
    v3 wi = vsub(lpos, pv.P);
    const float d2 = vdot(wi, wi);
    if (!(d2 > 0.f)) continue;
    const float idist = 1.0f / sqrtf(d2);
    wi = V3(wi.x * idist, wi.y * idist, wi.z * idist);
    const float cos_s = vdot(pv.ns, wi);
    if (!(cos_s > 0.f && vdot(pv.ng, wi) > 0.f)) continue;
    float fall = 1.f;
    if (lk[FFX_LK_TYPE] != 0.f) { // a spot: the falloff in the light's local frame (wave-uniform branch)
      const float *iv = lk + FFX_LK_INV;
      const v3 w = V3(-wi.x, -wi.y, -wi.z);
      const v3 ll = V3(iv[0] * w.x + iv[1] * w.y + iv[2] * w.z, iv[3] * w.x + iv[4] * w.y + iv[5] * w.z, iv[6] * w.x + iv[7] * w.y + iv[8] * w.z);
      const float cos_t = ll.z / sqrtf(vdot(ll, ll));
      fall = 0.f;
      if (cos_t >= lk[FFX_LK_CBEAM]) fall = 1.f;
      else if (cos_t > lk[FFX_LK_CCUT]) fall = (lk[FFX_LK_CUT] - acosf(cos_t)) * lk[FFX_LK_ITRANS];
      if (!(fall > 0.f)) continue;
    }
    if (c.shadows) { // shade_sample's ray: from the emitter to the lifted point, t in (0, 1 - eps)
      Hit hs;
      if (traverse<true, true>(a.nodes, a.recs, lpos, vsub(pv.Po, lpos), 0.f, 1.0f - SHADOW_EPS, hs, stack, stride)) continue;
    }
    float bA = cos_s, bB = 0.f, bT = 0.f;
    row_terms<false>(c, mt, st.shape, pv.textured, st.base, pv.ns, V3(-d.x, -d.y, -d.z), wi, bA, bB, bT);
    const float f = fall * bA / d2 * 0.3183098861837907f, fb = fall * bB / d2 * 0.3183098861837907f;
    FFX_LIGHT_ADD();
  }
}
#undef FFX_LIGHT_ADD
// The pass's one kernel.  RF: the gaussian film — the sums of the lights' radiance into `part` (k_lights_gather adds them to the image); else img += the pixel's mean.
// DIR (FFX_RENDER_LIGHTS_DIRECTIONAL, include/ffx.h): the table may hold directional records — all three record types in one walk per sample.
// AMB (FFX_RENDER_AMBIENT, include/ffx.h): the constant emitter in the same walk — its record (r, g, b, 0) stands behind the n_lights records
// (n_lights may be 0); every ray of the walk that escapes, and the closing ray at its last vertex (path_walk's AMB), adds throughput x radiance to the
// sample that the lights' terms go to
template <bool RF, bool DIR, bool AMB>
__global__ void __launch_bounds__(64)
    k_lights_fwd(ShadeK c, PathArgs a, const float *__restrict__ lights, int n_lights, float *__restrict__ img, float *__restrict__ part) {
  extern __shared__ int s_dyn[];
  __shared__ __attribute__((aligned(16))) float s_rf[RF ? FFX_RF_FLOATS : 4];
  __shared__ float s_l[FFX_RENDER_MAX_LIGHTS * FFX_LK_FLOATS];
  const int lane = threadIdx.x;
  const uint32_t pix = blockIdx.x;
  const int W = c.cam.W, px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
  const int n = n_lights < FFX_RENDER_MAX_LIGHTS ? n_lights : FFX_RENDER_MAX_LIGHTS; // (the host refuses more: s_l holds this many)
  lights_derive<DIR>(lights, n, lane, s_l);
  float la0 = 0.f, la1 = 0.f, la2 = 0.f;
  if constexpr (AMB) {
    const float *la = lights + (size_t)FFX_LIGHT_FLOATS * n; // (the ambient record, at a wave-uniform address: scalar loads)
    la0 = la[0]; la1 = la[1]; la2 = la[2];
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
    float jx, jy;
    sample_jitter(a.seed_key, idx, jx, jy);
    float L[3] = {0.f, 0.f, 0.f};
    if (s < a.spp) {
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      const auto at_vertex = [&](int, const SampleTerms &st, const PathVtxP &pv, v3 dv, const float (&beta)[3]) {
        lights_at_vertex<DIR>(kernarg_shade(), a, s_l, n, st, pv, dv, beta, s_dyn + lane, 64, L);
      };
      if constexpr (DIR || AMB)
        path_walk<false, false, false, AMB>(a, idx, o, d, nt, ft, s_dyn + lane, 64, at_vertex, NoBounce(),
                                            [&](const float (&beta)[3]) { L[0] += beta[0] * la0; L[1] += beta[1] * la1; L[2] += beta[2] * la2; });
      else // (the plain instances without the hooks, as they were written: with them the three sums of L change registers — tools/isa_same.py)
        path_walk<false, false, false>(a, idx, o, d, nt, ft, s_dyn + lane, 64, at_vertex);
    }
    if (RF) {
      float gx[5], gy[5];
      rf_weights(c.rf, jx, gx);
      rf_weights(c.rf, jy, gy);
      rf_fold(s_rf, lane, gx, gy, L[0], L[1], L[2], s < a.spp ? 1.f : 0.f, acc);
    } else {
      acc[0] += L[0]; acc[1] += L[1]; acc[2] += L[2];
    }
  }
  if (RF) {
    rf_store(part, pix, lane, acc);
    return;
  }
  const float inv_spp = 1.0f / (float)a.spp;
  const float m0 = wave_sum_tree(acc[0]) * inv_spp, m1 = wave_sum_tree(acc[1]) * inv_spp, m2 = wave_sum_tree(acc[2]) * inv_spp;
  if (lane == 0) {
    float *p = img + (size_t)pix * 3;
    p[0] += m0; p[1] += m1; p[2] += m2;
  }
}
// k_rf_gather's sums of the lights' pass, added to the image the main gather wrote: img += (r, g, b) / weight (the weight is the jitter's alone: the main image's)
__global__ void __launch_bounds__(64) k_lights_gather(const float4 *__restrict__ part, int W, int H, float *__restrict__ img) {
  __shared__ float4 s_seg[68 * 5];
  const int lane = threadIdx.x;
  const int x0 = blockIdx.x * 64, y = blockIdx.y;
  if (y >= H) return;
  float r, g, b, w;
  rf_window_sums(part, W, H, x0, y, lane, s_seg, r, g, b, w);
  const int x = x0 + lane;
  if (x >= W || !(w > 0.f)) return;
  float *p = img + ((size_t)y * W + x) * 3;
  p[0] += r / w; p[1] += g / w; p[2] += b / w;
}

// ---- the pieces of the per-lane replay adjoints (k_path_bwd, the direct-light leaves of 4.5 / 4.5.1, prb of 4.5.2): one wave = one pixel ----
// the adjoint of a pixel.  Box film: g = gimg[pixel] / spp; RF: gsrc is G = gimg / weight as float4 per pixel (k_rf_gather) and lanes 0..24 hold G of
// window pixel `lane`.  false: nothing flows into this pixel's samples (wave-uniform; box: block-uniform)
template <bool RF>
__device__ __forceinline__ bool pixel_adjoint(const float *__restrict__ gsrc, uint32_t pix, int px, int py, int W, int H, int lane, int spp, float (&g)[3]) {
  if (RF) {
    const float4 gw = rf_window_g(reinterpret_cast<const float4 *>(gsrc), px, py, W, H, lane, true);
    g[0] = gw.x; g[1] = gw.y; g[2] = gw.z;
    return wballot(g[0] != 0.f || g[1] != 0.f || g[2] != 0.f) != 0ull;
  }
  const float inv_spp = 1.0f / (float)spp;
  g[0] = gsrc[(size_t)pix * 3] * inv_spp; g[1] = gsrc[(size_t)pix * 3 + 1] * inv_spp; g[2] = gsrc[(size_t)pix * 3 + 2] * inv_spp;
  return !(g[0] == 0.f && g[1] == 0.f && g[2] == 0.f);
}
// cw (d loss / d texture value per channel at a vertex) into the projector texture's gradient through the vertex's four bilinear taps: path_tex's adjoint
// (taps_scatter's values; written out for the same reason as path_tex)
__device__ __forceinline__ void proj_tex_scatter(const ShadeK &k, const SampleTerms &st, const float (&cw)[3], float *__restrict__ gtex) {
  const int tc = k.tc;
  const size_t o00 = ((size_t)st.iy0 * k.tw + st.ix0) * tc, o01 = ((size_t)st.iy0 * k.tw + st.ix1) * tc;
  const size_t o10 = ((size_t)st.iy1 * k.tw + st.ix0) * tc, o11 = ((size_t)st.iy1 * k.tw + st.ix1) * tc;
  if (tc == 1) {
    const float ws = cw[0] * k.p_color[0] + cw[1] * k.p_color[1] + cw[2] * k.p_color[2];
    atomicAdd(gtex + o00, ws * st.wy0 * st.wx0);
    atomicAdd(gtex + o01, ws * st.wy0 * st.wx1);
    atomicAdd(gtex + o10, ws * st.wy1 * st.wx0);
    atomicAdd(gtex + o11, ws * st.wy1 * st.wx1);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      atomicAdd(gtex + o00 + ch, cw[ch] * st.wy0 * st.wx0);
      atomicAdd(gtex + o01 + ch, cw[ch] * st.wy0 * st.wx1);
      atomicAdd(gtex + o10 + ch, cw[ch] * st.wy1 * st.wx0);
      atomicAdd(gtex + o11 + ch, cw[ch] * st.wy1 * st.wx1);
    }
  }
}
// the adjoint: replays k_path_fwd's paths and scatters every vertex's projector term, weighted by the sample's d loss / d radiance, through its four
// bilinear taps
template <bool RF>
__global__ void __launch_bounds__(64)
    k_path_bwd(ShadeK c, PathArgs a, const float *__restrict__ gsrc, float *__restrict__ gtex) {
  extern __shared__ int s_dyn[];
  const int lane = threadIdx.x;
  const uint32_t pix = blockIdx.x;
  const int W = c.cam.W, H = c.cam.H, px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
  float g[3];
  if (!pixel_adjoint<RF>(gsrc, pix, px, py, W, H, lane, a.spp, g)) return;
  for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
    float jx, jy, q[3];
    sample_jitter(a.seed_key, idx, jx, jy);
    sample_adjoint<RF>(c.rf, jx, jy, g, q);
    if (s >= a.spp || (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f)) continue;
    v3 o, d;
    float nt, ft;
    cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
    path_walk(a, idx, o, d, nt, ft, s_dyn + lane, 64, [&](int, const SampleTerms &st, const AppTerms &, const MatVtx &, v3, const float (&beta)[3]) {
      if (!st.has_proj) return;
      float cw[3]; // d radiance / d (texture value) per channel, times the sample's gradient
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) cw[ch] = q[ch] * beta[ch] * (st.base[ch] * st.proj_fac + st.proj_fac_b);
      proj_tex_scatter(kernarg_shade(), st, cw, gtex);
    });
  }
}
// ------------------------------------------------------------------------------------------ extra emitters' adjoint
// FFX_RENDER_EMITTER_GRAD (include/ffx.h): d loss / d (the RGB power of every light record, the constant emitter's radiance).  The walk does not depend on the
// emitters, so the image is linear in those powers and the derivative is the adjoint-weighted image at unit power: k_lights_fwd<RF, true, AMB>'s walk once more
// (lights_derive<true>, path_walk<..., AMB>, the same jitter and path keys: the forward's paths by construction), where lights_at_vertex<true, ADJ> adds record k's
// q[ch] beta[ch] (base[ch] f + fb) to the record's sum and every escaped ray q[ch] beta[ch] to the ambient's.  One wave = one pixel, lane l takes samples
// l, l + 64, ...; a lane's 3 n record sums live in LDS, one column per lane (stride 64: conflict-free; a run-time record number never indexes registers)
// behind the traversal stack in the dynamic area (stack_ints ints, then 3 n x 64 floats: a table of one record does not pay LDS, and with it occupancy,
// for eight), the ambient's three in registers.  No atomics: the wave's sums go to the pixel's slot of the workspace [FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS]
// [pixels] — zeros from a pixel nothing flows into, so that every slot is written by every call — and k_lights_grad_reduce adds the slots in a fixed order
template <bool RF, bool AMB>
__global__ void __launch_bounds__(64)
    k_lights_bwd(ShadeK c, PathArgs a, const float *__restrict__ lights, int n_lights, const float *__restrict__ gsrc, float *__restrict__ slots, int stack_ints) {
  extern __shared__ int s_dyn[];
  __shared__ float s_l[FFX_RENDER_MAX_LIGHTS * FFX_LK_FLOATS];
  float *s_sum = reinterpret_cast<float *>(s_dyn + stack_ints);
  const int lane = threadIdx.x;
  const uint32_t pix = blockIdx.x;
  const int W = c.cam.W, H = c.cam.H, px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
  const int n = n_lights < FFX_RENDER_MAX_LIGHTS ? n_lights : FFX_RENDER_MAX_LIGHTS; // (the host refuses more: s_l holds this many)
  float *slot = slots + (size_t)lane * ((size_t)W * (size_t)H) + pix; // (lanes < FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS: entry `lane` of the pixel's slot)
  float g[3];
  bool flows; // pixel_adjoint<RF>'s values.  (The gaussian film's window is fetched by a statement of this kernel's own: one more caller of rf_window_g, and the
              // packet kernels that inline it compile to other machine code — commuted operands of the window's bounds tests, tools/isa_same.py.)
  if constexpr (RF) {
    const int wb = (lane * 13) >> 6, wa = lane - 5 * wb, tx = px + wa - 2, ty = py + wb - 2;
    float4 gw = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 25 && tx >= 0 && tx < W && ty >= 0 && ty < H) gw = reinterpret_cast<const float4 *>(gsrc)[(size_t)ty * W + tx];
    g[0] = gw.x; g[1] = gw.y; g[2] = gw.z;
    flows = wballot(g[0] != 0.f || g[1] != 0.f || g[2] != 0.f) != 0ull;
  } else {
    flows = pixel_adjoint<false>(gsrc, pix, px, py, W, H, lane, a.spp, g);
  }
  if (!flows) { // (wave-uniform, and the wave is the workgroup)
    if (lane < FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS) *slot = 0.f;
    return;
  }
  lights_derive<true>(lights, n, lane, s_l);
  for (int j = 0; j < 3 * n; ++j) s_sum[j * 64 + lane] = 0.f;
  float amb[3] = {0.f, 0.f, 0.f};
  for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
    float jx, jy, q[3];
    sample_jitter(a.seed_key, idx, jx, jy);
    sample_adjoint<RF>(c.rf, jx, jy, g, q);
    if (s >= a.spp || (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f)) continue;
    v3 o, d;
    float nt, ft;
    cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
    path_walk<false, false, false, AMB>(
        a, idx, o, d, nt, ft, s_dyn + lane, 64,
        [&](int, const SampleTerms &st, const PathVtxP &pv, v3 dv, const float (&beta)[3]) {
          lights_at_vertex<true, true>(kernarg_shade(), a, s_l, n, st, pv, dv, beta, s_dyn + lane, 64, amb, q, s_sum + lane);
        },
        NoBounce(), [&](const float (&beta)[3]) { amb[0] += q[0] * beta[0]; amb[1] += q[1] * beta[1]; amb[2] += q[2] * beta[2]; });
  }
  float mine = 0.f; // (lane j: the wave's sum j; rows of absent records and of an absent constant emitter stay 0)
  for (int j = 0; j < 3 * n; ++j) {
    const float v = wave_sum_tree(s_sum[j * 64 + lane]);
    if (lane == j) mine = v;
  }
  if constexpr (AMB) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = wave_sum_tree(amb[ch]);
      if (lane == 3 * FFX_RENDER_MAX_LIGHTS + ch) mine = v;
    }
  }
  if (lane < FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS) *slot = mine;
}
// the result block from the pixels' slots: workgroup j adds entry j of every slot (contiguous: slots[j][pixels]) — a thread its pixels in ascending order, then a tree over the threads
// (a fixed order: the same bits on every run) — and WRITES block[j]; 0 for the row of an absent record or of an absent constant emitter
#define FFX_EG_REDUCE_THREADS 1024
__global__ void __launch_bounds__(FFX_EG_REDUCE_THREADS) k_lights_grad_reduce(const float *__restrict__ slots, int n_pix, int n, int amb, float *__restrict__ block) {
  __shared__ float s_p[FFX_EG_REDUCE_THREADS];
  const int j = blockIdx.x, row = j / 3, t = threadIdx.x;
  const bool live = row < n || (row == FFX_RENDER_MAX_LIGHTS && amb); // (workgroup-uniform)
  float v = 0.f;
  if (live)
    for (int p = t; p < n_pix; p += FFX_EG_REDUCE_THREADS) v += slots[(size_t)j * (size_t)n_pix + p];
  s_p[t] = v;
  __syncthreads();
  for (int off = FFX_EG_REDUCE_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) s_p[t] += s_p[t + off];
    __syncthreads();
  }
  if (t == 0) block[j] = s_p[0];
}

// ------------------------------------------------------------------------------------------ appearance adjoint
// FFX_RENDER_GRAD_APPEARANCE (include/ffx.h): d loss / d (the rows' base colours, the spot's intensity, base-colour textures) at max_depth 2.  Per sample
// and channel L_c = b_c E_c + F_c with E_c = spot_c + tex_c proj_fac (the parts scaled by the base colour b, the tint terms pi tau / lum(b) included)
// and F_c their b-free parts.  With T_c the tint parts' numerators (s_int_c spot_t + tex_c proj_t) and the sample's adjoint weight q_c:
//   d/db_k sum_c q_c L_c = q_k E_k - (sum_c q_c b_c T_c) w_k / lum^2        (w = the luminance weights; T = 0 where lum <= 0)
//   d/dI_c              = q_c (b_c s_f + s_fb)                              (the spot's factors at unit intensity)
// Samples replay the forward's (same jitter and seed) with shade_sample's per-lane walk.  One wave = one pixel at a time, a workgroup of four waves
// strides over the film; row sums go through LDS (one global atomic per non-zero entry and workgroup), the spot's through a wave sum (one atomic per
// wave), a textured base colour's through its four bilinear taps (global atomics).
#define FFX_APP_WAVES 4
#define FFX_APP_LDS_ROWS 255
#define FFX_MAT_LDS_ROWS 64 // (k_render_bwd_material: rows of [FFX_MAT_GRAD_COLS] sums in LDS; more shapes go straight to global atomics)
static_assert(64 * FFX_APP_WAVES == TR_BLOCK, "k_render_bwd_appearance takes the per-lane kernels' traversal stack (stack_bytes)");
struct AppArgs {
  const BvhNode *nodes; const TriRec *recs; const float4 *nrec;
  const float *tex; // the projector texture [tex_h, tex_w, tex_channels] (NULL without a projector)
  int spp, n_pix, n_shapes;
  uint32_t seed_key;
  float *grow, *gspot, *gbt[FFX_MAX_BASE_TEX]; // [n_shapes][3], [3], [h][w][3] per base-colour texture
};
// the four texels (float offsets) and weights of base_tex_sample's bilinear lookup, by the same arithmetic
__device__ __forceinline__ void base_tex_taps(const ShadeK &c, int k, int slot, float bu, float bv, size_t (&o)[4], float (&w)[4]) {
  const float *uv = c.slot_uv + 6 * (size_t)slot;
  const float bw = (1.0f - bu) - bv;
  float u = fmaf(bw, uv[0], fmaf(bu, uv[2], bv * uv[4])), v = fmaf(bw, uv[1], fmaf(bu, uv[3], bv * uv[5]));
  u = u - floorf(u);
  v = v - floorf(v);
  const int tw = c.btw[k], th = c.bth[k];
  const float fx = fmaf(u, (float)tw, -0.5f), fy = fmaf(v, (float)th, -0.5f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  x0 = x0 < 0 ? x0 + tw : x0; x1 = x1 >= tw ? x1 - tw : x1; y0 = y0 < 0 ? y0 + th : y0; y1 = y1 >= th ? y1 - th : y1;
  x0 = x0 >= tw ? x0 - tw : x0; y0 = y0 >= th ? y0 - th : y0; x1 = x1 < 0 ? x1 + tw : x1; y1 = y1 < 0 ? y1 + th : y1;
  o[0] = ((size_t)y0 * tw + x0) * 3; o[1] = ((size_t)y0 * tw + x1) * 3; o[2] = ((size_t)y1 * tw + x0) * 3; o[3] = ((size_t)y1 * tw + x1) * 3;
  w[0] = (1.0f - ay) * (1.0f - ax); w[1] = (1.0f - ay) * ax; w[2] = ay * (1.0f - ax); w[3] = ay * ax;
}
__device__ __forceinline__ float base_lum(const SampleTerms &st) { return lum3(st.base[0], st.base[1], st.base[2]); }
// the appearance block at a vertex whose radiance carries the weight w (q at direct light, q beta in prb), tv = the projector's texture value there:
// gs += d/d (spot intensity), gb = d/d (base colour) = w E - r w_lum
__device__ __forceinline__ void base_colour_vjp(const ShadeK &k, const SampleTerms &st, const AppTerms &ap, const float (&tv)[3], const float (&w)[3], float (&gs)[3],
                                                float (&gb)[3]) {
  float E[3], qbt = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    E[ch] = st.spot[ch] + tv[ch] * st.proj_fac;
    qbt += w[ch] * st.base[ch] * (k.s_int[ch] * ap.spot_t + tv[ch] * ap.proj_t);
    gs[ch] += w[ch] * (st.base[ch] * ap.s_f + ap.s_fb);
  }
  const float lum = base_lum(st);
  const float r = lum > 0.f ? qbt / (lum * lum) : 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) gb[ch] = w[ch] * E[ch] - r * FFX_LUM_W[ch];
}
// the BSDF's adjoint at a vertex lit by the two emitters (FFX_RENDER_GRAD_MATERIAL): L_c = sum_e (b_c A_e + B_e) E_ec, one reverse pass per emitter —
// the projector's, then the spot's — with uA_e = sum_c w_c b_c E_ec, uB_e = sum_c w_c E_ec (wv: towards the viewer).  false: the row has no BSDF
// parameters or no emitter lights the vertex, gm is not formed
__device__ __forceinline__ bool emitters_material_vjp(const ShadeK &k, const SampleTerms &st, const MatVtx &mv, v3 wv, const float (&w)[3], const float (&tv)[3],
                                                      float (&gm)[FFX_MAT_GRAD_COLS]) {
  const float *mt = mat_table(k);
  if (!(principled_row(k, mt, st.shape) && (mv.kp != 0.f || mv.ks != 0.f))) return false;
  const float *mrow = mt + (size_t)FFX_MAT_STRIDE * st.shape;
  const float lum = base_lum(st);
#pragma unroll
  for (int j = 0; j < FFX_MAT_GRAD_COLS; ++j) gm[j] = 0.f;
  MatGeoD mg;
  if (mv.kp != 0.f) {
    float uA = 0.f, uB = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { const float e = w[ch] * tv[ch] * mv.kp; uA += e * st.base[ch]; uB += e; }
    material_geometry_d(mv.ns, wv, mv.wp, mg);
    material_terms_vjp(mrow, mg, lum, uA, uB, gm);
  }
  if (mv.ks != 0.f) {
    float uA = 0.f, uB = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { const float e = w[ch] * k.s_int[ch] * mv.ks; uA += e * st.base[ch]; uB += e; }
    material_geometry_d(mv.ns, wv, mv.ws, mg);
    material_terms_vjp(mrow, mg, lum, uA, uB, gm);
  }
  return true;
}
// a workgroup's sums per material row: base colours in s_rows when n_shapes <= FFX_APP_LDS_ROWS, BSDF parameters (MAT) in s_mat when n_shapes <=
// FFX_MAT_LDS_ROWS, global atomics otherwise; flush() leaves one global atomic per non-zero entry and workgroup.  nthr = the workgroup's threads
template <bool MAT>
struct RowSums {
  const AppArgs &a;
  float *s_rows, *s_mat, *gmat;
  bool lds, lds_m;
  __device__ __forceinline__ void init(int nthr) {
    lds = a.n_shapes <= FFX_APP_LDS_ROWS;
    if (lds)
      for (int i = threadIdx.x; i < a.n_shapes * 3; i += nthr) s_rows[i] = 0.f;
    lds_m = MAT && a.n_shapes <= FFX_MAT_LDS_ROWS;
    if (lds_m)
      for (int i = threadIdx.x; i < a.n_shapes * FFX_MAT_GRAD_COLS; i += nthr) s_mat[i] = 0.f;
    __syncthreads();
  }
  // d loss / d base colour at a vertex: into the row's sum, or through a base-colour texture's four taps
  __device__ __forceinline__ void add_base(int shape, const AppTerms &ap, const float (&gb)[3]) const {
    if (gb[0] == 0.f && gb[1] == 0.f && gb[2] == 0.f) return;
    if (ap.tix == 0) { // the row's own base colour
      if (lds) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) atomicAdd(&s_rows[shape * 3 + ch], gb[ch]);
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) atomicAdd(a.grow + (size_t)shape * 3 + ch, gb[ch]);
      }
    } else { // a base-colour texture: through the lookup's four taps
      float *gt = ap.tix == 1 ? a.gbt[0] : ap.tix == 2 ? a.gbt[1] : ap.tix == 3 ? a.gbt[2] : a.gbt[3];
      size_t to[4];
      float tw4[4];
      base_tex_taps(kernarg_shade(), ap.tix - 1, ap.slot, ap.bu, ap.bv, to, tw4);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) atomicAdd(gt + to[t] + ch, gb[ch] * tw4[t]);
      }
    }
  }
  __device__ __forceinline__ void add_mat(int shape, const float (&gm)[FFX_MAT_GRAD_COLS]) const {
    float *dst = lds_m ? s_mat + shape * FFX_MAT_GRAD_COLS : gmat + (size_t)shape * FFX_MAT_GRAD_COLS;
#pragma unroll
    for (int j = 0; j < FFX_MAT_GRAD_COLS; ++j)
      if (gm[j] != 0.f) atomicAdd(dst + j, gm[j]);
  }
  // gs: this lane's share of d loss / d spot intensity (a wave sum, one atomic per wave)
  __device__ __forceinline__ void flush(const float (&gs)[3], int lane, int nthr) const {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = wave_sum_tree(gs[ch]);
      if (lane == 0 && v != 0.f) atomicAdd(a.gspot + ch, v);
    }
    __syncthreads();
    if (lds)
      for (int i = threadIdx.x; i < a.n_shapes * 3; i += nthr) {
        const float v = s_rows[i];
        if (v != 0.f) atomicAdd(a.grow + i, v);
      }
    if (lds_m)
      for (int i = threadIdx.x; i < a.n_shapes * FFX_MAT_GRAD_COLS; i += nthr) {
        const float v = s_mat[i];
        if (v != 0.f) atomicAdd(gmat + i, v);
      }
  }
};
// the direct-light leaves: per sample the appearance block and — MAT (FFX_RENDER_GRAD_MATERIAL) — per lit emitter the BSDF's adjoint
// (material_terms_vjp) into gmat [n_shapes][FFX_MAT_GRAD_COLS].  One body for both kernels; each owns its static LDS
template <bool RF, bool MAT>
__device__ __forceinline__ void bwd_leaves(const ShadeK &c, const AppArgs &a, const float *__restrict__ gsrc, float *__restrict__ gmat, int *s_dyn, float *s_rows,
                                           float *s_mat) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RowSums<MAT> rs{a, s_rows, s_mat, gmat};
  rs.init(64 * FFX_APP_WAVES);
  const int W = c.cam.W, H = c.cam.H;
  float gs[3] = {0.f, 0.f, 0.f};
  for (long pl = (long)blockIdx.x * FFX_APP_WAVES + wave; pl < a.n_pix; pl += (long)gridDim.x * FFX_APP_WAVES) { // (wave-uniform)
    const uint32_t pix = (uint32_t)pl;
    const int px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
    float g[3];
    if (!pixel_adjoint<RF>(gsrc, pix, px, py, W, H, lane, a.spp, g)) continue;
    for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
      const int s = pass * 64 + lane;
      const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
      float jx, jy, q[3];
      sample_jitter(a.seed_key, idx, jx, jy);
      sample_adjoint<RF>(c.rf, jx, jy, g, q);
      if (s >= a.spp || (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f)) continue;
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      SampleTerms st;
      AppTerms ap;
      MatVtx mv;
      shade_sample<false, true, MAT>(kernarg_shade(), a.nodes, a.recs, a.nrec, o, d, nt, ft, st, s_dyn + threadIdx.x, 64 * FFX_APP_WAVES, nullptr, &ap, &mv);
      if (!st.hit) continue;
      const ShadeK &k = kernarg_shade();
      float tv[3] = {0.f, 0.f, 0.f};
      if (st.has_proj) path_tex(k, st, a.tex, tv);
      if (MAT) {
        float gm[FFX_MAT_GRAD_COLS];
        if (emitters_material_vjp(k, st, mv, V3(-d.x, -d.y, -d.z), q, tv, gm)) rs.add_mat(st.shape, gm);
      }
      float gb[3];
      base_colour_vjp(k, st, ap, tv, q, gs, gb);
      rs.add_base(st.shape, ap, gb);
    }
  }
  rs.flush(gs, lane, 64 * FFX_APP_WAVES);
}
// RF: gsrc is G = gimg / weight as float4 per pixel (k_rf_gather) and a sample's weight is sum_n w_n G[p + n]; else gsrc = gimg, weight gimg / spp
template <bool RF>
__global__ void __launch_bounds__(64 * FFX_APP_WAVES)
    k_render_bwd_appearance(ShadeK c, AppArgs a, const float *__restrict__ gsrc) {
  extern __shared__ int s_dyn[];
  __shared__ float s_rows[FFX_APP_LDS_ROWS * 3];
  bwd_leaves<RF, false>(c, a, gsrc, nullptr, s_dyn, s_rows, nullptr);
}
template <bool RF>
__global__ void __launch_bounds__(64 * FFX_APP_WAVES)
    k_render_bwd_material(ShadeK c, AppArgs a, const float *__restrict__ gsrc, float *__restrict__ gmat) {
  extern __shared__ int s_dyn[];
  __shared__ float s_rows[FFX_APP_LDS_ROWS * 3];
  __shared__ float s_mat[FFX_MAT_LDS_ROWS * FFX_MAT_GRAD_COLS];
  bwd_leaves<RF, true>(c, a, gsrc, gmat, s_dyn, s_rows, s_mat);
}

// ------------------------------------------------------------------------------------------ prb: the appearance and BSDF adjoints through bounces
// FFX_RENDER_GRAD_PRB (include/ffx.h): the blocks of FFX_RENDER_GRAD_APPEARANCE / FFX_RENDER_GRAD_MATERIAL at max_depth > 2, by path replay with the
// sampling decisions detached (Mitsuba's `prb`).  Per sample, with vertices v = 1 .. n, throughput beta_v, next-event term N_v = b R_v + F_v, bounce
// weight f_v = (b A_v + B_v) / cos_o (Lambert: b) and the roulette's q_v (1 where it does not run):
//   L = sum_v beta_v N_v,   S_v = N_v + (f_v / q_v) S_v+1,   dL/dtheta = sum_v beta_v [ dN_v/dtheta + (df_v/dtheta / q_v) S_v+1 ]
// Bounces are cosine-weighted, so no parameter moves a path; q_v and the survival tests are constants of the replay.  Two walks per sample: the first
// leaves N_v and f_v / q_v in LDS ([vertex][6][thread]), the lane folds them into the suffix radiances S_v, the second accumulates — at every vertex
// what k_render_bwd_appearance / k_render_bwd_material form per sample (weight q beta_v) and what k_path_bwd scatters into gtex, at every bounce the
// derivative of f_v.  Workgroups of 1, 2 or 4 waves (the host picks what fits 64 KB of LDS) stride over the film.
struct PrbArgs { int max_depth, rr_depth; uint32_t path_key; float *gtex, *gmat; };
// s_dyn: the traversal stack [stack_ints / threads][threads] followed by the path records [max_depth - 1][6][threads]
template <bool RF, bool MAT>
__device__ __forceinline__ void path_bwd_prb(const ShadeK &c, const AppArgs &a, const PrbArgs &p, const float *__restrict__ gsrc, int *s_dyn, int stack_ints,
                                             float *s_rows, float *s_mat) {
  const int nthr = blockDim.x, waves = nthr >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float *s_path = reinterpret_cast<float *>(s_dyn + stack_ints) + threadIdx.x;
  const int pstride = 6 * nthr; // floats per vertex
  const PathArgs pa = {a.nodes, a.recs, a.nrec, a.spp, p.max_depth, p.rr_depth, a.seed_key, p.path_key};
  RowSums<MAT> rs{a, s_rows, s_mat, p.gmat};
  rs.init(nthr);
  const int W = c.cam.W, H = c.cam.H;
  float gs[3] = {0.f, 0.f, 0.f};
  for (long pl = (long)blockIdx.x * waves + wave; pl < a.n_pix; pl += (long)gridDim.x * waves) { // (wave-uniform)
    const uint32_t pix = (uint32_t)pl;
    const int px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
    float g[3];
    if (!pixel_adjoint<RF>(gsrc, pix, px, py, W, H, lane, a.spp, g)) continue;
    for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
      const int s = pass * 64 + lane;
      const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
      float jx, jy, q[3];
      sample_jitter(a.seed_key, idx, jx, jy);
      sample_adjoint<RF>(c.rf, jx, jy, g, q);
      if (s >= a.spp || (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f)) continue;
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      // first walk: N_v into floats 0..2 of vertex v's record, f_v / q_v into 3..5
      int n = 0;
      path_walk(
          pa, idx, o, d, nt, ft, s_dyn + threadIdx.x, nthr,
          [&](int v, const SampleTerms &st, const AppTerms &, const MatVtx &, v3, const float (&)[3]) {
            float tv[3] = {0.f, 0.f, 0.f};
            if (st.has_proj) path_tex(kernarg_shade(), st, a.tex, tv);
            float *rec = s_path + (size_t)(v - 1) * pstride;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rec[ch * nthr] = st.base[ch] * (st.spot[ch] + tv[ch] * st.proj_fac) + (st.spot_b[ch] + tv[ch] * st.proj_fac_b);
            n = v;
          },
          [&](int v, const SampleTerms &, const PathVtx &, const AppTerms &, v3, v3, const float (&)[3], float iq, const float (&f)[3], const PrbBounce &) {
            float *rec = s_path + (size_t)(v - 1) * pstride;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rec[(3 + ch) * nthr] = f[ch] * iq;
          });
      if (n == 0) continue;
      { // the suffix radiances S_v over the N_v (S_n = N_n: the last vertex's f / q may be stale and is not read)
        float S[3] = {0.f, 0.f, 0.f};
        for (int v = n; v >= 1; --v) {
          float *rec = s_path + (size_t)(v - 1) * pstride;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            S[ch] = v < n ? __builtin_fmaf(rec[(3 + ch) * nthr], S[ch], rec[ch * nthr]) : rec[ch * nthr];
            rec[ch * nthr] = S[ch];
          }
        }
      }
      // second walk: the derivatives
      path_walk<true, MAT>(
          pa, idx, o, d, nt, ft, s_dyn + threadIdx.x, nthr,
          [&](int, const SampleTerms &st, const AppTerms &ap, const MatVtx &mv, v3 dv, const float (&beta)[3]) {
            const ShadeK &k = kernarg_shade();
            const float w[3] = {q[0] * beta[0], q[1] * beta[1], q[2] * beta[2]};
            float tv[3] = {0.f, 0.f, 0.f};
            if (st.has_proj) {
              path_tex(k, st, a.tex, tv);
              float cw[3]; // d radiance / d (texture value) per channel, times the sample's gradient: k_path_bwd's sum
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) cw[ch] = w[ch] * (st.base[ch] * st.proj_fac + st.proj_fac_b);
              proj_tex_scatter(k, st, cw, p.gtex);
            }
            if (MAT) { // N_c = sum_e (b_c A_e + B_e) E_ec: the direct-light leaves' reverse passes with the weight q beta
              float gm[FFX_MAT_GRAD_COLS];
              if (emitters_material_vjp(k, st, mv, V3(-dv.x, -dv.y, -dv.z), w, tv, gm)) rs.add_mat(st.shape, gm);
            }
            float gb[3];
            base_colour_vjp(k, st, ap, tv, w, gs, gb);
            rs.add_base(st.shape, ap, gb);
          },
          [&](int v, const SampleTerms &st, const PathVtx &pv, const AppTerms &ap, v3 dv, v3 wo, const float (&beta)[3], float iq, const float (&)[3],
              const PrbBounce &pb) {
            if (v >= n) return; // (no vertex behind this bounce: S_v+1 = 0)
            const float *rec = s_path + (size_t)v * pstride; // vertex v + 1
            float h[3], hb = 0.f; // h_c = q_c beta_v,c S_v+1,c / q_v
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              h[ch] = q[ch] * beta[ch] * iq * rec[ch * nthr];
              hb += h[ch] * st.base[ch];
            }
            if (h[0] == 0.f && h[1] == 0.f && h[2] == 0.f) return;
            float gb[3] = {h[0], h[1], h[2]}; // Lambert rows: f = b
            if (pb.model) { // f_c = (b_c A + B) / cos_o, A = A0 + pi tau / lum(b)
              const float lum = base_lum(st);
              const float r = lum > 0.f ? hb * pb.tau / (lum * lum) : 0.f;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) gb[ch] = (h[ch] * pb.A - r * FFX_LUM_W[ch]) * pb.ic;
              if (MAT) {
                const float *mrow = mat_table(kernarg_shade()) + (size_t)FFX_MAT_STRIDE * st.shape;
                float gm[FFX_MAT_GRAD_COLS];
#pragma unroll
                for (int j = 0; j < FFX_MAT_GRAD_COLS; ++j) gm[j] = 0.f;
                MatGeoD mg;
                material_geometry_d(pv.ns, V3(-dv.x, -dv.y, -dv.z), wo, mg);
                material_terms_vjp(mrow, mg, lum, hb * pb.ic, (h[0] + h[1] + h[2]) * pb.ic, gm);
                rs.add_mat(st.shape, gm);
              }
            }
            rs.add_base(st.shape, ap, gb);
          });
    }
  }
  rs.flush(gs, lane, nthr);
}
template <bool RF>
__global__ void __launch_bounds__(64 * FFX_APP_WAVES)
    k_path_bwd_prb(ShadeK c, AppArgs a, PrbArgs p, const float *__restrict__ gsrc, int stack_ints) {
  extern __shared__ int s_dyn[];
  __shared__ float s_rows[FFX_APP_LDS_ROWS * 3];
  path_bwd_prb<RF, false>(c, a, p, gsrc, s_dyn, stack_ints, s_rows, nullptr);
}
template <bool RF>
__global__ void __launch_bounds__(64 * FFX_APP_WAVES)
    k_path_bwd_prb_material(ShadeK c, AppArgs a, PrbArgs p, const float *__restrict__ gsrc, int stack_ints) {
  extern __shared__ int s_dyn[];
  __shared__ float s_rows[FFX_APP_LDS_ROWS * 3];
  __shared__ float s_mat[FFX_MAT_LDS_ROWS * FFX_MAT_GRAD_COLS];
  path_bwd_prb<RF, true>(c, a, p, gsrc, s_dyn, stack_ints, s_rows, s_mat);
}

// ------------------------------------------------------------------------------------------ forward mode: the tangent image
// FFX_RENDER_TANGENT (include/ffx.h): d image / d theta . dtheta for a tangent dtheta of everything the adjoints above differentiate — the projector's
// texture, the rows' base colours, the spot's intensity, base-colour textures, the BSDF columns.  Every piece is the transpose of the adjoint piece it
// stands next to: vertex_tangent of base_colour_vjp + emitters_material_vjp + proj_tex_scatter, bounce_tangent of path_bwd_prb's bounce.  One wave =
// one pixel (k_path_fwd's layout), one walk per sample that carries the throughput and its tangent; no atomics: the box film takes the fixed-order
// wave sum, the gaussian film rf_fold's sums and k_rf_gather, so two runs give the same bits.
struct JvpArgs {
  const float *tex, *dtex;                           // the projector's texture and its tangent (NULL without a projector)
  const float *drow, *dspot, *dbt[FFX_MAX_BASE_TEX]; // the tangents in the appearance block's layout: [n_shapes][3], [3], [h][w][3] per base-colour texture
  const float *dmat;                                 // [n_shapes][FFX_MAT_GRAD_COLS], or NULL: a table without material columns
  float *dimg, *part;                                // the tangent image (box film) / the pixels' [25][4] outgoing sums (gaussian film)
};
// (kernels <RF, MAT>: the BSDF's reverse passes cost registers — 2 waves per SIMD through the bounces against 4 without them)
// what a vertex's bounce needs of its tangents: the base colour's, its luminance-weighted sum, the row's material tangent (NULL: a Lambert row)
struct VtxTan { float db[3], lum, wdb; const float *md; };
// the tangent of (A, B) of material_terms along the row's tangent md: the reverse pass seeded with (1, 0) and with (0, 1), dotted with md
__device__ __forceinline__ void material_terms_jvp(const float *__restrict__ mrow, const MatGeoD &mg, float lum, const float *__restrict__ md, float &dA, float &dB) {
  float gA[FFX_MAT_GRAD_COLS], gB[FFX_MAT_GRAD_COLS];
#pragma unroll
  for (int j = 0; j < FFX_MAT_GRAD_COLS; ++j) gA[j] = gB[j] = 0.f;
  material_terms_vjp(mrow, mg, lum, 1.f, 0.f, gA);
  material_terms_vjp(mrow, mg, lum, 0.f, 1.f, gB);
  dA = dB = 0.f;
#pragma unroll
  for (int j = 0; j < FFX_MAT_GRAD_COLS; ++j) {
    const float t = md[j];
    dA = __builtin_fmaf(gA[j], t, dA);
    dB = __builtin_fmaf(gB[j], t, dB);
  }
}
// the next-event term N_c = b_c E_c + F_c of a vertex and its tangent (wv: towards the viewer):
//   dN_c = db_c E_c - b_c T_c (w . db) / lum^2 + dI_c (b_c s_f + s_fb) + dtex_c (b_c proj_fac + proj_fac_b) + sum_e (b_c dA_e + dB_e) E_ec
// (E, T, s_f: base_colour_vjp's; E_ec: emitters_material_vjp's; the last sum with MAT only).  vt receives what bounce_tangent needs
template <bool MAT>
__device__ __forceinline__ void vertex_tangent(const ShadeK &k, const JvpArgs &j, const SampleTerms &st, const AppTerms &ap, const MatVtx &mv, v3 wv, VtxTan &vt,
                                               float (&N)[3], float (&dN)[3]) {
  if (ap.tix == 0) { // the row's own base colour
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) vt.db[ch] = j.drow[(size_t)st.shape * 3 + ch];
  } else { // a base-colour texture: the tangent texture through the lookup's four taps
    const float *dt = ap.tix == 1 ? j.dbt[0] : ap.tix == 2 ? j.dbt[1] : ap.tix == 3 ? j.dbt[2] : j.dbt[3];
    size_t to[4];
    float tw4[4];
    base_tex_taps(k, ap.tix - 1, ap.slot, ap.bu, ap.bv, to, tw4);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) vt.db[ch] = tw4[0] * dt[to[0] + ch] + tw4[1] * dt[to[1] + ch] + tw4[2] * dt[to[2] + ch] + tw4[3] * dt[to[3] + ch];
  }
  const float *mt = mat_table(k);
  const bool model = principled_row(k, mt, st.shape);
  vt.md = MAT && model ? j.dmat + (size_t)st.shape * FFX_MAT_GRAD_COLS : nullptr;
  vt.lum = base_lum(st);
  vt.wdb = lum3(vt.db[0], vt.db[1], vt.db[2]);
  N[0] = N[1] = N[2] = 0.f;
  dN[0] = dN[1] = dN[2] = 0.f;
  // no emitter lights the vertex.  (MAT: by the emitters' own factors — a row whose A and B both vanish, as at spec_trans = 1 with eta = 1, still has
  // one-sided BSDF tangents)
  if (!st.has_proj && (MAT ? mv.ks == 0.f : ap.s_f == 0.f && ap.s_fb == 0.f)) return;
  float tv[3] = {0.f, 0.f, 0.f}, dtv[3] = {0.f, 0.f, 0.f};
  if (st.has_proj) {
    path_tex(k, st, j.tex, tv);
    path_tex(k, st, j.dtex, dtv);
  }
  const float r = vt.lum > 0.f ? vt.wdb / (vt.lum * vt.lum) : 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float E = st.spot[ch] + tv[ch] * st.proj_fac, T = k.s_int[ch] * ap.spot_t + tv[ch] * ap.proj_t;
    N[ch] = st.base[ch] * E + (st.spot_b[ch] + tv[ch] * st.proj_fac_b);
    dN[ch] = vt.db[ch] * E - st.base[ch] * T * r + j.dspot[ch] * (st.base[ch] * ap.s_f + ap.s_fb) + dtv[ch] * (st.base[ch] * st.proj_fac + st.proj_fac_b);
  }
  if (!MAT || !vt.md) return;
  const float *mrow = mt + (size_t)FFX_MAT_STRIDE * st.shape;
  MatGeoD mg;
  float dA, dB;
  if (mv.kp != 0.f) {
    material_geometry_d(mv.ns, wv, mv.wp, mg);
    material_terms_jvp(mrow, mg, vt.lum, vt.md, dA, dB);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dN[ch] += (st.base[ch] * dA + dB) * (tv[ch] * mv.kp);
  }
  if (mv.ks != 0.f) {
    material_geometry_d(mv.ns, wv, mv.ws, mg);
    material_terms_jvp(mrow, mg, vt.lum, vt.md, dA, dB);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dN[ch] += (st.base[ch] * dA + dB) * (k.s_int[ch] * mv.ks);
  }
}
// the tangent of the bounce weight f_c = (b_c A + B) / cos_o, A = A0 + pi tau / lum(b) (Lambert rows: f = b) at vertex pv towards wo
__device__ __forceinline__ void bounce_tangent(const ShadeK &k, const SampleTerms &st, const PathVtx &pv, v3 wv, v3 wo, const PrbBounce &pb, const VtxTan &vt,
                                               float (&df)[3]) {
  df[0] = vt.db[0]; df[1] = vt.db[1]; df[2] = vt.db[2];
  if (!pb.model) return;
  const float r = vt.lum > 0.f ? vt.wdb * pb.tau / (vt.lum * vt.lum) : 0.f;
  float dA = 0.f, dB = 0.f;
  if (vt.md) {
    MatGeoD mg;
    material_geometry_d(pv.ns, wv, wo, mg);
    material_terms_jvp(mat_table(k) + (size_t)FFX_MAT_STRIDE * st.shape, mg, vt.lum, vt.md, dA, dB);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) df[ch] = (vt.db[ch] * pb.A + st.base[ch] * (dA - r) + dB) * pb.ic;
}
// one pixel's tangent.  PATH: through the bounces, dL += dbeta_v N_v + beta_v dN_v, dbeta_v+1 = (dbeta_v f_v + beta_v df_v) / q_v with the roulette's
// q_v and both termination tests constants (prb's detached roulette); else direct light at the primary hit, by bwd_leaves' walk
// MAT: the table has material columns (the material block is there); else the BSDF's tangents are not formed
template <bool RF, bool PATH, bool MAT>
__device__ __forceinline__ void jvp_pixel(const ShadeK &c, const PathArgs &a, const JvpArgs &j, int *s_dyn, float *s_rf) {
  const int lane = threadIdx.x;
  const uint32_t pix = blockIdx.x;
  const int W = c.cam.W, px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < (a.spp + 63) >> 6; ++pass) {
    const int s = pass * 64 + lane;
    const uint32_t idx = pix * (uint32_t)a.spp + (uint32_t)s;
    float jx, jy;
    sample_jitter(a.seed_key, idx, jx, jy);
    float dL[3] = {0.f, 0.f, 0.f};
    if (s < a.spp) {
      v3 o, d;
      float nt, ft;
      cam_ray(c.cam, ((float)px + jx) * c.cam.inv_w, ((float)py + jy) * c.cam.inv_h, o, d, nt, ft);
      VtxTan vt;
      float N[3], dN[3];
      if (PATH) {
        float bd[3] = {0.f, 0.f, 0.f}; // the throughput's tangent
        path_walk<true, MAT>(
            a, idx, o, d, nt, ft, s_dyn + lane, 64,
            [&](int, const SampleTerms &st, const AppTerms &ap, const MatVtx &mv, v3 dv, const float (&beta)[3]) {
              vertex_tangent<MAT>(kernarg_shade(), j, st, ap, mv, V3(-dv.x, -dv.y, -dv.z), vt, N, dN);
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) dL[ch] += bd[ch] * N[ch] + beta[ch] * dN[ch];
            },
            [&](int, const SampleTerms &st, const PathVtx &pv, const AppTerms &, v3 dv, v3 wo, const float (&beta)[3], float iq, const float (&f)[3],
                const PrbBounce &pb) {
              float df[3];
              bounce_tangent(kernarg_shade(), st, pv, V3(-dv.x, -dv.y, -dv.z), wo, pb, vt, df);
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) bd[ch] = (bd[ch] * f[ch] + beta[ch] * df[ch]) * iq;
            });
      } else {
        SampleTerms st;
        AppTerms ap;
        MatVtx mv;
        shade_sample<false, true, MAT>(kernarg_shade(), a.nodes, a.recs, a.nrec, o, d, nt, ft, st, s_dyn + lane, 64, nullptr, &ap, &mv);
        if (st.hit && (st.has_proj || (MAT ? mv.ks != 0.f : ap.s_f != 0.f || ap.s_fb != 0.f))) { // (lit: st.base is then the row's)
          vertex_tangent<MAT>(kernarg_shade(), j, st, ap, mv, V3(-d.x, -d.y, -d.z), vt, N, dN);
          dL[0] = dN[0]; dL[1] = dN[1]; dL[2] = dN[2];
        }
      }
    }
    if (RF) {
      float gx[5], gy[5];
      rf_weights(c.rf, jx, gx);
      rf_weights(c.rf, jy, gy);
      rf_fold(s_rf, lane, gx, gy, dL[0], dL[1], dL[2], s < a.spp ? 1.f : 0.f, acc);
    } else {
      acc[0] += dL[0]; acc[1] += dL[1]; acc[2] += dL[2];
    }
  }
  if (RF) {
    rf_store(j.part, pix, lane, acc);
    return;
  }
  const float inv_spp = 1.0f / (float)a.spp;
  const float m0 = wave_sum_tree(acc[0]) * inv_spp, m1 = wave_sum_tree(acc[1]) * inv_spp, m2 = wave_sum_tree(acc[2]) * inv_spp;
  if (lane == 0) {
    float *p = j.dimg + (size_t)pix * 3;
    p[0] = m0; p[1] = m1; p[2] = m2;
  }
}
// RF: the gaussian film — the tangent's sums into j.part, k_rf_gather forms the tangent image (the weights carry no tangent: dI = sum w dL / sum w)
template <bool RF, bool MAT>
__global__ void __launch_bounds__(64)
    k_render_jvp(ShadeK c, PathArgs a, JvpArgs j) {
  extern __shared__ int s_dyn[];
  __shared__ __attribute__((aligned(16))) float s_rf[RF ? FFX_RF_FLOATS : 4];
  jvp_pixel<RF, false, MAT>(c, a, j, s_dyn, s_rf);
}
template <bool RF, bool MAT>
__global__ void __launch_bounds__(64)
    k_path_jvp(ShadeK c, PathArgs a, JvpArgs j) {
  extern __shared__ int s_dyn[];
  __shared__ __attribute__((aligned(16))) float s_rf[RF ? FFX_RF_FLOATS : 4];
  jvp_pixel<RF, true, MAT>(c, a, j, s_dyn, s_rf);
}

// ------------------------------------------------------------------------------------------ FFX_RENDER_AOV
// FFX_RENDER_AOV (include/ffx.h): what the camera sees at the primary hit, through the render's film over the render's samples.  The
// block's 17 floats are handled in GROUPS of three channels (the last holds two) — what rf_fold carries beside the weight, and what keeps a group's
// values, not the block's, live beside the walk.
#define FFX_AOV_GROUPS ((FFX_RENDER_AOV_FLOATS + 2) / 3)
#define FFX_AOV_PITCH (3 * FFX_AOV_GROUPS) // floats per pixel of the box film's sums in LDS (the block, padded to whole groups)
// channels 3 g .. 3 g + 2 of a sample that hit slot `slot` at distance t along (o, d); g is wave-uniform.  Barycentrics from the camera's apex record
// (u = d . B / d . A, v = d . C / d . A), normals from the update's per-slot records, texture coordinates, material row and base-colour lookup as
// shade_sample reads them
__device__ __forceinline__ void aov_group(const ShadeK &c, const int g, const TriRec *__restrict__ recs, const TriApex *__restrict__ arecs, const float4 *__restrict__ nrec,
                                          const float4 *__restrict__ gn, const Hit &h, const float nt, const v3 o, const v3 d, float (&v)[3]) {
  const int slot = h.slot;
  if (g == 0) {
    v[0] = h.t - nt;
    v[1] = fmaf(h.t, d.x, o.x);
    v[2] = fmaf(h.t, d.y, o.y);
    return;
  }
  if (g == 5) {
    v[0] = (float)recs[slot].shape;
    v[1] = (float)h.prim;
    return;
  }
  const float4 gq = g < 4 ? gn[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
  if (g == 1) {
    v[0] = fmaf(h.t, d.z, o.z);
    v[1] = gq.x;
    v[2] = gq.y;
    return;
  }
  const TriApex &ar = arecs[slot];
  const float det = d.x * ar.A[0] + d.y * ar.A[1] + d.z * ar.A[2];
  const float bu = (d.x * ar.B[0] + d.y * ar.B[1] + d.z * ar.B[2]) / det, bv = (d.x * ar.C[0] + d.y * ar.C[1] + d.z * ar.C[2]) / det;
  const float bw = (1.0f - bu) - bv;
  if (g == 2 || g == 3) {
    v3 ns = V3(gq.x, gq.y, gq.z);
    if ((__float_as_int(gq.w) & FFX_GN_SMOOTH_BIT) != 0 && nrec) {
      const float4 n0 = nrec[3 * (size_t)slot], n1 = nrec[3 * (size_t)slot + 1], n2 = nrec[3 * (size_t)slot + 2];
      const v3 ni = V3(fmaf(bw, n0.x, fmaf(bu, n1.x, bv * n2.x)), fmaf(bw, n0.y, fmaf(bu, n1.y, bv * n2.y)), fmaf(bw, n0.z, fmaf(bu, n1.z, bv * n2.z)));
      const float l2 = vdot(ni, ni);
      if (l2 > 0.f) {
        const float il = 1.0f / sqrtf(l2);
        ns = V3(ni.x * il, ni.y * il, ni.z * il);
      }
    }
    if (g == 2) {
      v[0] = gq.z;
      v[1] = ns.x;
      v[2] = ns.y;
      return;
    }
    v[0] = ns.z;
    if (c.slot_uv) {
      const float *uv = c.slot_uv + 6 * (size_t)slot;
      v[1] = fmaf(bw, uv[0], fmaf(bu, uv[2], bv * uv[4]));
      v[2] = fmaf(bw, uv[1], fmaf(bu, uv[3], bv * uv[5]));
    }
    return;
  }
  // g == 4: the base colour
  const float *row = mat_table(c) + (size_t)c.mat_stride * recs[slot].shape;
  v[0] = row[0]; v[1] = row[1]; v[2] = row[2];
  if (c.mat_stride == FFX_MAT_STRIDE && c.n_base_tex > 0) {
    const int tix = (int)row[FFX_MAT_BASE_TEX];
    if (tix > 0 && tix <= c.n_base_tex) base_tex_sample(c, tix - 1, slot, bu, bv, v);
  }
}

// K7's packet form (k_trace_primary_pk: a wave owns a compact block of bw x bh pixels with spp_w sample slots each, one pixel and 64 samples per pass from
// 33 samples per pixel up; candidates from the camera's tile bins, the tree walk when there are none) with the film behind it.
//   box film (RF = false): every group of every pass, one launch.  A pixel's samples sit in spp_w neighbouring lanes: an xor butterfly inside the group
//     (fixed order), the passes' sums added in order in LDS, the means stored as whole blocks — no atomics, the same bits on every run.
//   gaussian film (RF = true): group `group` alone — its three values and the weight through rf_fold / rf_fold_blk into `out` = the film's scratch
//     ([pixel][25][4]), as the render kernels leave the radiance there; k_aov_gather forms the channels.  One launch per group: the scratch holds one.
// The kernel's ONE argument, read in place like ShadeK (kernarg_first): a phase takes a fresh view of it and re-reads what it needs with scalar
// loads, so the walk's scalar registers do not also carry the pointers and counts of the phases around it (as by-value arguments they did: 29
// scalars spilled into vector lanes, and those vectors into scratch)
struct AovK {
  ShadeK c;
  const BvhNode *nodes; const TriRec *recs; const TriApex *arecs; WideScene ws;
  int spp; uint32_t seed_key; int bw_log2, bh_log2, blocks_x, n_blocks;
  const float4 *nrec, *gn;
  float *out; int group;
};
template <bool WIDE, bool RF>
__global__ void __launch_bounds__(PK_BLOCK) __attribute__((amdgpu_waves_per_eu(FFX_PK_MAT_WAVES, FFX_PK_MAT_WAVES)))
    k_render_aov(AovK args) {
  constexpr int WSTACK_N = WIDE ? FFX_WSTACK : 1, RF_N = (FFX_RF_FLOATS * 4 + 7) / 8;
  __shared__ __attribute__((aligned(16))) uint2 s_wstack[RF ? (WSTACK_N > RF_N ? WSTACK_N : RF_N) : WSTACK_N]; // (RF: the filter's rows alias the walk's stack)
  __shared__ float s_acc[RF ? 4 * 64 : 8 * FFX_AOV_PITCH]; // (box film: up to 8 pixels' sums; gaussian film: rf_fold's four sums per lane between the passes)
  const int blk = __builtin_amdgcn_readfirstlane(blockIdx.x);
  // what a lane derives from its number — its pixel of the block, its sample slot, the sample's jitter and ray — is formed in front of the walk and
  // AGAIN behind it, from a copy of the lane number the compiler cannot see through (the same instructions: the same bits): nothing per-lane stays
  // live across the walk, which takes every register of the budget
  struct Sample { int pl, sl, x, y, bx0, by0; bool active; uint32_t pix; float jx, jy, nt, ft; v3 o, d; };
  auto sample_of = [&](const AovK &a, int lane_, int pass) {
    Sample q;
    const int ppw_log2 = a.bw_log2 + a.bh_log2, spp_w = 64 >> ppw_log2;
    q.bx0 = (blk % a.blocks_x) << a.bw_log2;
    q.by0 = (blk / a.blocks_x) << a.bh_log2;
    q.pl = lane_ >> (6 - ppw_log2);
    q.sl = lane_ & (spp_w - 1);
    q.x = q.bx0 + (q.pl & ((1 << a.bw_log2) - 1));
    q.y = q.by0 + (q.pl >> a.bw_log2);
    q.pix = (uint32_t)q.y * (uint32_t)a.c.cam.W + (uint32_t)q.x;
    const int sidx = pass * spp_w + q.sl;
    q.active = q.x < a.c.cam.W && q.y < a.c.cam.H && sidx < a.spp;
    sample_jitter(a.seed_key, q.pix * (uint32_t)a.spp + (uint32_t)sidx, q.jx, q.jy);
    cam_ray(a.c.cam, ((float)q.x + q.jx) * a.c.cam.inv_w, ((float)q.y + q.jy) * a.c.cam.inv_h, q.o, q.d, q.nt, q.ft);
    return q;
  };
  auto lane_again = [] {
    int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    return l;
  };
  int passes;
  {
    const AovK &a = kernarg_first<AovK>();
    if (blk >= a.n_blocks) return; // whole wave
    const int spp_w = 64 >> (a.bw_log2 + a.bh_log2); // sample slots of one pixel per pass
    passes = (a.spp + spp_w - 1) / spp_w; // (more than one only for a wave that owns ONE pixel: the host gives a block's pixels >= spp slots)
  }
  for (int i = threadIdx.x & 63; i < (RF ? 4 * 64 : 8 * FFX_AOV_PITCH); i += 64) s_acc[i] = 0.f;
  __builtin_amdgcn_wave_barrier();
  for (int pass = 0; pass < passes; ++pass) {
    Hit h;
    bool hit;
    {
      const AovK &a = kernarg_first<AovK>();
      const Sample q = sample_of(a, threadIdx.x & 63, pass);
      const v3 o = q.o, d = q.d;
      const float nt = q.nt, ft = q.ft;
      const bool active = q.active;
      bool fnd;
      bool binned = false;
      if (a.c.bins.g[0].on) binned = bins_block(a.c.bins, q.bx0, q.by0, 1 << a.bw_log2, 1 << a.bh_log2, a.arecs, d, nt, ft, wballot(active), h);
      if (!binned) traverse_packet_any<false, WIDE>(a.nodes, a.arecs, a.ws, s_wstack, o, d, nt, ft, active, h, fnd);
      hit = active && h.prim >= 0;
    }
    const AovK &a = kernarg_first<AovK>();
    const int lane = lane_again();
    const Sample q = sample_of(a, lane, pass);
    const int ppw_log2 = a.bw_log2 + a.bh_log2;
    if constexpr (RF) {
      float v[3] = {0.f, 0.f, 0.f};
      if (hit) aov_group(a.c, a.group, a.recs, a.arecs, a.nrec, a.gn, h, q.nt, q.o, q.d, v);
      float gx[5], gy[5];
      rf_weights(a.c.rf, q.jx, gx);
      rf_weights(a.c.rf, q.jy, gy);
      if (ppw_log2 > 0) { // (a single pass)
        rf_fold_blk(reinterpret_cast<float *>(s_wstack), lane, gx, gy, v[0], v[1], v[2], q.active ? 1.f : 0.f, ppw_log2, a.bw_log2, q.bx0, q.by0, a.c.cam.W, a.c.cam.H,
                    a.out);
        return;
      }
      // (one pixel per wave: rf_fold's sums over the passes wait in LDS, four floats per lane)
      float acc[4] = {s_acc[lane], s_acc[64 + lane], s_acc[128 + lane], s_acc[192 + lane]};
      rf_fold(reinterpret_cast<float *>(s_wstack), lane, gx, gy, v[0], v[1], v[2], q.active ? 1.f : 0.f, acc);
      if (pass + 1 == passes) {
        rf_store(a.out, q.pix, lane, acc);
      } else {
        s_acc[lane] = acc[0]; s_acc[64 + lane] = acc[1]; s_acc[128 + lane] = acc[2]; s_acc[192 + lane] = acc[3];
      }
    } else {
      const int spp_w = 64 >> ppw_log2;
#pragma unroll 1
      for (int g = 0; g < FFX_AOV_GROUPS; ++g) {
        float v[3] = {0.f, 0.f, 0.f};
        if (hit) aov_group(a.c, g, a.recs, a.arecs, a.nrec, a.gn, h, q.nt, q.o, q.d, v);
        for (int m = 1; m < spp_w; m <<= 1) {
          v[0] += __shfl_xor(v[0], m, 64);
          v[1] += __shfl_xor(v[1], m, 64);
          v[2] += __shfl_xor(v[2], m, 64);
        }
        if (q.sl == 0) {
          float *s = s_acc + q.pl * FFX_AOV_PITCH + 3 * g;
          s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
        }
      }
    }
  }
  if constexpr (!RF) {
    __builtin_amdgcn_wave_barrier();
    const AovK &a = kernarg_first<AovK>();
    const int ppw_log2 = a.bw_log2 + a.bh_log2, W = a.c.cam.W, H = a.c.cam.H;
    const int bx0 = (blk % a.blocks_x) << a.bw_log2, by0 = (blk / a.blocks_x) << a.bh_log2;
    const float fspp = (float)a.spp;
    for (int i = lane_again(); i < (FFX_RENDER_AOV_FLOATS << ppw_log2); i += 64) { // the block's pixels, 17 consecutive floats each
      const int q = i / FFX_RENDER_AOV_FLOATS, ch = i - q * FFX_RENDER_AOV_FLOATS;
      const int qx = bx0 + (q & ((1 << a.bw_log2) - 1)), qy = by0 + (q >> a.bw_log2);
      if (qx < W && qy < H) a.out[((size_t)qy * W + qx) * FFX_RENDER_AOV_FLOATS + ch] = s_acc[q * FFX_AOV_PITCH + ch] / fspp;
    }
  }
}
// k_rf_gather for three (n_ch < 3: fewer) channels of the block: a pixel's 25 incoming sums, the same staging through LDS and the same order of
// additions; what differs is the store — channels ch0 .. ch0 + n_ch - 1 of a 17-float pixel instead of the film's 3-float pixel
__global__ void __launch_bounds__(64) k_aov_gather(const float4 *__restrict__ part, int W, int H, float *__restrict__ aov, int ch0, int n_ch) {
  __shared__ float4 seg[68 * 5];
  const int lane = threadIdx.x;
  const int x0 = blockIdx.x * 64, y = blockIdx.y;
  float r, g, b, w;
  rf_window_sums(part, W, H, x0, y, lane, seg, r, g, b, w);
  const int x = x0 + lane;
  if (x >= W) return;
  float *p = aov + ((size_t)y * W + x) * FFX_RENDER_AOV_FLOATS + ch0;
  p[0] = w > 0.f ? r / w : 0.f;
  if (n_ch > 1) p[1] = w > 0.f ? g / w : 0.f;
  if (n_ch > 2) p[2] = w > 0.f ? b / w : 0.f;
}

// ------------------------------------------------------------------------------------------ host side
static int cam_prepare(const ffx_camera *c, CamK &k) {
  if (c->width < 1 || c->height < 1) return 0;
  if (!ffx_inv4(c->camera_to_sample, k.s2c)) return 0;
  for (int i = 0; i < 12; ++i) k.tw[i] = c->to_world[i];
  k.near_clip = c->near_clip;
  k.far_clip = c->far_clip;
  k.W = c->width;
  k.H = c->height;
  k.inv_w = 1.0f / (float)c->width;
  k.inv_h = 1.0f / (float)c->height;
  k.w_uniform = (k.s2c[12] == 0.f && k.s2c[13] == 0.f && k.s2c[15] != 0.f) ? 1 : 0;
  k.iw_u = k.w_uniform ? 1.0f / k.s2c[15] : 0.f;
  return 1;
}

// the material table that travels with the call (ffx_scene_desc.mat_h: n_shapes rows of `ms` floats) into a kernel argument (ShadeK / BwdP / BwdF);
// 0: the table's size is wrong
template <class K> static int copy_mat_h(const ffx_scene_desc *sd, int ms, K &k) {
  if (sd->n_mat_h <= 0) return 1;
  if (sd->n_mat_h > FFX_MAX_MAT_H || sd->n_mat_h != sd->n_shapes * ms) return 0;
  k.mat_inline = 1;
  for (int i = 0; i < sd->n_mat_h; ++i) k.mat_h[i] = sd->mat_h[i];
  return 1;
}

// the pre-row p (columns FFX_PRE_*) of the material row m: what RowPre reads in place of RowRaw's per-evaluation forms
static void mat_pre_row(const float *m, float *p) {
  const float eta = m[FFX_MAT_ETA], r2 = m[FFX_MAT_ROUGHNESS] * m[FFX_MAT_ROUGHNESS], a = r2 > 0.001f ? r2 : 0.001f, a2 = a * a;
  const float metallic = m[FFX_MAT_METALLIC], m1 = 1.0f - metallic, tint = m[FFX_MAT_SPEC_TINT];
  const float r0 = (eta - 1.0f) / (eta + 1.0f);
  uint32_t flags = 0;
  if (m[FFX_MAT_ANISOTROPIC] != 0.f) flags |= FFX_PRE_ANISO;
  if (tint != 0.f) flags |= FFX_PRE_TINT;
  if (m[FFX_MAT_CLEARCOAT] > 0.f) flags |= FFX_PRE_CLEARCOAT;
  if (m[FFX_MAT_FLATNESS] > 0.f) flags |= FFX_PRE_FLAT;
  if (m[FFX_MAT_SHEEN] > 0.f && m1 > 0.f) flags |= FFX_PRE_SHEEN;
  p[FFX_PRE_ETA] = eta; p[FFX_PRE_INV_ETA2] = 1.0f / (eta * eta); p[FFX_PRE_A2] = a2; p[FFX_PRE_INV_A2] = 1.0f / a2;
  p[FFX_PRE_METALLIC] = metallic; p[FFX_PRE_C_SW] = metallic + m1 * tint; p[FFX_PRE_C_FD] = m1 * (1.0f - tint); p[FFX_PRE_BRDF] = m1 * (1.0f - m[FFX_MAT_SPEC_TRANS]);
  p[FFX_PRE_ROUGH2] = 2.0f * m[FFX_MAT_ROUGHNESS]; memcpy(&p[FFX_PRE_FLAGS], &flags, 4); p[FFX_PRE_R2] = r2; p[FFX_PRE_TINT_TERM] = m1 * tint * r0 * r0;
}

static int shade_prepare(const ffx_scene_desc *sd, ShadeK &c) {
  memset(&c, 0, sizeof c);
  if (!cam_prepare(&sd->cam, c.cam)) return 0;
  c.proj_on = sd->proj.enabled;
  c.spot_on = sd->spot.enabled;
  c.shadows = sd->shadows & FFX_SHADOWS_ON; // (the word's other bits are hints to the pre-pass and the caches)
  c.mat_stride = sd->mat_stride ? sd->mat_stride : 3;
  if (c.mat_stride != 3 && c.mat_stride != FFX_MAT_STRIDE) return 0;
  if (!copy_mat_h(sd, c.mat_stride, c)) return 0;
  if (c.mat_inline && c.mat_stride == FFX_MAT_STRIDE && sd->n_shapes <= 8) { // per-row constants of the principled rows (ShadeK.mat_pre)
    c.mat_pre_on = 1;
    for (int k = 0; k < sd->n_shapes; ++k) mat_pre_row(sd->mat_h + k * FFX_MAT_STRIDE, c.mat_pre + k * FFX_PRE_FLOATS);
  }
  if (sd->rfilter == FFX_RFILTER_GAUSSIAN) { // [EXT Mitsuba src/rfilters/gaussian.cpp] radius 4 stddev; the 5x5 window holds radius <= 2
    const float sdv = sd->rfilter_stddev > 0.f ? sd->rfilter_stddev : 0.5f;
    if (!(sdv <= 0.5f)) return 0;
    rf_constants(sdv, c.rf);
  } else if (sd->rfilter != FFX_RFILTER_BOX) return 0;
  c.n_base_tex = sd->n_base_tex;
  if (c.n_base_tex < 0 || c.n_base_tex > FFX_MAX_BASE_TEX || (c.n_base_tex > 0 && (c.mat_stride != FFX_MAT_STRIDE || !sd->slot_uv))) return 0;
  c.slot_uv = sd->slot_uv;
  for (int k = 0; k < c.n_base_tex; ++k) {
    c.btex[k] = sd->base_tex[k]; c.btw[k] = sd->base_tex_w[k]; c.bth[k] = sd->base_tex_h[k];
    if (!c.btex[k] || c.btw[k] < 1 || c.bth[k] < 1) return 0;
  }
  float inv[16];
  if (c.proj_on) {
    if (!ffx_inv4(sd->proj.to_world, inv)) return 0;
    for (int i = 0; i < 12; ++i) c.p_w2l[i] = inv[i];
    for (int i = 0; i < 16; ++i) c.p_c2s[i] = sd->proj.camera_to_sample[i];
    c.p_pos[0] = sd->proj.to_world[3]; c.p_pos[1] = sd->proj.to_world[7]; c.p_pos[2] = sd->proj.to_world[11];
    c.p_axis[0] = sd->proj.to_world[2]; c.p_axis[1] = sd->proj.to_world[6]; c.p_axis[2] = sd->proj.to_world[10];
    c.p_scale = sd->proj.scale;
    for (int i = 0; i < 3; ++i) c.p_color[i] = sd->proj.color[i];
    c.tw = sd->proj.tex_w; c.th = sd->proj.tex_h; c.tc = sd->proj.tex_channels;
    if (c.tw < 1 || c.th < 1 || (c.tc != 1 && c.tc != 3)) return 0;
  }
  if (c.spot_on) {
    if (!ffx_inv4(sd->spot.to_world, inv)) return 0;
    for (int i = 0; i < 12; ++i) c.s_w2l[i] = inv[i];
    {
      double worst = 0.0;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double d = 0.0;
          for (int k = 0; k < 3; ++k) d += (double)inv[4 * i + k] * (double)inv[4 * j + k];
          worst = fmax(worst, fabs(d - (i == j ? 1.0 : 0.0)));
        }
      c.s_rigid = worst < 2e-6 ? 1 : 0;
    }
    c.s_pos[0] = sd->spot.to_world[3]; c.s_pos[1] = sd->spot.to_world[7]; c.s_pos[2] = sd->spot.to_world[11];
    for (int i = 0; i < 3; ++i) c.s_int[i] = sd->spot.intensity[i];
    const float deg = 0.017453292519943295f;
    c.cutoff = sd->spot.cutoff_deg * deg;
    float beam = sd->spot.beam_width_deg * deg;
    c.cos_cut = cosf(c.cutoff);
    c.cos_beam = cosf(beam);
    c.inv_trans = 1.0f / (c.cutoff - beam);
  }
  return 1;
}

// Apex records (ffx_common.h): one lane per leaf slot writes the triangle's (A, B, C, T) for each of the
// requested apexes.  Runs in front of every packet render / trace launch on the same stream: the apex
// areas at the end of the blob are scratch owned by the most recent call (calls that share a blob must
// be stream-ordered, as they already are for the records themselves).  53 k triangles x 3 apexes: 7.7 MB.
struct ApexK { float o[FFX_N_APEX][3]; int on[FFX_N_APEX]; };
__global__ void __launch_bounds__(256)
    k_apex_records(const TriRec *__restrict__ recs, int n_tris, ApexK ak, TriApex *__restrict__ out, uint32_t astride, uint32_t *__restrict__ cache_hdr,
                   uint32_t cap_stray) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0 && cache_hdr) { // adjoint cache: stray arena empty (CacheHdr)
    cache_hdr[0] = 0u; cache_hdr[1] = cap_stray & ~FFX_CAP_KEEP_DROPPED;
    if (!(cap_stray & FFX_CAP_KEEP_DROPPED)) cache_hdr[2] = 0u;
    for (int i = 4; i < 12; ++i) cache_hdr[i] = 0u; // (the filtered film's cache: its arena's eight counters)
  }
  if (k >= n_tris) return;
  const float4 *r4 = reinterpret_cast<const float4 *>(recs + k);
  const float4 a = r4[0], b = r4[1], c = r4[2];
  const v3 v0 = V3(a.x, a.y, a.z), e1 = V3(a.w, b.x, b.y), e2 = V3(b.z, b.w, c.x);
#pragma unroll
  for (int j = 0; j < FFX_N_APEX; ++j) {
    if (!ak.on[j]) continue;
    const ApexVec av = apex_vectors(v0, e1, e2, V3(ak.o[j][0], ak.o[j][1], ak.o[j][2]));
    float4 *o4 = reinterpret_cast<float4 *>(reinterpret_cast<char *>(out) + (size_t)j * astride) + 3 * (size_t)k;
    o4[0] = make_float4(av.A.x, av.A.y, av.A.z, av.B.x);
    o4[1] = make_float4(av.B.y, av.B.z, av.C.x, av.C.y);
    o4[2] = make_float4(av.C.z, av.T, c.y, c.z); // prim, shape as in TriRec
  }
}

// FFX_TRAVERSAL=lane selects the per-lane (LDS stack) kernels; default: wave-packet kernels
// (the knobs are read at every launch: cheap, and lets one process exercise every variant)
static int use_packet() {
  const char *e = getenv("FFX_TRAVERSAL");
  return (e && strcmp(e, "lane") == 0) ? 0 : 1;
}

// FFX_WIDE=0 selects the binary packet walks (A/B baseline); default: the 64-wide walk
static int use_wide(const ffx_bvh_info *info) {
  const char *e = getenv("FFX_WIDE");
  return (e && strcmp(e, "0") == 0) || info->off_tq == 0 ? 0 : 1;
}
static WideScene wide_scene(const void *bvh, const ffx_bvh_info *info) {
  WideScene ws;
  const char *base = (const char *)bvh;
  ws.elems = (const WideChild *)(base + info->off_wnodes);
  ws.hdr = (const WideHdr *)(base + info->off_whdr);
  ws.root = info->wide_root;
  ws.tq0 = (uint32_t)((info->off_tq - info->off_wnodes) / sizeof(WideChild));
  return ws;
}

// log2 of the side (in 2x2-pixel tiles) of the square blocks in which tiles are enumerated: FFX_TILE_BLOCK,
// default 4 = 32x32-pixel blocks since the tile bins (round 4: 3 / 4 / 5 = 0.4033 / 0.4001 / 0.42 ms for K8 alone, renders/s 2 469 / 2 500,
// gradient steps/s 2 288 / 2 354, colon 8.39 / 8.31 ms — a block of 16 bin tiles keeps a workgroup round inside fewer tile lists);
// before them 3 = 16x16-pixel blocks (+1 % on both workloads against row-major; the blocked XCD interleave on top of it,
// FFX_XCD_REMAP >= 2: B = 64 / 128 / 256 / 512 / 1024 measured +0.5 / +1 / -1 / -2 / -10 % against the round-robin deal)
// (films above 512 k pixels — config 5: 1024^2 x 256 spp, 141 MB of tile-list entries per pose — keep the round-3 parameters: the larger block and
// the second pixel per wave buy them nothing (8.39 / 8.31 ms) and double the kernel's HBM traffic, 168 -> 343 MB of FETCH_SIZE per launch)
// The kernels that fold footprints (cache / forward + adjoint) take the larger block there too: colon 114.5 -> 126.5 gradient steps/s.
static int tile_block_log2(long pixels = 0, bool with_cache = false) {
  const char *e = getenv("FFX_TILE_BLOCK");
  // (round 5, tools/trafficsweep.sh: 64x64-pixel blocks with 1024 workgroups per XCD and round — half a block, 32 camera tiles, on one L2 — read
  // 45 MB per launch instead of 67 at the same speed (2 530 vs 2 527 - 2 558 renders/s); the floor is 40 MB: the tile lists are 16.6 MB of
  // 64-byte entries that a render reads once, and the counter correction doubles them.  Coarser deals — one block or more per XCD — reach
  // the floor but lose 14 % to load imbalance)
  const int dflt = (pixels > 2L * 512 * 512) ? (with_cache ? 4 : 3) : 5;
  int t = e ? atoi(e) : dflt;
  return (t < 0 || t > 8) ? dflt : t;
}

// pixels of its 2x2 tile a wave of k_render_fwd_pk walks: FFX_PIXELS_PER_WAVE = 1, 2 (default) or 4.
// Measured 4 / 2 / 1: 1133 / 1180 / 1165 renders/s (vocal fold), 62.0 / 62.6 / 62.2 (colon): shorter
// waves even out the tail of the launch, one pixel per wave pays the wave start-up four times.
// default: one pixel per wave for the plain forward (finest grain: +1-2 %), two for the cache-writing forward (whose
// per-pixel footprint bookkeeping amortises better: one pixel per wave was 1.5 % slower there); colon: no difference
static int pixels_per_wave(bool with_cache, long pixels = 0) {
  const char *e = getenv("FFX_PIXELS_PER_WAVE");
  // (round 4, with the tile bins and 32x32-pixel enumeration blocks: two pixels per wave for the plain forward too — 1 / 2 / 4 pixels =
  // 2 450 / 2 610 / 2 600 renders/s over 100 steps, 2 390 / 2 500 / 2 500 over the driver's 20, K8 alone 0.399 / 0.387 / 0.419 ms; colon
  // 117.9 / 118.8 / 106.2 renders/s.  Half as many waves to dispatch, and a wave's second pixel finds its tile list in the L1)
  const int dflt = (with_cache || pixels <= 2L * 512 * 512) ? 2 : 1;
  int w = e ? atoi(e) : dflt;
  return (w == 1 || w == 2 || w == 4) ? w : dflt;
}

// renders below 33 samples per pixel take k_render_fwd_blk (several pixels per wave); FFX_RENDER_BLOCKS=0: a pixel per wave whatever the count
static bool lowspp_blocks() {
  const char *e = getenv("FFX_RENDER_BLOCKS");
  return !(e && strcmp(e, "0") == 0);
}

// k_render_fwd_pk's plain-scene instance for the scenes it covers (plain_scene); FFX_K8_PLAIN=0: the generic instance for every scene (A/B runs, tests)
static bool k8_plain_enabled() {
  const char *e = getenv("FFX_K8_PLAIN");
  return !(e && strcmp(e, "0") == 0);
}

// ---- tile bins: the three grids of a scene description (ffx_common.h BinGrid).  A pure function of sd (and the environment), so that
// ffx_apex_prepare and the render calls that follow it derive the same grids.  A grid is switched off (its packets walk the tree)
// when its projection is not a central perspective, when a spot's cone is too wide for a perspective grid, or by FFX_BINS=0.
static int bins_enabled() {
  const char *e = getenv("FFX_BINS");
  return !(e && strcmp(e, "0") == 0);
}
static int env_pow2(const char *name, int dflt, int lo, int hi) {
  const char *e = getenv(name);
  int v = e ? atoi(e) : dflt;
  if (v < lo || v > hi || (v & (v - 1)) != 0) v = dflt;
  return v;
}
// rows of M for a sensor-like apex: tile coordinates = (film / tile) * sample coordinates of camera_to_sample * world_to_camera
static int grid_from_sensor(const float *to_world, const float *c2s, int width, int height, int tile, BinGrid &g) {
  memset(&g, 0, sizeof g);
  if (width < 1 || height < 1) return 0;
  float w2c[16];
  if (!ffx_inv4(to_world, w2c)) return 0;
  // a central projection: sample = (r0 . p, r1 . p) / (r3 . p) with no dependence on the homogeneous 1 of a camera-space point
  if (c2s[3] != 0.f || c2s[7] != 0.f || c2s[15] != 0.f || !(c2s[14] > 0.f)) return 0;
  while ((width + tile - 1) / tile > 128 || (height + tile - 1) / tile > 128) tile *= 2;
  g.nx = (width + tile - 1) / tile;
  g.ny = (height + tile - 1) / tile;
  if ((long)g.nx * g.ny > FFX_BIN_MAX_TILES) return 0;
  const double sx = (double)width / tile, sy = (double)height / tile;
  for (int j = 0; j < 3; ++j) {
    double x = 0, y = 0, z = 0;
    for (int k = 0; k < 3; ++k) {
      x += (double)c2s[k] * w2c[4 * k + j];
      y += (double)c2s[4 + k] * w2c[4 * k + j];
      z += (double)c2s[12 + k] * w2c[4 * k + j];
    }
    g.M[j] = (float)(sx * x); g.M[3 + j] = (float)(sy * y); g.M[6 + j] = (float)z;
  }
  g.o[0] = to_world[3]; g.o[1] = to_world[7]; g.o[2] = to_world[11];
  g.on = 1;
  return tile;
}
static void bins_grids(const ffx_scene_desc *sd, BinGrid (&g)[FFX_N_APEX], float &cam_its_x, float &cam_its_y) {
  memset(g, 0, sizeof g);
  cam_its_x = cam_its_y = 0.f;
  if (!sd || !bins_enabled()) return;
  const int ts = env_pow2("FFX_BIN_TILE", 8, 4, 32);
  const int tile = grid_from_sensor(sd->cam.to_world, sd->cam.camera_to_sample, sd->cam.width, sd->cam.height, ts, g[0]);
  if (tile > 0) cam_its_x = cam_its_y = 1.0f / (float)tile;
  if (sd->proj.enabled) grid_from_sensor(sd->proj.to_world, sd->proj.camera_to_sample, sd->proj.tex_w, sd->proj.tex_h, env_pow2("FFX_BIN_TILE_PROJ", 2 * ts, 4, 64), g[1]);
  if (sd->spot.enabled && sd->spot.cutoff_deg > 0.f && sd->spot.cutoff_deg <= 75.f) {
    // a square perspective grid around the cone's axis: half angle = cutoff + 1 degree, ~1 degree per tile at the centre
    float w2l[16];
    if (ffx_inv4(sd->spot.to_world, w2l)) {
      const char *e = getenv("FFX_BIN_SPOT_N");
      // (~1 degree per tile; 1.7 degrees under the caller's hint that this pose's renders are short — FFX_SHADOWS_PLAIN, below 33 samples per
      // pixel: such a render waits for the pre-pass chain, and a coarser grid lists a third fewer (triangle, tile) pairs: 16 spp 5 510 ->
      // 6 519 renders/s, 4 spp 5 657 -> 6 556; a long render prefers the finer grid's shorter lists: 64 spp 2 964 against 2 921)
      int n = e ? atoi(e) : (int)(((sd->shadows & FFX_SHADOWS_PLAIN) ? 1.2f : 2.0f) * sd->spot.cutoff_deg + 0.999f);
      n = n < 8 ? 8 : (n > 128 ? 128 : n);
      const double tanc = tan(((double)sd->spot.cutoff_deg + 1.0) * 0.017453292519943295);
      BinGrid &q = g[2];
      for (int j = 0; j < 3; ++j) {
        q.M[j] = (float)(0.5 * n * (w2l[j] / tanc + w2l[8 + j]));
        q.M[3 + j] = (float)(0.5 * n * (w2l[4 + j] / tanc + w2l[8 + j]));
        q.M[6 + j] = w2l[8 + j];
      }
      q.o[0] = sd->spot.to_world[3]; q.o[1] = sd->spot.to_world[7]; q.o[2] = sd->spot.to_world[11];
      q.nx = q.ny = n;
      q.on = 1;
    }
  }
}
// FFX_ENVELOPE=0: no envelopes (every shadow packet runs its any-hit stage: the A/B baseline and the tests' reference).  -> a mask over the
// emitters (bit 0 projector, bit 1 spot).  A pure function of (sd, info, environment), like the grids: the pre-pass and the renders behind it agree.
static int env_enabled(const ffx_scene_desc *sd, const ffx_bvh_info *info) {
  const char *e = getenv("FFX_ENVELOPE");
  if (!(sd && (sd->shadows & FFX_SHADOWS_ON) && bins_enabled() && info->off_bins)) return 0;
  if (sd->shadows & FFX_SHADOWS_PLAIN) return 0; // (the caller's hint: this pose's renders are short — the envelope launch would only lengthen the pre-pass chain)
  if (info->bins_stride < ffx_bin_stride(info->n_tris) || ffx_bin_off_env(info->n_tris) >= (1ull << 32)) return 0; // (a blob of another library version)
  const int m = e ? atoi(e) : 3;
  return (m < 0 || m > 3) ? 0 : m;
}
// the envelope launch's constants for the grids g (ffx_common.h EnvBuild); an emitter whose grid is off or not invertible drops out of the mask
static int env_build(const BinGrid (&g)[FFX_N_APEX], int mask, int n_tris, EnvBuild &eb) {
  memset(&eb, 0, sizeof eb);
  eb.env_off = (uint32_t)ffx_bin_off_env(n_tris);
  eb.kap = (float)((1.0 - (double)SHADOW_EPS) * (1.0 + 6e-5));
  int out = 0;
  for (int a = 1; a < FFX_N_APEX; ++a) {
    if (!((mask >> (a - 1)) & 1) || !g[a].on) continue;
    const float *M = g[a].M;
    const double m[9] = {M[0], M[1], M[2], M[3], M[4], M[5], M[6], M[7], M[8]};
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(fabs(det) > 1e-30)) continue;
    const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    double umax = 0.0; // |Minv (x, y, 1)| is convex in (x, y): its maximum over the grid sits at a corner
    for (int c = 0; c < 4; ++c) {
      const double x = (c & 1) ? g[a].nx : 0.0, y = (c & 2) ? g[a].ny : 0.0;
      const double ux = inv[0] * x + inv[1] * y + inv[2], uy = inv[3] * x + inv[4] * y + inv[5], uz = inv[6] * x + inv[7] * y + inv[8];
      umax = fmax(umax, sqrt(ux * ux + uy * uy + uz * uz));
    }
    for (int k = 0; k < 9; ++k) eb.Minv[a][k] = (float)inv[k];
    eb.graz[a] = (float)(umax * 1.001 / 40.0);
    eb.on[a] = 1;
    out |= 1 << (a - 1);
  }
  return out;
}
// the kernels' view of the bins of `sd` in the blob (grids as bins_grids gives them; built by launch_apex / ffx_apex_prepare)
static void bins_k(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, BinsK &bk) {
  memset(&bk, 0, sizeof bk);
  if (!info->off_bins || !info->bins_stride) return;
  bins_grids(sd, bk.g, bk.cam_inv_ts_x, bk.cam_inv_ts_y);
  for (int a = 0; a < FFX_N_APEX; ++a) bk.base[a] = (const char *)bvh + info->off_bins + (uint64_t)a * info->bins_stride;
  EnvBuild eb;
  bk.env_on = env_build(bk.g, env_enabled(sd, info), info->n_tris, eb);
  bk.env_off = eb.env_off;
}

// fills the blob's apex areas for the camera (and the enabled emitters of sd, if given) on stream s
// (cap_stray's top bit: FFX_RENDER_CACHE_KEEP_DROPPED — the arena is emptied, the header's `dropped` count stays: ffx_common.h FFX_CAP_KEEP_DROPPED)
__global__ void k_cache_reset(uint32_t *__restrict__ cache_hdr, uint32_t cap_stray) {
  cache_hdr[0] = 0u; cache_hdr[1] = cap_stray & ~FFX_CAP_KEEP_DROPPED;
  if (!(cap_stray & FFX_CAP_KEEP_DROPPED)) cache_hdr[2] = 0u;
  for (int i = 4; i < 12; ++i) cache_hdr[i] = 0u; // (the filtered film's cache: its arena's eight counters)
}
// flags: FFX_RENDER_APEX_READY — the areas already hold this call's apexes (ffx_apex_prepare, or an earlier call with the same
// origins on records that have not changed since): no launch; FFX_RENDER_CACHE_ZEROED — the caller has cleared the cache header.
static int launch_apex(const void *bvh, const ffx_bvh_info *info, const float *cam_to_world, const ffx_scene_desc *sd, const TriApex **arecs,
                       uint32_t *astride, hipStream_t s, void *cache = nullptr, uint32_t cap_stray = 0, int flags = 0) {
  ApexK ak;
  memset(&ak, 0, sizeof ak);
  ak.on[0] = 1;
  ak.o[0][0] = cam_to_world[3]; ak.o[0][1] = cam_to_world[7]; ak.o[0][2] = cam_to_world[11];
  if (sd && sd->proj.enabled) {
    ak.on[1] = 1;
    ak.o[1][0] = sd->proj.to_world[3]; ak.o[1][1] = sd->proj.to_world[7]; ak.o[1][2] = sd->proj.to_world[11];
  }
  if (sd && sd->spot.enabled) {
    ak.on[2] = 1;
    ak.o[2][0] = sd->spot.to_world[3]; ak.o[2][1] = sd->spot.to_world[7]; ak.o[2][2] = sd->spot.to_world[11];
  }
  const uint64_t stride = ffx_apex_stride(info->n_tris);
  if (info->total_bytes < info->off_recs + FFX_N_APEX * stride || stride >= (1ull << 32)) {
    ffx_set_error("blob has no apex areas (built by another library version?)");
    return 0;
  }
  TriApex *out = (TriApex *)((char *)bvh + ffx_apex_offset(info, 0));
  const TriRec *recs = (const TriRec *)((const char *)bvh + info->off_recs);
  if (flags & FFX_RENDER_CACHE_ZEROED) cache = nullptr;
  if (flags & FFX_RENDER_CACHE_KEEP_DROPPED) cap_stray |= FFX_CAP_KEEP_DROPPED; // (the reset launches' view of the flag; capacities stay far below 2^31)
  if (!(flags & FFX_RENDER_APEX_READY)) {
    // ONE pre-pass for both: the counting launch of the tile bins writes the apex records too (ffx_bins.hip k_bin<false>), the fill
    // launch follows when a grid is on.  A blob without a bins area (or a primary-visibility call: sd == NULL) gets the apex records alone.
    BinBuild bb;
    memset(&bb, 0, sizeof bb);
    if (sd && info->off_bins && info->bins_stride >= ffx_bin_stride(info->n_tris)) {
      float ix, iy;
      bins_grids(sd, bb.g, ix, iy);
      for (int a = 0; a < FFX_N_APEX; ++a) bb.base[a] = (char *)bvh + info->off_bins + (uint64_t)a * info->bins_stride;
      bb.cap = (uint32_t)ffx_bin_cap(info->n_tris);
      if (const char *ce = getenv("FFX_BIN_CAP")) { // (test knob, include/ffx.h: a smaller capacity makes a grid's lists overflow — its packets then walk the tree)
        const long cv = atol(ce);
        if (cv >= 0 && (uint64_t)cv < bb.cap) bb.cap = (uint32_t)cv;
      }
      bb.arrive = (uint32_t *)(bb.base[0] + offsetof(BinHdr, pad0));
    }
    if (!bb.arrive) { // no bins area to hold the arrival counter: the plain apex launch
      hipLaunchKernelGGL(k_apex_records, dim3(ffx_cdiv(info->n_tris, 256)), dim3(256), 0, s, recs, info->n_tris, ak, out, (uint32_t)stride, (uint32_t *)cache, cap_stray);
    } else {
      // (the render kernels these launches will run beside: material rows -> seven waves of 72 VGPRs per SIMD, Lambert -> eight of 64)
      EnvBuild eb;
      const int env_mask = env_build(bb.g, env_enabled(sd, info), info->n_tris, eb);
      bb.env_mask = env_mask;
      ffx_bins_launch(recs, info->n_tris, bb, out, ak.o, ak.on, (uint32_t)stride, (uint32_t *)cache, cap_stray, s, sd && sd->mat_stride != FFX_MAT_STRIDE,
                      env_mask ? &eb : nullptr);
    }
  } else if (cache)
    hipLaunchKernelGGL(k_cache_reset, dim3(1), dim3(1), 0, s, (uint32_t *)cache, cap_stray);
  *arecs = out;
  *astride = (uint32_t)stride;
  return 1;
}

// default 128 workgroups per XCD per round of the blocked interleave; 256 for films above 512 k pixels: with four times the tiles the
// load still balances at the coarser grain and each L2 walks a smaller part of a larger scene (tools/xcdsweep_colon.sh, config 5:
// 64 / 128 / 256 / 512 / 1024 / 2048 = 90.1 / 90.2 / 89.7 / 88.2 / 84.2 / 67.7 renders/s at 181 / 128 / 80 / 64 / 56 / 54 MB of raw
// FETCH_SIZE per launch; the vocal fold at 512x512 loses 1 % at 256)
static int xcd_mode(long pixels = 0) {
  const char *e = getenv("FFX_XCD_REMAP");
  int m = e ? atoi(e) : (pixels > 2L * 512 * 512 ? 256 : 1024);
  return m < 0 ? 0 : m;
}

static inline uint32_t seed_key_of(uint32_t seed) { return hash32(seed + 0x9e3779b9U); }

static int check_info(const ffx_bvh_info *info, const char *what) {
  if (info->n_tris < 1 || info->n_nodes < 1 || info->max_depth < 1 || info->max_depth > FFX_STACK_DEPTH) {
    ffx_set_error("%s: bad bvh info (n_tris %d, n_nodes %d, max_depth %d)", what, info->n_tris, info->n_nodes, info->max_depth);
    return 0;
  }
  return 1;
}
static inline size_t stack_bytes(const ffx_bvh_info *info) {
  int depth = info->max_depth < 8 ? 8 : info->max_depth;
  return (size_t)depth * TR_BLOCK * sizeof(int);
}

#ifdef FFX_STATS
#endif
#ifdef FFX_BINCHECK
extern "C" int ffx_debug_bincheck(unsigned long long *out24, int reset) {
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_ffx_chk), sizeof(unsigned long long) * 24) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[24] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ffx_chk), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#ifdef FFX_TIMERS
extern "C" int ffx_debug_timers(unsigned long long *out32, int reset) {
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_ffx_tim), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ffx_tim), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#ifdef FFX_STATS
extern "C" int ffx_debug_stats(unsigned long long *out16, int reset) { // the tree walks' counters [0, 32); resets all 48
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ffx_stats), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[48] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ffx_stats), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
extern "C" int ffx_debug_stats48(unsigned long long *out48, int reset) { // ... with the tile bins' counters [32, 48)
  if (hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_ffx_stats), sizeof(unsigned long long) * 48) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[48] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ffx_stats), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// ---- what the render calls share: the blob's areas, one setup per call, the grids, the gaussian film's steps, one launcher per kernel family
struct BlobView { const BvhNode *nodes; const TriRec *recs; const float4 *nrec, *gn; }; // nrec: vertex normals per slot (ffx_smooth), gn: unit geometric normals per slot
static BlobView blob_view(const void *bvh, const ffx_bvh_info *info) {
  const char *b = (const char *)bvh;
  return {(const BvhNode *)(b + info->off_nodes), (const TriRec *)(b + info->off_recs), info->off_nrec ? (const float4 *)(b + info->off_nrec) : nullptr,
          info->off_gn ? (const float4 *)(b + info->off_gn) : nullptr};
}

// the path integrator's depths from a flags word (include/ffx.h FFX_RENDER_PATH): 0 = a bad field, else 1 with max_depth (2: direct light only, the
// existing kernels) and rr_depth
static int path_depths(int flags, int &max_depth, int &rr_depth) {
  const int md = (flags >> FFX_RENDER_MAX_DEPTH_SHIFT) & 15, rr = (flags >> FFX_RENDER_RR_DEPTH_SHIFT) & 15;
  max_depth = md == 0 ? 2 : md;
  rr_depth = rr == 0 ? 5 : rr;
  return max_depth >= 2 && max_depth <= FFX_RENDER_MAX_DEPTH_LIMIT;
}
static inline size_t path_stack_bytes(const ffx_bvh_info *info) { return (size_t)(info->max_depth < 8 ? 8 : info->max_depth) * 64 * sizeof(int); }

// the scene's reconstruction filter against the entry point (`what`: "render_fwd" / "render_bwd"): the gaussian film's calls take a scratch and the wide packet kernels
static int check_filter(const char *what, const ffx_scene_desc *sd, const ffx_bvh_info *info, const void *rf_scratch) {
  if (rf_scratch && sd->rfilter == FFX_RFILTER_BOX) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s_filtered: rfilter must be FFX_RFILTER_GAUSSIAN", what);
  if (!rf_scratch && sd->rfilter != FFX_RFILTER_BOX) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: the scene's reconstruction filter is not the box (use ffx_%s_filtered)", what, what);
  if (rf_scratch && (!use_packet() || !use_wide(info))) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s_filtered: only the default (wide packet) kernels carry the filter", what);
  return FFX_OK;
}

// what a render call derives from its arguments before it picks a route; c.mats is the caller's material table (shape_albedo).  matm: 0 Lambert,
// 1 material rows, 2 material rows with textured base colours (their own instantiation — the default kernels pay nothing)
struct RenderSetup { ShadeK c; BlobView b; long n_pix; int spp, matm; uint32_t seed_key; int max_depth, rr_depth; };
// the bvh info, the filter, the scene description, the rows' alignment, the 2^32-samples limit and the path depths of `flags`, refused in this order
// with messages that begin with `what`
static int render_setup(const char *what, const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed,
                        int flags, const void *rf_scratch, RenderSetup &r) {
  if (!check_info(info, what)) return FFX_ERR_ARG;
  if (const int rc = check_filter(what, sd, info, rf_scratch)) return rc;
  if (!shade_prepare(sd, r.c)) FFX_FAIL(rf_scratch ? FFX_ERR_UNSUPPORTED : FFX_ERR_ARG, "%s: bad scene description%s", what, rf_scratch ? " (gaussian filter: stddev <= 0.5)" : "");
  r.c.mats = shape_albedo;
  const bool mat = r.c.mat_stride == FFX_MAT_STRIDE;
  if (mat && !r.c.mat_inline && ((uintptr_t)shape_albedo & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "%s: material rows must be 16-byte aligned", what);
  r.n_pix = (long)r.c.cam.W * r.c.cam.H;
  if (r.n_pix * spp >= (1L << 32)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: more than 2^32 samples", what);
  r.b = blob_view(bvh, info);
  r.spp = spp;
  r.matm = !mat ? 0 : (r.c.n_base_tex > 0 ? 2 : 1);
  r.seed_key = seed_key_of(seed);
  if (!path_depths(flags, r.max_depth, r.rr_depth)) FFX_FAIL(FFX_ERR_ARG, "%s: max_depth must be 2 .. %d", what, FFX_RENDER_MAX_DEPTH_LIMIT);
  return FFX_OK;
}
static PathArgs path_args(const RenderSetup &r) {
  return {r.b.nodes, r.b.recs, r.b.nrec, r.spp, r.max_depth, r.rr_depth, r.seed_key, hash32(r.seed_key ^ 0x5bd1e995U)};
}

// what the packet kernels read besides the setup: the pre-pass's apex records (launch_apex), the wide tree and the grid — the film's 2x2-pixel tiles
// enumerated in square blocks of 2^tb x 2^tb tiles (ptx carries tb in its top byte; pn counts the tiles of whole blocks, those outside the image are
// skipped) at ppw pixels per wave (k_render_fwd_pk; the adjoint's 4 = a tile per wave)
struct Packets { const TriApex *arecs; uint32_t astride; WideScene ws; int ptx, pn, pgrid, ppw; };
static void packet_grid(Packets &p, const CamK &cam, int tb, int ppw) {
  const int ptx = ffx_cdiv(cam.W, 2), pty = ffx_cdiv(cam.H, 2);
  p.pn = (ffx_cdiv(ptx, 1 << tb) * ffx_cdiv(pty, 1 << tb)) << (2 * tb);
  p.ptx = ptx | tb << 24;
  p.pgrid = ((p.pn * (4 / ppw) + 7) / 8) * 8; // multiple of 8 so the XCD remap is a bijection onto [0, grid)
  p.ppw = ppw;
}
// k_render_fwd_blk's pixel blocks: sample slots per pixel = the next power of two >= spp (at least min_slots), 64 / slots pixels per wave but at most
// 2^cap, the blocks enumerated in whole 8 x 8 patches
struct PixBlocks { int bw_log2, bh_log2, blocks_x, n_blocks; };
static PixBlocks pixel_blocks(const CamK &cam, int spp, int min_slots, int cap) {
  int slots = min_slots, ppw_log2 = 0;
  while (slots < spp) slots <<= 1;
  while ((slots << (ppw_log2 + 1)) <= 64) ++ppw_log2;
  if (ppw_log2 > cap) ppw_log2 = cap;
  const int bw_log2 = (ppw_log2 + 1) / 2, bh_log2 = ppw_log2 / 2, blocks_x = ffx_cdiv(cam.W, 1 << bw_log2);
  return {bw_log2, bh_log2, blocks_x, 64 * ffx_cdiv(blocks_x, 8) * ffx_cdiv(ffx_cdiv(cam.H, 1 << bh_log2), 8)};
}

static int check_launch(const char *what) { FFX_CHECK_LAUNCH(what); return FFX_OK; }
// the filtered calls' scratch: [pixel][25][4] partial sums, then G = gimg / weight as float4 per pixel (ffx_render_filter_bytes)
static float4 *rf_G_area(void *rf_scratch, long n_pix) { return (float4 *)((float *)rf_scratch + (size_t)n_pix * 100); }
// G = gimg / weight: the weight every pixel receives (the jitter alone decides it) into the partial sums, then the gather into G; NULL if a launch fails
static float4 *rf_G(const RenderSetup &r, const float *gimg, void *rf_scratch, hipStream_t s, const char *what_weights, const char *what_gather) {
  hipLaunchKernelGGL(k_rf_weights, dim3((unsigned)r.n_pix), dim3(64), 0, s, r.c.rf, (int)r.n_pix, r.spp, r.seed_key, (float *)rf_scratch);
  if (check_launch(what_weights) != FFX_OK) return nullptr;
  hipLaunchKernelGGL(k_rf_gather, dim3(ffx_cdiv(r.c.cam.W, 64), ffx_cdiv(r.c.cam.H, FFX_RFG_WAVES)), dim3(64 * FFX_RFG_WAVES), 0, s, (const float4 *)rf_scratch,
                     r.c.cam.W, r.c.cam.H, 0, (void *)nullptr, gimg, rf_G_area(rf_scratch, r.n_pix));
  return check_launch(what_gather) == FFX_OK ? rf_G_area(rf_scratch, r.n_pix) : nullptr;
}
// the image from the partial sums (and, if wsum is given, the weight every pixel received: ffx_render_fwd_cache_filtered)
static int rf_develop(const RenderSetup &r, int fp16, void *img, void *rf_scratch, hipStream_t s, const char *what, float *wsum = nullptr) {
  hipLaunchKernelGGL(k_rf_gather, dim3(ffx_cdiv(r.c.cam.W, 64), ffx_cdiv(r.c.cam.H, FFX_RFG_WAVES)), dim3(64 * FFX_RFG_WAVES), 0, s, (const float4 *)rf_scratch,
                     r.c.cam.W, r.c.cam.H, fp16 & 1, img, (const float *)nullptr, (float4 *)nullptr, wsum);
  FFX_CHECK_LAUNCH(what);
  return FFX_OK;
}

// (wide, matm) as template arguments: f(std::bool_constant<WIDE>, std::integral_constant<int, MATM>).  The launchers instantiate only the kernels that
// exist (`if constexpr`): the host refuses the other combinations first — a filtered film off the wide walk, textured base colours with an adjoint
// cache or the fused adjoint.  (The order of the references is the order of the kernels in the code object.)
template <class F> static void dispatch_wm(bool wide, int matm, F &&f) {
  auto by_matm = [&](auto w) {
    if (matm == 2) f(w, std::integral_constant<int, 2>());
    else if (matm == 1) f(w, std::integral_constant<int, 1>());
    else f(w, std::integral_constant<int, 0>());
  };
  if (wide) by_matm(std::true_type());
  else by_matm(std::false_type());
}
// (filtered film, material block) as template arguments, for the per-lane appearance kernels: f(std::bool_constant<RF>, std::bool_constant<MAT>)
template <class F> static void dispatch_rf_mat(bool rf, bool mat, F &&f) {
  auto by_mat = [&](auto r) {
    if (mat) f(r, std::true_type());
    else f(r, std::false_type());
  };
  if (rf) by_mat(std::true_type());
  else by_mat(std::false_type());
}
// ... with the lights' pass's third (filtered film, directional records, constant emitter), for k_lights_fwd: f(std::bool_constant<RF>, <DIR>, <AMB>)
template <class F> static void dispatch_rf_dir_amb(bool rf, bool dir, bool amb, F &&f) {
  dispatch_rf_mat(rf, dir, [&](auto r, auto d) {
    if (amb) f(r, d, std::true_type());
    else f(r, d, std::false_type());
  });
}
// What k_render_fwd_pk<..., PLAIN> takes as constants, proved here from what the call carries (anything less: the generic instance).  The rows
// travel inline and shade_prepare derived a pre-row for each (mat_pre_on), every row is a principled row (model != 0) with no optional lobe (its
// flag word is 0), the blob's last update flagged no shape smooth (ffx_blob_flat: a blob this process has not updated is not known to be flat), a spot
// is rigid, a projector texture has one channel, the film is f32 and takes one pass.  Box film: the route's own condition; with or without an adjoint cache
// (whose buffer keeps its 64-bit addressing: it is not among the areas proved below 2^32 bytes).
// The camera is in band (ffx_band.h: w_uniform, qz one-signed over the film, |np|^2 and |dl.z| within [2^-40, 2^40], bounded in double from the
// film's corners with the float roundings covered) — cam_ray<BAND> then takes its root and its two reciprocals as seed + fma chain, without the
// IEEE expansions' scaling, fix-up and class steps, which do nothing there.  The blob (tile bins with their envelopes, gn, apex records) and the
// projector's texture are below 2^32 bytes, the texture's sides below 2^24; the rows are kernel arguments: the instance addresses all of them by
// 32-bit offsets from their scalar bases (at32).
int ffx_blob_flat(const void *bvh); // (ffx_scene.hip; not part of the C ABI)
static bool plain_scene(const RenderSetup &r, const ffx_scene_desc *sd, const void *bvh, const ffx_bvh_info *info, int fp16) {
  if (!k8_plain_enabled() || r.matm != 1 || !r.c.mat_inline || !r.c.mat_pre_on || (fp16 & FFX_RENDER_FP16) || r.spp > 64) return false;
  if ((r.c.spot_on && !r.c.s_rigid) || (r.c.proj_on && r.c.tc != 1)) return false;
  if (FFX_K8_BAND && !ffx_cam_in_band(r.c.cam.s2c, r.c.cam.w_uniform, r.c.cam.iw_u)) return false;
  if (FFX_K8_OFF32 && (info->total_bytes >= (1ull << 32) || (r.c.proj_on && (r.c.tw >= (1 << 24) || r.c.th >= (1 << 24) || 4ull * (uint64_t)r.c.tw * (uint64_t)r.c.th >= (1ull << 32))))) return false;
  for (int k = 0; k < sd->n_shapes; ++k) { // (mat_pre_on: at most 8 rows, all inline)
    uint32_t flags;
    memcpy(&flags, &r.c.mat_pre[k * FFX_PRE_FLOATS + FFX_PRE_FLAGS], 4);
    if (flags != 0u || r.c.mat_h[k * FFX_MAT_STRIDE + FFX_MAT_MODEL] == 0.f) return false;
  }
  return ffx_blob_flat(bvh) == 1;
}
// ---- the table-fed plain instances' pixel-rectangle tables (ffx_rect.h; read by bins_primary<..., RECT>).  A table depends on the film's size and the
// camera grid's tile side alone — not on the pose, the seed, the texture or the materials —, so the library keeps it on the device per (device, W, H,
// its_x, its_y): built and uploaded at a key's first launch, found again by every later one (a run renders one film; another film or another
// FFX_BIN_TILE is another key).  A table, once made, is NEVER freed or moved: a launch that is queued, in flight or recorded for replay keeps a valid
// pointer whatever other threads or later calls do, and the mutex needs to cover the lookup only.  FFX_RECT_KEYS keys (at most FFX_RECT_KEYS x 128 KB,
// which stay with the process's device context: the library's unload makes no HIP call, which at process exit would come after the runtime's own
// teardown); a process that has used them all renders further films through the generic instance
// and says so once on stderr (the issue asked for a handful of keys freed at unload: DESIGN 5.1, round 11, gives the reasons for this form).  The upload is a copy on the render's own stream
// followed by a wait for that stream: ordered before the launch that follows, complete before any later launch on any stream, and the host vector
// outlives it.  Constraint: a key's FIRST launch allocates and waits, so it must not be made while its stream is being captured (render the film once
// before capturing; later launches of the key make no HIP call here).
// -> false: no table for this launch (a film beyond FFX_RECT_MAX_SIDE, every key in use, no device memory) — the launch takes the generic instance.
static_assert(FFX_RECT_BIN_PAD == FFX_BIN_PAD, "ffx_rect.h restates the bins' pad");
#define FFX_RECT_KEYS 32
struct RectTab { int dev, W, H; float its_x, its_y, hx, hy; void *d; };
static RectTab g_rect_tab[FFX_RECT_KEYS];
static std::mutex g_rect_mu;
static bool rect_tables(const ShadeK &c, RectK &rk, hipStream_t s) {
  const BinsK &bk = c.bins;
  memset(&rk, 0, sizeof rk);
  for (int a = 0; a < FFX_N_APEX; ++a) { rk.gxf[a] = (float)bk.g[a].nx; rk.gyf[a] = (float)bk.g[a].ny; } // (bins_shadow<..., GF>: the conversion it made per call)
  if (!bk.g[0].on) return true; // (no camera grid: bins_primary leaves before it looks at a table)
  const int W = c.cam.W, H = c.cam.H;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(g_rect_mu);
  RectTab *e = nullptr, *free_slot = nullptr;
  for (RectTab &t : g_rect_tab) {
    if (t.d && t.dev == dev && t.W == W && t.H == H && t.its_x == bk.cam_inv_ts_x && t.its_y == bk.cam_inv_ts_y) { e = &t; break; }
    if (!t.d && !free_slot) free_slot = &t;
  }
  if (!e) {
    if (!free_slot) { // every key in use: said once, since from here on this process renders new films through the generic instance
      static bool told = false;
      if (!told) fprintf(stderr, "libffx_hip: all %d pixel-rectangle tables are in use; further film sizes render through the generic K8 instance\n", FFX_RECT_KEYS);
      told = true;
      return false;
    }
    std::vector<FfxRectEntry> tab;
    float hx, hy;
    if (!ffx_rect_fill(W, H, bk.cam_inv_ts_x, bk.cam_inv_ts_y, tab, hx, hy)) return false;
    void *d = nullptr;
    if (hipMalloc(&d, tab.size() * sizeof(FfxRectEntry)) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(FfxRectEntry), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(d); // (never handed out)
      return false;
    }
    *free_slot = {dev, W, H, bk.cam_inv_ts_x, bk.cam_inv_ts_y, hx, hy, d};
    e = free_slot;
  }
  rk.tab = e->d;
  rk.hx = e->hx;
  rk.hy = e->hy;
  rk.row0 = (uint32_t)W;
  return true;
}
// launches of k_render_fwd_pk by instance: [0] plain-scene, [1] generic (a data symbol, not an entry point: fireflies_amd/ops.py
// k8_launch_counters reads it in place — how mi.Scene.render_paths and the tests see which instance ran)
extern "C" { unsigned long long ffx_k8_instance_launches[2] = {0ull, 0ull}; }
// a k_render_fwd_pk launch's own arguments (the kernel's parameters: fp16, img, cache, cache_foot_off / cache_arena_off / cache_foot_b_off, ...);
// plain: the scene passed plain_scene (the box film's route only: its forward, its forward + adjoint and its cache-writing forward)
// kernarg_rect: k_render_fwd_pk's last argument, read in place.  The kernarg segment lays the arguments out in order, each at its own alignment, so
// the last one's offset follows from the kernel's parameter types — taken from the kernel's own type here, nothing restates the list (the code
// object's metadata says the same: .offset of the last .args entry, 1856).
template <class F> struct KernargLast;
template <class... A> struct KernargLast<void (*)(A...)> {
  static constexpr size_t offset() {
    size_t off = 0, last = 0;
    ((off = (off + alignof(A) - 1) / alignof(A) * alignof(A), last = off, off += sizeof(A)), ...);
    return last;
  }
};
__device__ __forceinline__ const RectK &kernarg_rect() {
  const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const RectK *)(p + KernargLast<decltype(&k_render_fwd_pk<1, true, 1>)>::offset());
}
struct FwdPkArgs { int fp16; void *img; char *cache; uint32_t off[3], cap_stray; const float *adj_gimg; float *adj_gtex, *adj_dot; bool plain = false; RectK rk = {}; };
// ADJ: k_render_fwd_pk's ADJ (0 / 1), or 2 for the box film's route, which takes the fused adjoint iff a.adj_gtex
template <int ADJ, bool RF = false, bool RFC = false>
static void launch_fwd_pk(bool wide, const RenderSetup &r, const Packets &p, const float *tex, const FwdPkArgs &a, hipStream_t s) {
  dispatch_wm(wide, r.matm, [&](auto w, auto m) {
    auto launch = [&](auto adj) {
      constexpr bool WIDE = decltype(w)::value, A = decltype(adj)::value;
      constexpr int MATM = decltype(m)::value;
      auto go = [&](auto plain, auto with_cache) {
        constexpr bool PLAIN = decltype(plain)::value, CACHE = decltype(with_cache)::value;
        __atomic_fetch_add(&ffx_k8_instance_launches[PLAIN ? 0 : 1], 1ull, __ATOMIC_RELAXED);
        hipLaunchKernelGGL((k_render_fwd_pk<1, WIDE, MATM, A, RF, RFC, PLAIN, CACHE>), dim3(p.pgrid), dim3(64), 0, s, r.c, r.b.nodes, r.b.recs, p.arecs, p.astride, p.ws,
                           r.c.mats, tex, r.spp, r.seed_key, p.ptx, p.pn, xcd_mode(r.n_pix), a.fp16, a.img, a.cache, p.ppw, 1.0f / (float)r.spp, a.off[0],
                           a.off[1], a.off[2], r.b.nrec, r.b.gn, a.cap_stray, a.adj_gimg, a.adj_gtex, a.adj_dot, a.rk);
      };
      if constexpr ((WIDE || !RF) && (MATM < 2 || (!A && !RFC))) {
        if constexpr (ADJ == 2 && MATM == 1) { // (the box film's route: the only one with plain-scene instances — forward, forward + adjoint, cache-writing forward)
          if (a.plain) {
            if constexpr (!A) {
              if (a.cache) { go(std::true_type(), std::true_type()); return; }
            }
            go(std::true_type(), std::false_type());
            return;
          }
        }
        go(std::false_type(), std::false_type());
      }
    };
    if constexpr (ADJ != 2) launch(std::bool_constant<ADJ == 1>());
    else if (a.adj_gtex) launch(std::true_type());
    else launch(std::false_type());
  });
}
template <bool RF = false>
static void launch_fwd_blk(bool wide, const RenderSetup &r, const Packets &p, const PixBlocks &pb, const float *tex, int fp16, void *img, hipStream_t s) {
  dispatch_wm(wide, r.matm, [&](auto w, auto m) {
    if constexpr (decltype(w)::value || !RF)
      hipLaunchKernelGGL((k_render_fwd_blk<decltype(w)::value, decltype(m)::value, RF>), dim3(pb.n_blocks), dim3(64), 0, s, r.c, r.b.nodes, r.b.recs, p.arecs,
                         p.astride, p.ws, r.c.mats, tex, r.spp, r.seed_key, pb.bw_log2, pb.bh_log2, pb.blocks_x, pb.n_blocks, fp16, img, 1.0f / (float)r.spp,
                         r.b.nrec, r.b.gn);
  });
}
template <bool RF>
static void launch_bwd_pk(bool wide, const RenderSetup &r, const Packets &p, const float *gsrc, float *gtex, const DetK &det, hipStream_t s) {
  dispatch_wm(wide, r.matm, [&](auto w, auto m) {
    if constexpr (decltype(w)::value || !RF)
      hipLaunchKernelGGL((k_render_bwd_pk<1, decltype(w)::value, decltype(m)::value, RF>), dim3(p.pgrid), dim3(64), 0, s, r.c, r.b.nodes, r.b.recs, p.arecs,
                         p.astride, p.ws, r.c.mats, r.spp, r.seed_key, p.ptx, p.pn, xcd_mode(r.n_pix), gsrc, gtex, r.b.nrec, r.b.gn, det);
  });
}

extern "C" {

int ffx_trace_primary(const void *bvh, const ffx_bvh_info *info, const ffx_camera *cam, int spp, int jitter, uint32_t seed, float *t_out,
                      int32_t *shape_out, int32_t *prim_out, ffx_stream s) {
  if (!bvh || !info || !cam || !t_out || spp < 1) FFX_FAIL(FFX_ERR_ARG, "trace_primary: bad argument");
  if (!check_info(info, "trace_primary")) return FFX_ERR_ARG;
  CamK k;
  if (!cam_prepare(cam, k)) FFX_FAIL(FFX_ERR_ARG, "trace_primary: bad camera");
  long total = (long)k.W * k.H * spp;
  if (total >= (1L << 32)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "trace_primary: more than 2^32 samples");
  const BlobView b = blob_view(bvh, info);
  if (use_packet()) {
    // pixels per wave: 64 / spp when spp divides 64 (a compact bw x bh block), else one pixel per wave
    int ppw_log2 = 0;
    if (spp < 64 && 64 % spp == 0)
      while ((spp << (ppw_log2 + 1)) <= 64) ++ppw_log2;
    {
      // ... but never more than 8 pixels per wave: a smaller block leaves lanes idle, yet it makes
      // more and thinner packets — fewer exact tests per walk (24 per walk with 8x8-pixel packets) and enough waves to
      // hide the walk's latency (4096 waves of 64 pixels do not fill the GPU).  Measured at 512^2 (tools/k7time.py):
      // 1 / 2 / 4 spp 0.118 / 0.105 / 0.095 ms with full waves, 0.071 / 0.056 / 0.057 ms capped; >= 8 spp unchanged.
      // (tools/lowspp.py, 512^2: 4 / 8 / 16 / 32 / 64 pixels per wave at 1 spp = 0.174 / 0.160 / 0.169 / 0.192 / 0.239 ms; at 4 spp 0.193 / 0.175 / 0.185)
      if (ppw_log2 > 3) ppw_log2 = 3;
    }
    const int bw_log2 = (ppw_log2 + 1) / 2, bh_log2 = ppw_log2 / 2;
    const int blocks_x = ffx_cdiv(k.W, 1 << bw_log2), n_blocks = blocks_x * ffx_cdiv(k.H, 1 << bh_log2);
    const TriApex *arecs;
    uint32_t astride;
    // the pre-pass of a camera-only scene: apex records and (round 4) the camera's tile bins; with FFX_RENDER_APEX_READY in `jitter` the
    // camera's area already holds both — a render of this pose from this camera wrote them — and nothing is launched in front of the kernel
    ffx_scene_desc sdt;
    memset(&sdt, 0, sizeof sdt);
    sdt.cam = *cam;
    if (!launch_apex(bvh, info, cam->to_world, &sdt, &arecs, &astride, (hipStream_t)s, nullptr, 0, jitter & FFX_RENDER_APEX_READY)) return FFX_ERR_ARG;
    BinsK bk;
    bins_k(bvh, info, &sdt, bk);
    const int jit = jitter & 1;
    const WideScene ws = wide_scene(bvh, info);
    if (use_wide(info))
      hipLaunchKernelGGL(k_trace_primary_pk<true>, dim3(n_blocks), dim3(64), 0, (hipStream_t)s, k, b.nodes, b.recs, arecs, ws, spp, jit,
                         seed_key_of(seed), bw_log2, bh_log2, blocks_x, n_blocks, t_out, shape_out, prim_out, bk);
    else
      hipLaunchKernelGGL(k_trace_primary_pk<false>, dim3(n_blocks), dim3(64), 0, (hipStream_t)s, k, b.nodes, b.recs, arecs, ws, spp, jit,
                         seed_key_of(seed), bw_log2, bh_log2, blocks_x, n_blocks, t_out, shape_out, prim_out, bk);
    FFX_CHECK_LAUNCH("trace_primary");
    return FFX_OK;
  }
  hipLaunchKernelGGL(k_trace_primary, dim3(ffx_cdiv(total, TR_BLOCK)), dim3(TR_BLOCK), stack_bytes(info), (hipStream_t)s, k, b.nodes, b.recs, spp, jitter & 1,
                     seed_key_of(seed), total, t_out, shape_out, prim_out);
  FFX_CHECK_LAUNCH("trace_primary");
  return FFX_OK;
}

int ffx_trace_rays(const void *bvh, const ffx_bvh_info *info, const float *origins, const float *dirs, int n, float tmax, float *t_out,
                   int32_t *shape_out, int32_t *prim_out, ffx_stream s) {
  if (n == 0) return FFX_OK;
  if (!bvh || !info || !origins || !dirs || !t_out || n < 0) FFX_FAIL(FFX_ERR_ARG, "trace_rays: bad argument");
  if (!check_info(info, "trace_rays")) return FFX_ERR_ARG;
  if (n == 0) return FFX_OK;
  const BlobView b = blob_view(bvh, info);
  hipLaunchKernelGGL(k_trace_rays, dim3(ffx_cdiv(n, TR_BLOCK)), dim3(TR_BLOCK), stack_bytes(info), (hipStream_t)s, b.nodes, b.recs, origins, dirs, n, tmax,
                     t_out, shape_out, prim_out);
  FFX_CHECK_LAUNCH("trace_rays");
  return FFX_OK;
}

int ffx_trace_rays_bwd(const void *bvh, const ffx_bvh_info *info, const float *origins, const float *dirs, int n, const float *t, const int32_t *prim,
                       const float *gt, float *gorig, float *gdir, ffx_stream s) {
  if (n < 0) FFX_FAIL(FFX_ERR_ARG, "trace_rays_bwd: n = %d is negative", n);
  if (!bvh) FFX_FAIL(FFX_ERR_ARG, "trace_rays_bwd: bvh is NULL");
  if (!info) FFX_FAIL(FFX_ERR_ARG, "trace_rays_bwd: info is NULL");
  if (!check_info(info, "trace_rays_bwd")) return FFX_ERR_ARG;
  if (n == 0) return FFX_OK;
  const struct { const void *p; const char *name; } ptrs[] = {{origins, "origins"}, {dirs, "dirs"}, {t, "t"}, {prim, "prim"}, {gt, "gt"}, {gorig, "gorig"}, {gdir, "gdir"}};
  for (const auto &a : ptrs)
    if (!a.p) FFX_FAIL(FFX_ERR_ARG, "trace_rays_bwd: %s is NULL", a.name);
  const BlobView b = blob_view(bvh, info);
  hipLaunchKernelGGL(k_trace_rays_bwd, dim3(ffx_cdiv(n, TR_BLOCK)), dim3(TR_BLOCK), stack_bytes(info), (hipStream_t)s, b.nodes, b.recs, origins, dirs, n, t, prim,
                     gt, gorig, gdir);
  FFX_CHECK_LAUNCH("trace_rays_bwd");
  return FFX_OK;
}

static int render_fwd_impl(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                           uint32_t seed, int call_flags, void *img, void *cache, ffx_stream s, const float *adj_gimg = nullptr, float *adj_gtex = nullptr,
                           float *adj_dot = nullptr, void *rf_scratch = nullptr, void *rf_cache = nullptr) {
  const int img_fp16 = call_flags & (FFX_RENDER_FP16 | FFX_RENDER_SPARSE_ADJOINT); // what the kernels see; the other bits steer the pre-pass
  if (!bvh || !info || !sd || (!shape_albedo && sd->n_mat_h <= 0) || !img || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_fwd: bad argument");
  if (sd->proj.enabled && !tex) FFX_FAIL(FFX_ERR_ARG, "render_fwd: projector enabled but tex is NULL");
  RenderSetup r;
  if (const int rc = render_setup("render_fwd", bvh, info, sd, shape_albedo, spp, seed, call_flags, rf_scratch, r)) return rc;
  const hipStream_t st = (hipStream_t)s;
  if (r.max_depth > 2) { // the path integrator: one wave per pixel; no apex records, no tile bins
    if (cache || adj_gtex) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd: max_depth > 2 has neither an adjoint cache nor a fused adjoint (use ffx_render_bwd)");
    if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd: more than 2^31 pixels");
    const PathArgs pa = path_args(r);
    if (rf_scratch) {
      hipLaunchKernelGGL(k_path_fwd<true>, dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, tex, 0, (void *)nullptr, (float *)rf_scratch);
      FFX_CHECK_LAUNCH("render_fwd_filtered (path)");
      return rf_develop(r, img_fp16, img, rf_scratch, st, "render_fwd_filtered (path)/gather");
    }
    hipLaunchKernelGGL(k_path_fwd<false>, dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, tex, img_fp16 & 1, img, (float *)nullptr);
    FFX_CHECK_LAUNCH("render_fwd (path)");
    return FFX_OK;
  }
  if (cache && sd->n_base_tex > 0) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_cache: textured base colours (the footprint folds one base colour per shape): use ffx_render_bwd");
  if (cache && sd->proj.enabled && (sd->proj.tex_w > 4094 || sd->proj.tex_h > 4094 || sd->n_shapes > 255))
    FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_cache: texture larger than 4094^2 or more than 255 shapes");
  if (adj_gtex && sd->n_base_tex > 0) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_adjoint: textured base colours (the footprint folds one base colour per shape): use ffx_render_bwd");
  const bool packet = use_packet() || cache || adj_gtex; // the per-sample cache / the fused adjoint are the packet kernels'
  if (packet && !r.b.gn) FFX_FAIL(FFX_ERR_ARG, "render_fwd: blob without per-slot normals (built by another library version?)");
  if (packet) {
    const bool folds = cache != nullptr || adj_gtex != nullptr || rf_cache != nullptr;
    Packets p;
    packet_grid(p, r.c.cam, tile_block_log2(r.n_pix, folds), pixels_per_wave(folds, r.n_pix));
    // (capacity of the cache's arena: single-sample records of the box film's footprint cache / 64-sample blocks of the filtered film's record cache)
    uint32_t cap_stray = cache ? (uint32_t)cache_stray_capacity(r.c.cam.W, r.c.cam.H, spp) : (rf_cache ? (uint32_t)rfc_cap_blocks((size_t)r.n_pix, (size_t)spp, rfc_all(sd)) : 0u);
    if (rf_cache)
      if (const char *ce = getenv("FFX_RFC_CAP")) { // (test knob, include/ffx.h: fewer blocks than the cache has room for — the overflow path)
        const long cv = atol(ce);
        if (cv >= 0 && (unsigned long)cv < cap_stray) cap_stray = (uint32_t)cv;
      }
    if (!launch_apex(bvh, info, sd->cam.to_world, sd, &p.arecs, &p.astride, st, cache ? cache : rf_cache, cap_stray, call_flags)) return FFX_ERR_ARG;
    p.ws = wide_scene(bvh, info);
    bins_k(bvh, info, sd, r.c.bins);
    // offsets of the cache areas in units of 128 bytes (both are multiples of 128; a 1024^2 x 256-spp cache is 160 MB)
    const uint32_t foot_off = (uint32_t)(cache_off_foot((size_t)r.n_pix) >> 7), arena_off = (uint32_t)(cache_off_arena((size_t)r.n_pix) >> 7);
    const uint32_t foot_b_off = (uint32_t)(cache_off_foot_b((size_t)r.n_pix, cache_stray_capacity(r.c.cam.W, r.c.cam.H, spp)) >> 7);
    if (rf_scratch && adj_gtex) { // ... with the adjoint of a loss that is linear in the image folded in (ffx_render_fwd_adjoint_filtered)
      if (sd->proj.tex_channels != 1 || r.matm == 2) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_adjoint_filtered: 1-channel projector textures without textured base colours (use ffx_render_fwd_filtered + ffx_render_bwd_filtered)");
      // G = gimg / weight behind the partial sums; then the render, whose footprints take every sample's own gradient from G; then the image
      const float4 *G = rf_G(r, adj_gimg, rf_scratch, st, "render_fwd_adjoint_filtered/weights", "render_fwd_adjoint_filtered/gather G");
      if (!G) return FFX_ERR_LAUNCH;
      launch_fwd_pk<1, true>(true, r, p, tex, {img_fp16, img, (char *)rf_scratch, {foot_off, arena_off, foot_b_off}, cap_stray, (const float *)G, adj_gtex, nullptr}, st);
      FFX_CHECK_LAUNCH("render_fwd_adjoint_filtered");
      return rf_develop(r, img_fp16, img, rf_scratch, st, "render_fwd_adjoint_filtered/gather");
    }
    if (rf_scratch && rf_cache) { // ... that also stores its adjoint's per-sample records (ffx_render_fwd_cache_filtered; rfc_off_* above)
      if (r.matm == 2) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: textured base colours (the records carry one base colour per shape): use ffx_render_bwd_filtered");
      if (sd->proj.enabled && (sd->proj.tex_w > 4094 || sd->proj.tex_h > 4094 || sd->n_shapes > 255)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: texture larger than 4094^2 or more than 255 shapes");
      if (spp > 1024) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: more than 1024 samples per pixel (16 passes)");
      const size_t n_pix = (size_t)r.n_pix;
      const uint32_t recs_off = (uint32_t)(rfc_off_recs(n_pix) >> 7), facb_off = (uint32_t)(rfc_off_facb(n_pix, (size_t)spp, rfc_all(sd)) >> 7);
      launch_fwd_pk<0, true, true>(true, r, p, tex, {img_fp16, img, (char *)rf_scratch, {recs_off, arena_off, facb_off}, cap_stray, nullptr, (float *)rf_cache, nullptr}, st);
      FFX_CHECK_LAUNCH("render_fwd_cache_filtered");
      return rf_develop(r, img_fp16, img, rf_scratch, st, "render_fwd_cache_filtered/gather", (float *)((char *)rf_cache + rfc_off_wsum(n_pix)));
    }
    if (rf_scratch && spp <= 32 && lowspp_blocks()) { // ... below 33 samples per pixel: several pixels per wave, the same scratch contents (k_render_fwd_blk<..., RF>)
      // (at least 8 sample slots per pixel: rf_fold_blk reads them in groups of four, two pixels per round -> 8 / 4 / 2 pixels per wave at <= 8 / 16 / 32 spp)
      launch_fwd_blk<true>(true, r, p, pixel_blocks(r.c.cam, spp, 8, 3), tex, img_fp16 & 1, rf_scratch, st);
      FFX_CHECK_LAUNCH("render_fwd_filtered (pixel blocks)");
      return rf_develop(r, img_fp16, img, rf_scratch, st, "render_fwd_filtered/gather");
    }
    if (rf_scratch) { // the filtered render: the kernel leaves every pixel's 25 x 4 outgoing sums in the scratch area, the gather forms the image
      launch_fwd_pk<0, true>(true, r, p, tex, {img_fp16 & 1, img, (char *)rf_scratch, {foot_off, arena_off, foot_b_off}, cap_stray, adj_gimg, adj_gtex, adj_dot}, st);
      FFX_CHECK_LAUNCH("render_fwd_filtered");
      return rf_develop(r, img_fp16, img, rf_scratch, st, "render_fwd_filtered/gather");
    }
    if (!cache && !adj_gtex && spp <= 32 && lowspp_blocks()) {
      // fewer than 64 samples per pixel: several pixels per wave (k_render_fwd_blk).  Sample slots per pixel = the next power of two >= spp; the
      // block never exceeds 8 pixels (K7's reason, ffx_trace_primary: thinner packets, fewer exact tests per walk, more waves)
      launch_fwd_blk(use_wide(info), r, p, pixel_blocks(r.c.cam, spp, 1, spp == 1 ? 4 : 3), tex, img_fp16, img, st);
      FFX_CHECK_LAUNCH("render_fwd (pixel blocks)");
      return FFX_OK;
    }
    // (a plain scene AND the film's rectangle tables at hand, which the plain instances read: rect_tables)
    RectK rk = {};
    // (the cache-writing plain forward — a cache and no fused adjoint — reads no table: launch_fwd_pk's choice of instance)
    const bool reads_tables = FFX_K8_RECTTAB && (adj_gtex || !cache);
    const bool plain = plain_scene(r, sd, bvh, info, img_fp16) && (!reads_tables || rect_tables(r.c, rk, st));
    launch_fwd_pk<2>(use_wide(info), r, p, tex, {img_fp16, img, (char *)cache, {foot_off, arena_off, foot_b_off}, cap_stray, adj_gimg, adj_gtex, adj_dot, plain, rk}, st);
    FFX_CHECK_LAUNCH("render_fwd");
    return FFX_OK;
  }
  int tiles_x = ffx_cdiv(r.c.cam.W, 8), tiles_y = ffx_cdiv(r.c.cam.H, 8);
  int n_tiles = tiles_x * tiles_y;
  int grid = ((n_tiles + 7) / 8) * 8;
  hipLaunchKernelGGL(k_render_fwd, dim3(grid), dim3(TR_BLOCK), stack_bytes(info), st, r.c, r.b.nodes, r.b.recs, r.b.nrec, shape_albedo, tex, spp,
                     r.seed_key, tiles_x, n_tiles, xcd_mode(), img_fp16, img);
  FFX_CHECK_LAUNCH("render_fwd");
  return FFX_OK;
}

// the appearance adjoint's bits belong to ffx_render_bwd[_filtered]: every other render entry point refuses them
#define FFX_NO_APPEARANCE(flags_, what_)                                                                                                                  \
  do {                                                                                                                                                    \
    if ((flags_) & FFX_RENDER_GRAD_APPEARANCE) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_GRAD_APPEARANCE is served by ffx_render_bwd[_filtered] only", what_); \
    if ((flags_) & FFX_RENDER_GRAD_MATERIAL) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_GRAD_MATERIAL is served by ffx_render_bwd[_filtered] only", what_);     \
    if ((flags_) & FFX_RENDER_GRAD_PRB) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_GRAD_PRB is served by ffx_render_bwd[_filtered] only", what_);               \
  } while (0)
// the tangent image's bit belongs to ffx_render_fwd[_filtered]: every other render entry point refuses it
#define FFX_NO_TANGENT(flags_, what_) \
  do { if ((flags_) & FFX_RENDER_TANGENT) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_TANGENT is served by ffx_render_fwd[_filtered] only", what_); } while (0)
// FFX_RENDER_TANGENT (include/ffx.h): the primal by the launches of a call without the bit, then one launch of k_render_jvp (max_depth 2)
// or k_path_jvp into the tangent image behind it (the gaussian film: into the scratch, which the primal's gather has read by then, and a second gather)
static int render_jvp(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp, uint32_t seed,
                      int img_fp16, void *img, ffx_stream s, void *rf_scratch) {
  const char *what = rf_scratch ? "render_fwd_filtered" : "render_fwd";
  if (img_fp16 & FFX_RENDER_FP16) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_TANGENT has no fp16 film", what);
  if (!shape_albedo) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_TANGENT needs the device material table (shape_albedo is NULL)", what);
  if (!bvh || !info || !sd || !img || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_fwd: bad argument");
  if (!tex) FFX_FAIL(FFX_ERR_ARG, "render_fwd: FFX_RENDER_TANGENT but tex (the tangent blocks) is NULL");
  RenderSetup r;
  if (const int rc = render_setup("render_fwd", bvh, info, sd, shape_albedo, spp, seed, img_fp16, rf_scratch, r)) return rc;
  if (sd->n_shapes < 1) FFX_FAIL(FFX_ERR_ARG, "render_fwd: n_shapes < 1");
  const long n_tex = sd->proj.enabled ? (long)sd->proj.tex_w * sd->proj.tex_h * sd->proj.tex_channels : 0;
  if (n_tex < 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd: bad projector texture size");
  if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd: more than 2^31 pixels");
  if (const int rc = render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & (FFX_RENDER_APEX_READY | FFX_RENDER_PATH_MASK), img, nullptr, s, nullptr,
                                     nullptr, nullptr, rf_scratch))
    return rc;
  JvpArgs j;
  memset(&j, 0, sizeof j);
  if (sd->proj.enabled) { j.tex = tex; j.dtex = tex + n_tex; }
  j.drow = tex + 2 * n_tex; j.dspot = j.drow + (size_t)3 * sd->n_shapes;
  const float *bt = j.dspot + 3;
  for (int k = 0; k < r.c.n_base_tex; ++k) {
    j.dbt[k] = bt;
    bt += (size_t)3 * r.c.btw[k] * r.c.bth[k];
  }
  // (a table of stride 3 has no material columns: the block is not there)
  j.dmat = r.c.mat_stride == FFX_MAT_STRIDE ? tex + 2 * n_tex + FFX_RENDER_APPEARANCE_FLOATS(sd) : nullptr;
  j.dimg = (float *)img + (size_t)r.n_pix * 3;
  j.part = (float *)rf_scratch;
  const hipStream_t st = (hipStream_t)s;
  const PathArgs pa = path_args(r);
  const bool path = r.max_depth > 2;
  dispatch_rf_mat(rf_scratch != nullptr, j.dmat != nullptr, [&](auto rf, auto m) {
    constexpr bool RF = decltype(rf)::value, MAT = decltype(m)::value;
    if (path) hipLaunchKernelGGL((k_path_jvp<RF, MAT>), dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, j);
    else hipLaunchKernelGGL((k_render_jvp<RF, MAT>), dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, j);
  });
  FFX_CHECK_LAUNCH(path ? (rf_scratch ? "render_fwd_filtered (path, tangent)" : "render_fwd (path, tangent)") : (rf_scratch ? "render_fwd_filtered (tangent)" : "render_fwd (tangent)"));
  if (rf_scratch) return rf_develop(r, 0, j.dimg, rf_scratch, st, "render_fwd_filtered (tangent)/gather");
  return FFX_OK;
}
// the AOV block's bit belongs to ffx_render_fwd[_filtered]: every other render entry point refuses it
#define FFX_NO_AOV(flags_, what_) \
  do { if ((flags_) & FFX_RENDER_AOV) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_AOV is served by ffx_render_fwd[_filtered] only", what_); } while (0)
// FFX_RENDER_AOV (include/ffx.h): the image by the launches of a call without the bit, then k_render_aov into the block behind it — one
// launch under the box film; under the gaussian film one launch into the scratch (which the image's gather has read by then) and one gather per group
static int render_aov(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp, uint32_t seed,
                      int img_fp16, void *img, ffx_stream s, void *rf_scratch) {
  const char *what = rf_scratch ? "render_fwd_filtered" : "render_fwd";
  if (img_fp16 & FFX_RENDER_FP16) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_AOV has no fp16 film", what);
  if (img_fp16 & FFX_RENDER_TANGENT) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_AOV is not served together with FFX_RENDER_TANGENT", what);
  if (sd && !shape_albedo && sd->n_mat_h <= 0) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_AOV needs a material table (shape_albedo is NULL and sd->mat_h is empty)", what);
  if (!bvh || !info || !sd || !img || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_fwd: bad argument");
  RenderSetup r;
  if (const int rc = render_setup("render_fwd", bvh, info, sd, shape_albedo, spp, seed, img_fp16, rf_scratch, r)) return rc;
  if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd: more than 2^31 pixels");
  if (!r.b.gn) FFX_FAIL(FFX_ERR_ARG, "render_fwd: blob without per-slot normals (built by another library version?)");
  if (const int rc = render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & (FFX_RENDER_APEX_READY | FFX_RENDER_PATH_MASK), img, nullptr, s, nullptr,
                                     nullptr, nullptr, rf_scratch))
    return rc;
  const hipStream_t st = (hipStream_t)s;
  // the camera's apex records and bins: a packet render at direct light has just written them; the path kernels and the per-lane kernels write none,
  // and the caller's FFX_RENDER_APEX_READY then says whether the blob holds them (as for ffx_trace_primary)
  const bool fresh = use_packet() && r.max_depth == 2;
  const TriApex *arecs;
  uint32_t astride;
  if (!launch_apex(bvh, info, sd->cam.to_world, sd, &arecs, &astride, st, nullptr, 0, fresh ? FFX_RENDER_APEX_READY : (img_fp16 & FFX_RENDER_APEX_READY))) return FFX_ERR_ARG;
  bins_k(bvh, info, sd, r.c.bins);
  // below 33 samples per pixel a compact block of pixels per wave (at least 8 sample slots per pixel under the gaussian film: rf_fold_blk), else one
  // pixel — and one pixel whatever the count under FFX_RENDER_BLOCKS=0, as the render beside it
  int bw_log2 = 0, bh_log2 = 0;
  if (spp <= 32 && lowspp_blocks()) {
    const PixBlocks pb = pixel_blocks(r.c.cam, spp, rf_scratch ? 8 : 1, 3);
    bw_log2 = pb.bw_log2; bh_log2 = pb.bh_log2;
  }
  AovK a;
  a.c = r.c;
  a.nodes = r.b.nodes; a.recs = r.b.recs; a.arecs = arecs; a.ws = wide_scene(bvh, info);
  a.spp = spp; a.seed_key = r.seed_key; a.bw_log2 = bw_log2; a.bh_log2 = bh_log2;
  a.blocks_x = ffx_cdiv(r.c.cam.W, 1 << bw_log2);
  a.n_blocks = a.blocks_x * ffx_cdiv(r.c.cam.H, 1 << bh_log2);
  a.nrec = r.b.nrec; a.gn = r.b.gn;
  a.out = (float *)img + (size_t)r.n_pix * 3;
  a.group = 0;
  if (!rf_scratch) {
    if (use_wide(info)) hipLaunchKernelGGL((k_render_aov<true, false>), dim3(a.n_blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_render_aov<false, false>), dim3(a.n_blocks), dim3(64), 0, st, a);
    FFX_CHECK_LAUNCH("render_fwd (aov)");
    return FFX_OK;
  }
  float *aov = a.out;
  a.out = (float *)rf_scratch;
  for (int g = 0; g < FFX_AOV_GROUPS; ++g) { // (check_filter: the filtered film runs on the wide walk)
    a.group = g;
    hipLaunchKernelGGL((k_render_aov<true, true>), dim3(a.n_blocks), dim3(64), 0, st, a);
    FFX_CHECK_LAUNCH("render_fwd_filtered (aov)");
    const int n_ch = FFX_RENDER_AOV_FLOATS - 3 * g < 3 ? FFX_RENDER_AOV_FLOATS - 3 * g : 3;
    hipLaunchKernelGGL(k_aov_gather, dim3(ffx_cdiv(r.c.cam.W, 64), r.c.cam.H), dim3(64), 0, st, (const float4 *)rf_scratch, r.c.cam.W, r.c.cam.H, aov, 3 * g, n_ch);
    FFX_CHECK_LAUNCH("render_fwd_filtered (aov)/gather");
  }
  return FFX_OK;
}
// the extra emitters' adjoint (FFX_RENDER_EMITTER_GRAD) belongs to ffx_render_bwd[_filtered]: every other render entry point refuses the bit
#define FFX_NO_EMITTER_GRAD(flags_, what_) \
  do { if ((flags_) & FFX_RENDER_EMITTER_GRAD) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_EMITTER_GRAD is served by ffx_render_bwd[_filtered] only", what_); } while (0)
// the extra emitters' bits belong to ffx_render_fwd[_filtered] (and are ignored by ffx_render_bwd[_filtered] without FFX_RENDER_EMITTER_GRAD): every other render
// entry point refuses them
#define FFX_NO_LIGHTS(flags_, what_) \
  do { \
    if ((flags_) & FFX_RENDER_LIGHTS_MASK) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_LIGHTS is served by ffx_render_fwd[_filtered] only", what_); \
    if ((flags_) & FFX_RENDER_AMBIENT) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_AMBIENT is served by ffx_render_fwd[_filtered] only", what_); \
    if ((flags_) & FFX_RENDER_LIGHTS_DIRECTIONAL) \
      FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_LIGHTS_DIRECTIONAL is served by ffx_render_fwd[_filtered] only", what_); \
    FFX_NO_EMITTER_GRAD(flags_, what_); \
  } while (0)
// FFX_RENDER_LIGHTS (include/ffx.h).  The three bits of the extra emitters: what each is called, who it stands for and the device buffer it reads (NULL: the table's bit reads nothing of its own)
struct EmitterBit { int mask; const char *name, *who, *buffer; };
static const EmitterBit kLightsBit = {FFX_RENDER_LIGHTS_MASK, "FFX_RENDER_LIGHTS", "the extra emitters are", "material table | lights"};
static const EmitterBit kAmbientBit = {FFX_RENDER_AMBIENT, "FFX_RENDER_AMBIENT", "the constant emitter is", "material table | lights | ambient"};
static const EmitterBit kDirectionalBit = {FFX_RENDER_LIGHTS_DIRECTIONAL, "FFX_RENDER_LIGHTS_DIRECTIONAL", "the extra emitters are", nullptr};
// a bit of the extra emitters beside a FFX_RENDER_GRAD_* bit: refused by the forwards and by ffx_render_bwd[_filtered] alike
static int emitter_bit_no_grad(int flags, const char *what, const EmitterBit &b) {
  if (flags & (FFX_RENDER_GRAD_APPEARANCE | FFX_RENDER_GRAD_MATERIAL | FFX_RENDER_GRAD_PRB))
    FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: %s is not served together with a FFX_RENDER_GRAD_* bit (%s not differentiated)", what, b.name, b.who);
  return FFX_OK;
}
// what a forward refuses about a set bit, the same for the three under each one's name
static int emitter_bit_check(int flags, const float *shape_albedo, const char *what, const EmitterBit &b) {
  if (flags & FFX_RENDER_FP16) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: %s has no fp16 film", what, b.name);
  if (flags & FFX_RENDER_TANGENT) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: %s is not served together with FFX_RENDER_TANGENT", what, b.name);
  if (const int rc = emitter_bit_no_grad(flags, what, b)) return rc;
  if (b.buffer && !shape_albedo) FFX_FAIL(FFX_ERR_ARG, "%s: %s needs the device buffer [%s] (shape_albedo is NULL)", what, b.name, b.buffer);
  return FFX_OK;
}
// what a forward refuses about the bits before it launches anything: FFX_OK, or the error
static int lights_check(int flags, const float *shape_albedo, const char *what) {
  const int n = (flags & FFX_RENDER_LIGHTS_MASK) >> FFX_RENDER_LIGHTS_SHIFT;
  if (flags & FFX_RENDER_AMBIENT) { // the constant emitter
    if (const int rc = emitter_bit_check(flags, shape_albedo, what, kAmbientBit)) return rc;
  }
  if (flags & FFX_RENDER_LIGHTS_DIRECTIONAL) { // directional records in the table: the bit belongs to a table, and is refused where the table is
    if (n == 0) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1): the bit says what the table may hold", what);
    if (const int rc = emitter_bit_check(flags, shape_albedo, what, kDirectionalBit)) return rc;
  }
  if (n == 0) return FFX_OK;
  if (n > FFX_RENDER_MAX_LIGHTS) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_LIGHTS(%d): at most %d extra emitters", what, n, FFX_RENDER_MAX_LIGHTS);
  return emitter_bit_check(flags, shape_albedo, what, kLightsBit);
}
// the emitters' records in the caller's device buffer [material table | lights | ambient]: behind the rows (mat_stride: 3 or FFX_MAT_STRIDE — max(mat_stride, 3))
static const float *lights_table(const float *shape_albedo, const ffx_scene_desc *sd, const RenderSetup &r) {
  return shape_albedo + (size_t)sd->n_shapes * (size_t)r.c.mat_stride;
}
// ... and the pass, behind the launches of the main image on the same stream (the call without the bits has succeeded: its arguments are good):
// k_lights_fwd adds to img; the gaussian film: into the scratch, which the image's (and an AOV block's) gathers have read by then, and k_lights_gather adds.
// One walk per sample serves the n lights (with FFX_RENDER_AMBIENT n may be 0), whatever their types, and the constant emitter
static int render_lights(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags, void *img,
                         ffx_stream s, void *rf_scratch) {
  const int n = (flags & FFX_RENDER_LIGHTS_MASK) >> FFX_RENDER_LIGHTS_SHIFT;
  RenderSetup r;
  if (const int rc = render_setup("render_fwd", bvh, info, sd, shape_albedo, spp, seed, flags & FFX_RENDER_PATH_MASK, rf_scratch, r)) return rc;
  if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_LIGHTS: more than 2^31 pixels");
  if (sd->n_shapes < 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd: n_shapes < 0");
  const float *table = lights_table(shape_albedo, sd, r);
  const PathArgs pa = path_args(r);
  const hipStream_t st = (hipStream_t)s;
  dispatch_rf_dir_amb(rf_scratch != nullptr, (flags & FFX_RENDER_LIGHTS_DIRECTIONAL) != 0, (flags & FFX_RENDER_AMBIENT) != 0, [&](auto rf, auto dir, auto amb) {
    hipLaunchKernelGGL((k_lights_fwd<decltype(rf)::value, decltype(dir)::value, decltype(amb)::value>), dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c,
                       pa, table, n, rf_scratch ? (float *)nullptr : (float *)img, (float *)rf_scratch);
  });
  FFX_CHECK_LAUNCH(rf_scratch ? "render_fwd_filtered (lights)" : "render_fwd (lights)");
  if (!rf_scratch) return FFX_OK;
  hipLaunchKernelGGL(k_lights_gather, dim3(ffx_cdiv(r.c.cam.W, 64), r.c.cam.H), dim3(64), 0, st, (const float4 *)rf_scratch, r.c.cam.W, r.c.cam.H, (float *)img);
  FFX_CHECK_LAUNCH("render_fwd_filtered (lights)/gather");
  return FFX_OK;
}
// ffx_render_fwd[_filtered] (scratch: the filtered film's): the call without the lights' bits, then their pass
static int render_fwd_entry(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp, uint32_t seed,
                            int img_fp16, void *img, ffx_stream s, void *scratch) {
  const char *what = scratch ? "render_fwd_filtered" : "render_fwd";
  FFX_NO_EMITTER_GRAD(img_fp16, what);
  if (const int rc = lights_check(img_fp16, shape_albedo, what)) return rc;
  FFX_NO_APPEARANCE(img_fp16, what);
  const int lights = img_fp16 & (FFX_RENDER_LIGHTS_MASK | FFX_RENDER_AMBIENT | FFX_RENDER_LIGHTS_DIRECTIONAL);
  img_fp16 &= ~(FFX_RENDER_LIGHTS_MASK | FFX_RENDER_AMBIENT | FFX_RENDER_LIGHTS_DIRECTIONAL);
  int rc;
  if (img_fp16 & FFX_RENDER_AOV) rc = render_aov(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16, img, s, scratch);
  else if (img_fp16 & FFX_RENDER_TANGENT) rc = render_jvp(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16, img, s, scratch);
  else rc = render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & (FFX_RENDER_FP16 | FFX_RENDER_APEX_READY | FFX_RENDER_PATH_MASK), img, nullptr, s,
                            nullptr, nullptr, nullptr, scratch);
  if (rc != FFX_OK || !lights) return rc;
  return render_lights(bvh, info, sd, shape_albedo, spp, seed, img_fp16 | lights, img, s, scratch);
}
int ffx_render_fwd(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                   uint32_t seed, int img_fp16, void *img, ffx_stream s) {
  return render_fwd_entry(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16, img, s, nullptr);
}
// the entry points without the path integrator refuse its bits rather than render direct light only
#define FFX_NO_PATH(flags_, what_) \
  do { if ((flags_) & FFX_RENDER_PATH_MASK) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: max_depth > 2 is served by ffx_render_fwd[_filtered] / ffx_render_bwd[_filtered] only", what_); } while (0)

size_t ffx_render_cache_bytes(int width, int height, int spp) {
  if (width < 1 || height < 1 || spp < 1) return 0;
  return cache_off_arena((size_t)width * height) + sizeof(CacheStray) * cache_stray_capacity(width, height, spp);
}

size_t ffx_render_cache_bytes_sd(const ffx_scene_desc *sd, int spp) {
  if (!sd || sd->cam.width < 1 || sd->cam.height < 1 || spp < 1) return 0;
  if (sd->rfilter != FFX_RFILTER_BOX) return rfc_bytes((size_t)sd->cam.width * sd->cam.height, (size_t)spp, sd->mat_stride == FFX_MAT_STRIDE, rfc_all(sd)); // the filtered film's cache
  if (sd->mat_stride != FFX_MAT_STRIDE) return ffx_render_cache_bytes(sd->cam.width, sd->cam.height, spp);
  const size_t n_pix = (size_t)sd->cam.width * sd->cam.height;
  return cache_off_foot_b(n_pix, cache_stray_capacity(sd->cam.width, sd->cam.height, spp)) + sizeof(CacheFoot) * n_pix;
}

int ffx_render_fwd_cache(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                         uint32_t seed, int img_fp16, void *img, void *cache, ffx_stream s) {
  if (!cache) FFX_FAIL(FFX_ERR_ARG, "render_fwd_cache: cache is NULL");
  if (((uintptr_t)cache & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd_cache: cache must be 16-byte aligned");
  FFX_NO_PATH(img_fp16, "render_fwd_cache");
  FFX_NO_APPEARANCE(img_fp16, "render_fwd_cache");
  FFX_NO_TANGENT(img_fp16, "render_fwd_cache");
  FFX_NO_AOV(img_fp16, "render_fwd_cache");
  FFX_NO_LIGHTS(img_fp16, "render_fwd_cache");
  return render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & 31, img, cache, s);
}

int ffx_render_cache_status(const void *cache, uint32_t *out3, ffx_stream s) {
  if (!cache || !out3) FFX_FAIL(FFX_ERR_ARG, "render_cache_status: bad argument");
  CacheHdr h;
  if (hipMemcpyAsync(&h, cache, sizeof h, hipMemcpyDeviceToHost, (hipStream_t)s) != hipSuccess || hipStreamSynchronize((hipStream_t)s) != hipSuccess)
    FFX_FAIL(FFX_ERR_LAUNCH, "render_cache_status: reading the cache header failed");
  out3[0] = h.n_stray; out3[1] = h.cap_stray; out3[2] = h.dropped;
  for (int i = 1; i <= 8; ++i) out3[0] += h.pad[i]; // (a filtered film's cache counts its blocks in eight sub-arenas; zero in a box film's)
  return FFX_OK;
}

int ffx_render_fwd_adjoint(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                           uint32_t seed, int img_fp16, void *img, const float *gimg, float *gtex, float *dot_out, ffx_stream s) {
  if (!gimg || !gtex) FFX_FAIL(FFX_ERR_ARG, "render_fwd_adjoint: gimg / gtex is NULL");
  if (sd && !sd->proj.enabled) FFX_FAIL(FFX_ERR_ARG, "render_fwd_adjoint: the scene has no projector (nothing to differentiate)");
  FFX_NO_PATH(img_fp16, "render_fwd_adjoint");
  FFX_NO_APPEARANCE(img_fp16, "render_fwd_adjoint");
  FFX_NO_TANGENT(img_fp16, "render_fwd_adjoint");
  FFX_NO_AOV(img_fp16, "render_fwd_adjoint");
  FFX_NO_LIGHTS(img_fp16, "render_fwd_adjoint");
  return render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & (FFX_RENDER_FP16 | FFX_RENDER_SPARSE_ADJOINT | FFX_RENDER_APEX_READY), img, nullptr, s, gimg,
                         gtex, dot_out);
}

int ffx_apex_prepare(void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, ffx_stream s) {
  if (!bvh || !info || !sd) FFX_FAIL(FFX_ERR_ARG, "apex_prepare: bad argument");
  if (!check_info(info, "apex_prepare")) return FFX_ERR_ARG;
  const TriApex *arecs;
  uint32_t astride;
  if (!launch_apex(bvh, info, sd->cam.to_world, sd, &arecs, &astride, (hipStream_t)s)) return FFX_ERR_ARG;
  FFX_CHECK_LAUNCH("apex_prepare");
  return FFX_OK;
}

// at most 256 slots (one per 8x8-pixel block, folded modulo 256): enough to take the contention out of the atomics (a 512x512 film
// adds 16 values to each) and few enough for ONE load per thread of the launch that sums them (ffx_pattern_bwd's block 0)
size_t ffx_render_dot_slots(int width, int height) {
  if (width < 1 || height < 1) return 0;
  const size_t b = (size_t)ffx_cdiv(width, 8) * (size_t)ffx_cdiv(height, 8);
  return b < 256 ? b : 256;
}

static int render_bwd_cached_impl(const ffx_scene_desc *sd, const float *shape_albedo, const void *cache, int spp, const float *gimg, float *gtex, const void *img,
                                  int img_fp16, float *dot_out, const float *l1_target, float l1_weight, ffx_stream s);
int ffx_render_bwd_cached(const ffx_scene_desc *sd, const float *shape_albedo, const void *cache, int spp, const float *gimg, float *gtex, const void *img,
                          int img_fp16, float *dot_out, ffx_stream s) {
  if (!gimg) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached: bad argument");
  FFX_NO_PATH(img_fp16, "render_bwd_cached");
  FFX_NO_APPEARANCE(img_fp16, "render_bwd_cached");
  FFX_NO_TANGENT(img_fp16, "render_bwd_cached");
  FFX_NO_AOV(img_fp16, "render_bwd_cached");
  FFX_NO_EMITTER_GRAD(img_fp16, "render_bwd_cached");
  return render_bwd_cached_impl(sd, shape_albedo, cache, spp, gimg, gtex, img, img_fp16, dot_out, nullptr, 0.f, s);
}
// K9 under an L1 loss against a target image (include/ffx.h): the loss launch (ffx_l1_value_grad) and its gradient image are folded into the scatter
int ffx_render_bwd_cached_l1(const ffx_scene_desc *sd, const float *shape_albedo, const void *cache, int spp, const float *img, const float *target, float weight,
                             float *gtex, float *loss_slots, ffx_stream s) {
  if (!img || !target || !loss_slots) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached_l1: bad argument");
  if (sd && (!sd->proj.enabled || sd->proj.tex_channels != 1)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached_l1: a projector with a one-channel texture (else ffx_l1_value_grad + ffx_render_bwd_cached)");
  return render_bwd_cached_impl(sd, shape_albedo, cache, spp, nullptr, gtex, img, 0, loss_slots, target, weight, s);
}
static int render_bwd_cached_impl(const ffx_scene_desc *sd, const float *shape_albedo, const void *cache, int spp, const float *gimg, float *gtex, const void *img,
                                  int img_fp16, float *dot_out, const float *l1_target, float l1_weight, ffx_stream s) {
  if (!sd || (!shape_albedo && sd->n_mat_h <= 0) || !cache || (!gimg && !l1_target) || !gtex || spp < 1 || (dot_out && !img)) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached: bad argument");
  if (sd->rfilter != FFX_RFILTER_BOX) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached: the scene's reconstruction filter is not the box (use ffx_render_bwd_filtered)");
  if (!sd->proj.enabled) {
    if (dot_out) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached: <gimg, img> is accumulated by the footprint kernel, which a scene without projector does not launch");
    return FFX_OK;
  }
  BwdP p;
  memset(&p, 0, sizeof p);
  p.mats = shape_albedo;
  if (!copy_mat_h(sd, sd->mat_stride ? sd->mat_stride : 3, p)) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached: n_mat_h must be n_shapes x stride (<= %d)", FFX_MAX_MAT_H);
  p.img = dot_out ? img : nullptr; p.img_fp16 = img_fp16 & 1; p.dot_out = dot_out;
  p.dot_slots = (int)ffx_render_dot_slots(sd->cam.width, sd->cam.height);
  if (l1_target) { // (sign(img - target) * weight / n per element; value weight / n * sum |img - target|: ffx_l1_value_grad's)
    const float n_el = 3.0f * (float)sd->cam.width * (float)sd->cam.height;
    p.l1_tgt = l1_target; p.l1_gs = l1_weight / n_el; p.l1_vs = l1_weight / n_el;
  }
  p.tw = sd->proj.tex_w; p.th = sd->proj.tex_h; p.tc = sd->proj.tex_channels; p.spp = spp;
  if (p.tw < 1 || p.th < 1 || (p.tc != 1 && p.tc != 3) || sd->cam.width < 1 || sd->cam.height < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached: bad scene description");
  for (int i = 0; i < 3; ++i) p.color[i] = sd->proj.color[i];
  p.inv_spp = 1.0f / (float)spp;
  const long n_pix = (long)sd->cam.width * sd->cam.height;
  p.W = sd->cam.width; p.H = sd->cam.height;
  p.ms = sd->mat_stride ? sd->mat_stride : 3;
  if (p.ms != 3 && p.ms != FFX_MAT_STRIDE) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached: bad material stride");
  p.off_foot_b = cache_off_foot_b((size_t)n_pix, cache_stray_capacity(sd->cam.width, sd->cam.height, spp));
  const int stray_blocks = ffx_cdiv((long)cache_stray_capacity(sd->cam.width, sd->cam.height, spp), 256);
  if (p.tc == 1) {
    // footprints by 16x16-pixel blocks through an LDS tile; the tail of the grid replays the stray records
    const int blocks_x = ffx_cdiv(p.W, 16), blocks_y = ffx_cdiv(p.H, 16);
    hipLaunchKernelGGL(k_render_bwd_cached_tiled16, dim3(blocks_x * blocks_y + stray_blocks), dim3(256), 0, (hipStream_t)s, p, (const char *)cache, blocks_x,
                       blocks_x * blocks_y, gimg, gtex);
    FFX_CHECK_LAUNCH("render_bwd_cached/tiled16");
    return FFX_OK;
  }
  const int slot_blocks = ffx_cdiv(n_pix, 8);
  hipLaunchKernelGGL(k_render_bwd_cached, dim3(slot_blocks + stray_blocks), dim3(256), 0, (hipStream_t)s, p, (const char *)cache, n_pix, slot_blocks, gimg, gtex);
  FFX_CHECK_LAUNCH("render_bwd_cached");
  return FFX_OK;
}

static int render_bwd_impl(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                           const float *gimg, float *gtex, ffx_stream s, void *rf_scratch, void *det_ws = nullptr, const DetPart *det_part = nullptr) {
  if (!bvh || !info || !sd || (!shape_albedo && sd->n_mat_h <= 0) || !gimg || (!gtex && !det_part) || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd: bad argument");
  // (the filter is refused before a scene without projector returns, and that before the bvh info is looked at; render_setup's repeat then passes)
  if (const int rc = check_filter("render_bwd", sd, info, rf_scratch)) return rc;
  if (!sd->proj.enabled) return FFX_OK;
  RenderSetup r;
  if (const int rc = render_setup("render_bwd", bvh, info, sd, shape_albedo, spp, seed, flags, rf_scratch, r)) return rc;
  const hipStream_t st = (hipStream_t)s;
  if (r.max_depth > 2) { // the path integrator's adjoint: replays the forward's paths
    if (det_ws || det_part) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_det: max_depth > 2 has no deterministic adjoint");
    if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd: more than 2^31 pixels");
    const PathArgs pa = path_args(r);
    if (rf_scratch) { // G = gimg / weight as in the re-tracing filtered adjoint below
      const float4 *G = rf_G(r, gimg, rf_scratch, st, "render_bwd_filtered (path)/weights", "render_bwd_filtered (path)/gather");
      if (!G) return FFX_ERR_LAUNCH;
      hipLaunchKernelGGL(k_path_bwd<true>, dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, (const float *)G, gtex);
      FFX_CHECK_LAUNCH("render_bwd_filtered (path)");
      return FFX_OK;
    }
    hipLaunchKernelGGL(k_path_bwd<false>, dim3((unsigned)r.n_pix), dim3(64), path_stack_bytes(info), st, r.c, pa, gimg, gtex);
    FFX_CHECK_LAUNCH("render_bwd (path)");
    return FFX_OK;
  }
  if (use_packet() && !r.b.gn) FFX_FAIL(FFX_ERR_ARG, "render_bwd: blob without per-slot normals (built by another library version?)");
  if (use_packet()) {
    Packets p;
    packet_grid(p, r.c.cam, tile_block_log2(r.n_pix), 4);
    if (!launch_apex(bvh, info, sd->cam.to_world, sd, &p.arecs, &p.astride, st, nullptr, 0, flags & FFX_RENDER_APEX_READY)) return FFX_ERR_ARG;
    p.ws = wide_scene(bvh, info);
    bins_k(bvh, info, sd, r.c.bins);
    DetK det;
    memset(&det, 0, sizeof det);
    const float *gsrc = gimg; // what the kernel gathers from: gimg, or (filtered film) G = gimg / weight as float4 per pixel
    if (rf_scratch) {
      // 1. the weight every pixel received (jitter only) -> G = gimg / weight behind the partial sums; 2. the re-trace gathers through the filter
      gsrc = (const float *)rf_G(r, gimg, rf_scratch, st, "render_bwd_filtered/weights", "render_bwd_filtered/gather");
      if (!gsrc) return FFX_ERR_LAUNCH;
    }
    const bool wide = use_wide(info) != 0;
    auto launch = [&]() {
      if (rf_scratch) launch_bwd_pk<true>(true, r, p, gsrc, gtex, det, st);
      else launch_bwd_pk<false>(wide, r, p, gsrc, gtex, det, st);
    };
    if (det_part) { // one pass of the deterministic accumulation alone: the caller owns the accumulators and the scale (ffx_render_bwd_det_part)
      det.mode = det_part->part;
      det.vmax = det_part->vmax;
      det.fix = det_part->fix;
      det.scale = ldexpf(1.0f, det_part->scale_log2);
      launch();
      FFX_CHECK_LAUNCH(det_part->part == 1 ? "render_bwd_det_part/max" : "render_bwd_det_part/sum");
      return FFX_OK;
    }
    if (det_ws) {
      // deterministic accumulation (DetK above): the largest tap of the launch -> a power-of-two scale -> 64-bit fixed-point sums -> gtex.  The
      // scale needs the first pass's result on the host: ONE 4-byte read and a stream synchronisation per call (a debugging / cross-checking mode)
      const long n_t = (long)r.c.tw * r.c.th * r.c.tc;
      det.fix = (unsigned long long *)det_ws;
      det.vmax = (unsigned int *)(det.fix + n_t);
      if (hipMemsetAsync(det_ws, 0, (size_t)n_t * 8 + 8, st) != hipSuccess) FFX_FAIL(FFX_ERR_LAUNCH, "render_bwd_det: clearing the workspace failed");
      det.mode = 1;
      launch();
      FFX_CHECK_LAUNCH("render_bwd_det/max");
      unsigned int vbits = 0;
      if (hipMemcpyAsync(&vbits, det.vmax, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        FFX_FAIL(FFX_ERR_LAUNCH, "render_bwd_det: reading the largest tap failed");
      float vmax;
      memcpy(&vmax, &vbits, 4);
      if (!(vmax > 0.f)) return FFX_OK; // nothing lit: gtex unchanged
      if (!(vmax < 3.0e38f)) { // a non-finite tap: the plain adjoint reports it (NaN / inf in gtex)
        det.mode = 0;
        launch();
        FFX_CHECK_LAUNCH("render_bwd_det/non-finite");
        return FFX_OK;
      }
      // (b = bits of this launch's tap count — 4 taps per sample: 2^-36 of the largest tap at 512 x 512 x 64 spp; a fixed b = 34 — room for 2^32
      // samples — had left 2^-28, round-5 advisor)
      const int sh = det_scale_log2(vbits, 4ull * (unsigned long long)r.c.cam.W * (unsigned long long)r.c.cam.H * (unsigned long long)(spp > 0 ? spp : 1));
      det.scale = ldexpf(1.0f, sh);
      det.mode = 2;
      launch();
      FFX_CHECK_LAUNCH("render_bwd_det/sum");
      hipLaunchKernelGGL(k_det_finish, dim3(ffx_cdiv(n_t, 256)), dim3(256), 0, st, det.fix, 1.0f / det.scale, n_t, gtex);
      FFX_CHECK_LAUNCH("render_bwd_det/finish");
      return FFX_OK;
    }
    launch();
    FFX_CHECK_LAUNCH(rf_scratch ? "render_bwd_filtered" : "render_bwd");
    return FFX_OK;
  }
  if (det_ws || det_part) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_det: the per-lane kernels (FFX_TRAVERSAL=lane) have no deterministic mode");
  int tiles_x = ffx_cdiv(r.c.cam.W, 8), tiles_y = ffx_cdiv(r.c.cam.H, 8);
  int n_tiles = tiles_x * tiles_y;
  int grid = ((n_tiles + 7) / 8) * 8;
  hipLaunchKernelGGL(k_render_bwd, dim3(grid), dim3(TR_BLOCK), stack_bytes(info), st, r.c, r.b.nodes, r.b.recs, r.b.nrec, shape_albedo, spp, r.seed_key,
                     tiles_x, n_tiles, xcd_mode(), gimg, gtex);
  FFX_CHECK_LAUNCH("render_bwd");
  return FFX_OK;
}

// what both appearance routes set up after their own refusals: render_setup, the n_shapes / texture-size checks and the kernels' AppArgs over the layout
// of gimg (the forward's texture behind the image gradient) and gtex (the appearance block behind the texture's n_tex floats)
static int app_args(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                    const float *gimg, float *gtex, void *rf_scratch, RenderSetup &r, AppArgs &a, long &n_tex) {
  if (const int rc = render_setup("render_bwd", bvh, info, sd, shape_albedo, spp, seed, flags, rf_scratch, r)) return rc;
  if (sd->n_shapes < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd: n_shapes < 1");
  n_tex = (long)sd->proj.tex_w * sd->proj.tex_h * sd->proj.tex_channels;
  if (n_tex < 0) FFX_FAIL(FFX_ERR_ARG, "render_bwd: bad projector texture size");
  memset(&a, 0, sizeof a);
  a.nodes = r.b.nodes; a.recs = r.b.recs; a.nrec = r.b.nrec;
  a.tex = sd->proj.enabled ? gimg + (size_t)r.n_pix * 3 : nullptr;
  a.spp = spp; a.n_pix = (int)r.n_pix; a.n_shapes = sd->n_shapes; a.seed_key = r.seed_key;
  a.grow = gtex + n_tex; a.gspot = a.grow + (size_t)3 * sd->n_shapes;
  float *bt = a.gspot + 3;
  for (int k = 0; k < r.c.n_base_tex; ++k) {
    a.gbt[k] = bt;
    bt += (size_t)3 * r.c.btw[k] * r.c.bth[k];
  }
  return FFX_OK;
}
// FFX_RENDER_GRAD_APPEARANCE (include/ffx.h): after the texture part — the launches of a call without the bit, which leave G = gimg / weight
// in the filtered film's scratch when the scene has a projector — one launch of k_render_bwd_appearance (with FFX_RENDER_GRAD_MATERIAL:
// k_render_bwd_material, FFX_RENDER_MATERIAL_FLOATS(sd) more floats) into the block behind gtex
static int render_bwd_appearance(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                                 const float *gimg, float *gtex, ffx_stream s, void *rf_scratch) {
  if (flags & FFX_RENDER_PATH_MASK) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_GRAD_APPEARANCE is served at max_depth 2 only");
  if (const int rc = render_bwd_impl(bvh, info, sd, shape_albedo, spp, seed, flags & ~(FFX_RENDER_GRAD_APPEARANCE | FFX_RENDER_GRAD_MATERIAL), gimg, gtex, s, rf_scratch))
    return rc;
  RenderSetup r;
  AppArgs a;
  long n_tex;
  if (const int rc = app_args(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, rf_scratch, r, a, n_tex)) return rc;
  const hipStream_t st = (hipStream_t)s;
  const float *gsrc = gimg;
  if (rf_scratch) { // G = gimg / weight: the texture part left it in the scratch, or (no projector) launched nothing and it is formed here
    gsrc = (const float *)(sd->proj.enabled ? rf_G_area(rf_scratch, r.n_pix)
                                            : rf_G(r, gimg, rf_scratch, st, "render_bwd_filtered (appearance)/weights", "render_bwd_filtered (appearance)/gather"));
    if (!gsrc) return FFX_ERR_LAUNCH;
  }
  const long blocks = ffx_cdiv(r.n_pix, (long)FFX_APP_WAVES);
  const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048); // (every workgroup strides over the film: 2048 x 4 waves fill the device)
  const bool material = (flags & FFX_RENDER_GRAD_MATERIAL) != 0;
  float *gmat = gtex + n_tex + FFX_RENDER_APPEARANCE_FLOATS(sd);
  dispatch_rf_mat(rf_scratch != nullptr, material, [&](auto rf, auto m) {
    constexpr bool RF = decltype(rf)::value;
    if constexpr (decltype(m)::value) hipLaunchKernelGGL(k_render_bwd_material<RF>, dim3(grid), dim3(64 * FFX_APP_WAVES), stack_bytes(info), st, r.c, a, gsrc, gmat);
    else hipLaunchKernelGGL(k_render_bwd_appearance<RF>, dim3(grid), dim3(64 * FFX_APP_WAVES), stack_bytes(info), st, r.c, a, gsrc);
  });
  FFX_CHECK_LAUNCH(material ? (rf_scratch ? "render_bwd_filtered (material)" : "render_bwd (material)")
                            : (rf_scratch ? "render_bwd_filtered (appearance)" : "render_bwd (appearance)"));
  return FFX_OK;
}
// FFX_RENDER_GRAD_PRB (include/ffx.h): the appearance (and material) blocks at max_depth > 2 — ONE launch of k_path_bwd_prb[_material],
// which also forms the texture part (k_path_bwd's sum) while it replays the paths
#define FFX_PRB_STATIC_LDS ((FFX_APP_LDS_ROWS * 3 + FFX_MAT_LDS_ROWS * FFX_MAT_GRAD_COLS) * sizeof(float))
static int render_bwd_prb(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                          const float *gimg, float *gtex, ffx_stream s, void *rf_scratch) {
  RenderSetup r;
  AppArgs a;
  long n_tex;
  if (const int rc = app_args(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, rf_scratch, r, a, n_tex)) return rc;
  if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd: more than 2^31 pixels");
  const hipStream_t st = (hipStream_t)s;
  const bool material = (flags & FFX_RENDER_GRAD_MATERIAL) != 0;
  PrbArgs p;
  p.max_depth = r.max_depth; p.rr_depth = r.rr_depth; p.path_key = path_args(r).path_key;
  p.gtex = gtex; p.gmat = material ? gtex + n_tex + FFX_RENDER_APPEARANCE_FLOATS(sd) : nullptr;
  const float *gsrc = gimg;
  if (rf_scratch) {
    gsrc = (const float *)rf_G(r, gimg, rf_scratch, st, "render_bwd_filtered (prb)/weights", "render_bwd_filtered (prb)/gather");
    if (!gsrc) return FFX_ERR_LAUNCH;
  }
  // LDS per wave: the traversal stack and the path records [max_depth - 1][6] per lane; the widest workgroup (4, 2, 1 waves) that stays inside 64 KB
  const int depth = info->max_depth < 8 ? 8 : info->max_depth;
  const size_t wave_stack = (size_t)depth * 64 * sizeof(int), wave_path = (size_t)(r.max_depth - 1) * 6 * 64 * sizeof(float);
  int waves = FFX_APP_WAVES;
  while (waves > 1 && waves * (wave_stack + wave_path) + FFX_PRB_STATIC_LDS > 65536) waves >>= 1;
  const size_t dyn = waves * (wave_stack + wave_path);
  const int stack_ints = depth * 64 * waves;
  const long blocks = ffx_cdiv(r.n_pix, (long)waves), cap = 8192 / waves; // (every workgroup strides over the film, as k_render_bwd_appearance's)
  const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
  dispatch_rf_mat(rf_scratch != nullptr, material, [&](auto rf, auto m) {
    constexpr bool RF = decltype(rf)::value;
    if constexpr (decltype(m)::value) hipLaunchKernelGGL(k_path_bwd_prb_material<RF>, dim3(grid), dim3(64 * waves), dyn, st, r.c, a, p, gsrc, stack_ints);
    else hipLaunchKernelGGL(k_path_bwd_prb<RF>, dim3(grid), dim3(64 * waves), dyn, st, r.c, a, p, gsrc, stack_ints);
  });
  FFX_CHECK_LAUNCH(material ? (rf_scratch ? "render_bwd_filtered (prb, material)" : "render_bwd (prb, material)")
                            : (rf_scratch ? "render_bwd_filtered (prb)" : "render_bwd (prb)"));
  return FFX_OK;
}
// FFX_RENDER_GRAD_MATERIAL and FFX_RENDER_GRAD_PRB extend FFX_RENDER_GRAD_APPEARANCE: alone each is an argument error
#define FFX_MATERIAL_NEEDS_APPEARANCE(flags_, what_)                                                                                      \
  do {                                                                                                                                    \
    if (((flags_) & (FFX_RENDER_GRAD_MATERIAL | FFX_RENDER_GRAD_APPEARANCE)) == FFX_RENDER_GRAD_MATERIAL)                                 \
      FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_GRAD_MATERIAL needs FFX_RENDER_GRAD_APPEARANCE", what_);                                      \
    if (((flags_) & FFX_RENDER_GRAD_PRB) && !((flags_) & FFX_RENDER_GRAD_APPEARANCE))                                                     \
      FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_GRAD_PRB needs FFX_RENDER_GRAD_APPEARANCE", what_);                                           \
  } while (0)
// the appearance route of a flags word: with FFX_RENDER_GRAD_PRB and max_depth > 2 (or a bad depth field, which render_setup reports) the path replay;
// else the direct-light kernels, which ignore the bit (and refuse path bits without it, as before)
static int render_bwd_leaves(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                             const float *gimg, float *gtex, ffx_stream s, void *rf_scratch) {
  if (!bvh || !info || !sd || (!shape_albedo && sd->n_mat_h <= 0) || !gimg || !gtex || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd: bad argument");
  if (flags & FFX_RENDER_GRAD_PRB) {
    int md, rr;
    if (!path_depths(flags, md, rr) || md > 2) return render_bwd_prb(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, rf_scratch);
    flags &= ~(FFX_RENDER_GRAD_PRB | FFX_RENDER_PATH_MASK); // (max_depth 2: direct light, whatever rr_depth says)
  }
  return render_bwd_appearance(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, rf_scratch);
}
// FFX_RENDER_EMITTER_GRAD (include/ffx.h), behind the entry points' own refusals (the lights' bits beside a GRAD bit among them): the texture
// part — the launches of the call without the bit, which ignore the lights' bits and leave G = gimg / weight in the filtered film's scratch when the scene has
// a projector — then k_lights_bwd into the workspace behind the result block and k_lights_grad_reduce into the block.  `what`: the entry point's name
static int render_bwd_emitters(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                               const float *gimg, float *gtex, ffx_stream s, void *rf_scratch) {
  const char *what = rf_scratch ? "render_bwd_filtered" : "render_bwd";
  if (flags & (FFX_RENDER_GRAD_APPEARANCE | FFX_RENDER_GRAD_MATERIAL | FFX_RENDER_GRAD_PRB))
    FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_EMITTER_GRAD is not served together with FFX_RENDER_GRAD_APPEARANCE, FFX_RENDER_GRAD_MATERIAL or FFX_RENDER_GRAD_PRB", what);
  const int n = (flags & FFX_RENDER_LIGHTS_MASK) >> FFX_RENDER_LIGHTS_SHIFT;
  const bool amb = (flags & FFX_RENDER_AMBIENT) != 0;
  if (n == 0 && !amb) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_EMITTER_GRAD needs FFX_RENDER_LIGHTS(n >= 1) or FFX_RENDER_AMBIENT: there is nothing to differentiate", what);
  if (n == 0 && (flags & FFX_RENDER_LIGHTS_DIRECTIONAL))
    FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1): the bit says what the table may hold", what);
  if (n > FFX_RENDER_MAX_LIGHTS) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_LIGHTS(%d): at most %d extra emitters", what, n, FFX_RENDER_MAX_LIGHTS);
  if (!shape_albedo) FFX_FAIL(FFX_ERR_ARG, "%s: FFX_RENDER_EMITTER_GRAD needs the device buffer [material table | lights | ambient] (shape_albedo is NULL)", what);
  const int plain = flags & ~(FFX_RENDER_EMITTER_GRAD | FFX_RENDER_LIGHTS_MASK | FFX_RENDER_AMBIENT | FFX_RENDER_LIGHTS_DIRECTIONAL); // (the call without the bits)
  if (const int rc = render_bwd_impl(bvh, info, sd, shape_albedo, spp, seed, plain, gimg, gtex, s, rf_scratch)) return rc;
  RenderSetup r;
  if (const int rc = render_setup("render_bwd", bvh, info, sd, shape_albedo, spp, seed, flags & FFX_RENDER_PATH_MASK, rf_scratch, r)) return rc;
  if (r.n_pix >= (1L << 31)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "%s: FFX_RENDER_EMITTER_GRAD: more than 2^31 pixels", what);
  if (sd->n_shapes < 0) FFX_FAIL(FFX_ERR_ARG, "%s: n_shapes < 0", what);
  const long n_tex = (long)sd->proj.tex_w * sd->proj.tex_h * sd->proj.tex_channels;
  if (n_tex < 0) FFX_FAIL(FFX_ERR_ARG, "%s: bad projector texture size", what);
  const float *table = lights_table(shape_albedo, sd, r);
  float *block = gtex + n_tex, *slots = block + FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS;
  const PathArgs pa = path_args(r);
  const hipStream_t st = (hipStream_t)s;
  const float *gsrc = gimg;
  if (rf_scratch) { // G = gimg / weight: the texture part left it in the scratch, or (no projector) launched nothing and it is formed here
    gsrc = (const float *)(sd->proj.enabled ? rf_G_area(rf_scratch, r.n_pix)
                                            : rf_G(r, gimg, rf_scratch, st, "render_bwd_filtered (emitters)/weights", "render_bwd_filtered (emitters)/gather"));
    if (!gsrc) return FFX_ERR_LAUNCH;
  }
  const size_t stack = path_stack_bytes(info); // (dynamic LDS: the lanes' traversal stacks, then their 3 n record sums)
  dispatch_rf_mat(rf_scratch != nullptr, amb, [&](auto rf, auto am) {
    hipLaunchKernelGGL((k_lights_bwd<decltype(rf)::value, decltype(am)::value>), dim3((unsigned)r.n_pix), dim3(64), stack + (size_t)3 * n * 64 * sizeof(float), st, r.c, pa,
                       table, n, gsrc, slots, (int)(stack / sizeof(int)));
  });
  FFX_CHECK_LAUNCH(rf_scratch ? "render_bwd_filtered (emitters)" : "render_bwd (emitters)");
  hipLaunchKernelGGL(k_lights_grad_reduce, dim3(FFX_RENDER_EMITTER_GRAD_BLOCK_FLOATS), dim3(FFX_EG_REDUCE_THREADS), 0, st, (const float *)slots, (int)r.n_pix, n, (int)amb, block);
  FFX_CHECK_LAUNCH(rf_scratch ? "render_bwd_filtered (emitters)/reduce" : "render_bwd (emitters)/reduce");
  return FFX_OK;
}

// ffx_render_bwd[_filtered] (scratch: the filtered film's): what both refuse about the flags, then the adjoint the flags name
static int render_bwd_entry(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                            const float *gimg, float *gtex, ffx_stream s, void *scratch) {
  const char *what = scratch ? "render_bwd_filtered" : "render_bwd";
  FFX_NO_TANGENT(flags, what);
  FFX_NO_AOV(flags, what);
  FFX_MATERIAL_NEEDS_APPEARANCE(flags, what);
  for (const EmitterBit *b : {&kLightsBit, &kAmbientBit, &kDirectionalBit}) {
    if (flags & b->mask) {
      if (const int rc = emitter_bit_no_grad(flags, what, *b)) return rc;
    }
  }
  if (flags & FFX_RENDER_EMITTER_GRAD) return render_bwd_emitters(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, scratch);
  flags &= ~(FFX_RENDER_LIGHTS_MASK | FFX_RENDER_AMBIENT | FFX_RENDER_LIGHTS_DIRECTIONAL); // (the texture's adjoint sees neither the extra emitters nor the constant one: the bits are ignored, the tail behind the table is not read)
  if (flags & FFX_RENDER_GRAD_APPEARANCE) return render_bwd_leaves(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, scratch);
  return render_bwd_impl(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, scratch);
}
int ffx_render_bwd(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                   const float *gimg, float *gtex, ffx_stream s) {
  return render_bwd_entry(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, nullptr);
}

size_t ffx_render_bwd_det_bytes(const ffx_scene_desc *sd) {
  if (!sd || sd->proj.tex_w < 1 || sd->proj.tex_h < 1 || (sd->proj.tex_channels != 1 && sd->proj.tex_channels != 3)) return 0;
  return (size_t)sd->proj.tex_w * sd->proj.tex_h * sd->proj.tex_channels * 8 + 8 + (sd->rfilter != FFX_RFILTER_BOX ? ffx_render_filter_bytes(sd) : 0);
}

int ffx_render_bwd_det(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                       const float *gimg, float *gtex, void *workspace, ffx_stream s) {
  if (!workspace || ((uintptr_t)workspace & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_bwd_det: workspace is NULL or not 16-byte aligned");
  if (!sd) FFX_FAIL(FFX_ERR_ARG, "render_bwd_det: bad argument");
  FFX_NO_PATH(flags, "render_bwd_det");
  FFX_NO_APPEARANCE(flags, "render_bwd_det");
  FFX_NO_TANGENT(flags, "render_bwd_det");
  FFX_NO_AOV(flags, "render_bwd_det");
  FFX_NO_LIGHTS(flags, "render_bwd_det");
  // workspace: [the filtered film's scratch (16-byte multiple)] [one 64-bit sum per texel and channel] [the largest tap]
  void *rf = sd->rfilter != FFX_RFILTER_BOX ? workspace : nullptr;
  void *det = (char *)workspace + (rf ? ffx_render_filter_bytes(sd) : 0);
  return render_bwd_impl(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, rf, det);
}

int ffx_render_bwd_det_part(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                            const float *gimg, int part, int scale_log2, void *acc, void *workspace, ffx_stream s) {
  if (!sd || !acc || (part != 1 && part != 2) || ((uintptr_t)acc & (part == 1 ? 3 : 7)) != 0) FFX_FAIL(FFX_ERR_ARG, "render_bwd_det_part: bad argument");
  if (scale_log2 < -126 || scale_log2 > 126) FFX_FAIL(FFX_ERR_ARG, "render_bwd_det_part: scale_log2 out of range");
  FFX_NO_PATH(flags, "render_bwd_det_part");
  FFX_NO_APPEARANCE(flags, "render_bwd_det_part");
  FFX_NO_TANGENT(flags, "render_bwd_det_part");
  FFX_NO_AOV(flags, "render_bwd_det_part");
  FFX_NO_LIGHTS(flags, "render_bwd_det_part");
  void *rf = nullptr;
  if (sd->rfilter != FFX_RFILTER_BOX) {
    if (!workspace || ((uintptr_t)workspace & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_bwd_det_part: a filtered film needs its scratch (ffx_render_filter_bytes), 16-byte aligned");
    rf = workspace;
  }
  DetPart dp;
  dp.part = part; dp.scale_log2 = scale_log2;
  dp.vmax = part == 1 ? (unsigned int *)acc : nullptr;
  dp.fix = part == 2 ? (unsigned long long *)acc : nullptr;
  return render_bwd_impl(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, nullptr, s, rf, nullptr, &dp);
}
int ffx_det_scale_log2(uint32_t vmax_bits, uint64_t n_taps) { return det_scale_log2(vmax_bits, (unsigned long long)n_taps); }
int ffx_det_finish(const void *acc, int scale_log2, size_t n, float *gtex, ffx_stream s) {
  if (!acc || !gtex || n == 0 || scale_log2 < -126 || scale_log2 > 126) FFX_FAIL(FFX_ERR_ARG, "det_finish: bad argument");
  hipLaunchKernelGGL(k_det_finish, dim3(ffx_cdiv((long)n, 256)), dim3(256), 0, (hipStream_t)s, (const unsigned long long *)acc, ldexpf(1.0f, -scale_log2), (long)n, gtex);
  FFX_CHECK_LAUNCH("det_finish");
  return FFX_OK;
}

// scratch of the filtered calls: [pixel][25][4] outgoing sums (400 B per pixel) + G = gimg / weight as float4 per pixel (the adjoint)
size_t ffx_render_filter_bytes(const ffx_scene_desc *sd) {
  if (!sd || sd->cam.width < 1 || sd->cam.height < 1) return 0;
  return (size_t)sd->cam.width * sd->cam.height * (25 * 4 + 4) * sizeof(float);
}

int ffx_render_fwd_filtered(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                            uint32_t seed, int img_fp16, void *img, void *scratch, ffx_stream s) {
  if (!scratch || ((uintptr_t)scratch & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd_filtered: scratch is NULL or not 16-byte aligned");
  return render_fwd_entry(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16, img, s, scratch);
}

int ffx_render_fwd_adjoint_filtered(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                                    uint32_t seed, int img_fp16, void *img, const float *gimg, float *gtex, void *scratch, ffx_stream s) {
  if (!gimg || !gtex) FFX_FAIL(FFX_ERR_ARG, "render_fwd_adjoint_filtered: gimg / gtex is NULL");
  if (!scratch || ((uintptr_t)scratch & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd_adjoint_filtered: scratch is NULL or not 16-byte aligned");
  if (sd && !sd->proj.enabled) FFX_FAIL(FFX_ERR_ARG, "render_fwd_adjoint_filtered: the scene has no projector (nothing to differentiate)");
  FFX_NO_PATH(img_fp16, "render_fwd_adjoint_filtered");
  FFX_NO_APPEARANCE(img_fp16, "render_fwd_adjoint_filtered");
  FFX_NO_TANGENT(img_fp16, "render_fwd_adjoint_filtered");
  FFX_NO_AOV(img_fp16, "render_fwd_adjoint_filtered");
  FFX_NO_LIGHTS(img_fp16, "render_fwd_adjoint_filtered");
  return render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed, img_fp16 & (FFX_RENDER_FP16 | FFX_RENDER_SPARSE_ADJOINT | FFX_RENDER_APEX_READY), img, nullptr, s, gimg,
                         gtex, nullptr, scratch);
}

int ffx_render_bwd_filtered(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, int spp, uint32_t seed, int flags,
                            const float *gimg, float *gtex, void *scratch, ffx_stream s) {
  if (!scratch || ((uintptr_t)scratch & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_bwd_filtered: scratch is NULL or not 16-byte aligned");
  return render_bwd_entry(bvh, info, sd, shape_albedo, spp, seed, flags, gimg, gtex, s, scratch);
}

int ffx_render_fwd_cache_filtered(const void *bvh, const ffx_bvh_info *info, const ffx_scene_desc *sd, const float *shape_albedo, const float *tex, int spp,
                                  uint32_t seed, int img_fp16, void *img, void *cache, void *scratch, ffx_stream s) {
  if (!cache || ((uintptr_t)cache & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd_cache_filtered: cache is NULL or not 16-byte aligned");
  if (!scratch || ((uintptr_t)scratch & 15) != 0) FFX_FAIL(FFX_ERR_ARG, "render_fwd_cache_filtered: scratch is NULL or not 16-byte aligned");
  FFX_NO_PATH(img_fp16, "render_fwd_cache_filtered");
  FFX_NO_APPEARANCE(img_fp16, "render_fwd_cache_filtered");
  FFX_NO_TANGENT(img_fp16, "render_fwd_cache_filtered");
  FFX_NO_AOV(img_fp16, "render_fwd_cache_filtered");
  FFX_NO_LIGHTS(img_fp16, "render_fwd_cache_filtered");
  return render_fwd_impl(bvh, info, sd, shape_albedo, tex, spp, seed,
                         img_fp16 & (FFX_RENDER_FP16 | FFX_RENDER_SPARSE_ADJOINT | FFX_RENDER_APEX_READY | FFX_RENDER_CACHE_ZEROED | FFX_RENDER_CACHE_KEEP_DROPPED), img, nullptr, s,
                         nullptr, nullptr, nullptr, scratch, cache);
}

int ffx_render_bwd_cached_filtered(const ffx_scene_desc *sd, const float *shape_albedo, const void *cache, int spp, uint32_t seed, const float *gimg, float *gtex,
                                   ffx_stream s) {
  if (!sd || (!shape_albedo && sd->n_mat_h <= 0) || !cache || !gimg || !gtex || spp < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached_filtered: bad argument");
  if (sd->rfilter != FFX_RFILTER_GAUSSIAN) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached_filtered: rfilter must be FFX_RFILTER_GAUSSIAN (the box film: ffx_render_bwd_cached)");
  if (spp > 1024) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached_filtered: more than 1024 samples per pixel");
  if (!sd->proj.enabled) return FFX_OK;
  BwdF p;
  memset(&p, 0, sizeof p);
  p.mats = shape_albedo;
  p.ms = sd->mat_stride ? sd->mat_stride : 3;
  if (p.ms != 3 && p.ms != FFX_MAT_STRIDE) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached_filtered: bad material stride");
  if (!copy_mat_h(sd, p.ms, p)) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached_filtered: n_mat_h must be n_shapes x stride (<= %d)", FFX_MAX_MAT_H);
  p.tw = sd->proj.tex_w; p.th = sd->proj.tex_h; p.tc = sd->proj.tex_channels; p.spp = spp;
  p.W = sd->cam.width; p.H = sd->cam.height;
  if (p.tw < 1 || p.th < 1 || (p.tc != 1 && p.tc != 3) || p.W < 1 || p.H < 1) FFX_FAIL(FFX_ERR_ARG, "render_bwd_cached_filtered: bad scene description");
  for (int i = 0; i < 3; ++i) p.color[i] = sd->proj.color[i];
  const float sdv = sd->rfilter_stddev > 0.f ? sd->rfilter_stddev : 0.5f;
  if (!(sdv <= 0.5f)) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached_filtered: gaussian filter: stddev <= 0.5");
  rf_constants(sdv, p.rf); // (as shade_prepare)
  p.seed_key = seed_key_of(seed);
  p.n_shapes = sd->n_shapes;
  if (p.n_shapes < 1 || p.n_shapes > 255) FFX_FAIL(FFX_ERR_UNSUPPORTED, "render_bwd_cached_filtered: 1 .. 255 shapes");
  const size_t n_pix = (size_t)p.W * p.H;
  p.off_wsum = rfc_off_wsum(n_pix); p.off_recs = rfc_off_recs(n_pix); p.off_facb = rfc_off_facb(n_pix, (size_t)spp, rfc_all(sd));
  const int blocks_x = ffx_cdiv(p.W, K9F_BLOCK), blocks_y = ffx_cdiv(p.H, K9F_BLOCK);
  hipLaunchKernelGGL(k_render_bwd_cached_filtered, dim3(blocks_x * blocks_y * K9F_SUB), dim3(64), 0, (hipStream_t)s, p, (const char *)cache, blocks_x, gimg, gtex);
  FFX_CHECK_LAUNCH("render_bwd_cached_filtered");
  return FFX_OK;
}

} // extern "C"
