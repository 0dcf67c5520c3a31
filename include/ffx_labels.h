/* ffx_labels.h — the entry points of libffx_hip.so that have no restatement in the CPU oracle.
 *
 * include/ffx.h is the header BOTH shared libraries implement, symbol for symbol.  What is declared here is implemented by
 * fireflies_amd/csrc/libffx_hip.so alone and is held to numpy / scipy references by its own tests (tests/ref_components.py,
 * tests/ref_perlin.py, tests/ref_sparse_depth.py).  The
 * conventions are ffx.h's: FFX_OK or a negative code with a message in ffx_last_error(), the caller owns every buffer, every call is
 * asynchronous on `stream`, arrays are dense and row-major.  FFX_ABI_VERSION is ffx.h's; additions here do not change it.
 */
#ifndef FFX_LABELS_H
#define FFX_LABELS_H

#include "ffx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Dataset path, the acceptance step: connected components of an integer image with statistics.
 * Replaces cv2.connectedComponentsWithStats(seg_test.astype(np.uint8)) at main.py:168-180 (and :217-229), where the reference drops
 * a sample whose mask "everything but the glottis" falls into more than two pieces (n_labels > 3).  DESIGN.md 4.11 is the definition;
 * in short:
 *   a pixel is foreground when img[y][x] != background (a 1-byte pixel is zero-extended, 4- and 8-byte pixels are signed);
 *   a component is a maximal set of foreground pixels joined by 4- or 8-neighbour steps; components are numbered 1..C in raster
 *   order of their first pixel (scipy.ndimage.label's numbering; cv2's is not promised);
 *   n_labels[0]   = C + 1 (the background is label 0 whether or not a pixel has it);
 *   labels[y][x]  = 0 on the background, else the component's number — complete whatever max_labels is;
 *   stats[k]      = left, top, width, height, area of label k for k < min(n_labels, max_labels) (row 0: the background pixels); a row
 *                   of area 0 and every later row: zeros;
 *   centroids[k]  = (sum x / area, sum y / area): exact 64-bit integer sums, each converted to float64, one IEEE division; NaN where
 *                   stats[k] is zeros.
 * labels, stats and centroids may each be NULL (the launches that only serve them are skipped); centroids without stats is refused.
 * Everything is written, nothing accumulated; integer atomics only: two calls give the same bytes.  No host synchronisation and no
 * host read of device memory: the call can be captured into a graph.
 * Limits: 1 <= h, w <= 32768, h * w <= 2^30, elem_size 1 / 4 / 8, connectivity 4 / 8, max_labels >= 1 with stats; workspace 8-byte
 * aligned.  Outside them, or with a NULL img / n_labels / workspace: FFX_ERR_ARG before any launch, the parameter named in the message.
 * ---------------------------------------------------------------------------------------- */
/* bytes of `workspace`: two int32 per pixel (the union-find's parents; tile-local slots, then ranks), one int32 per 1024 pixels
 * (root counts, then their prefix sums) padded to 16 bytes, and 40 bytes per statistics row */
#define FFX_COMPONENTS_WORKSPACE_BYTES(h, w, max_labels) \
  ((size_t)8 * (size_t)(h) * (size_t)(w) + (size_t)16 * (((size_t)(h) * (size_t)(w) + 4095) / 4096) + (size_t)40 * (size_t)((max_labels) > 0 ? (max_labels) : 0))

int ffx_connected_components(const void *img /*[dev][h,w] integers of elem_size bytes*/, int elem_size, int h, int w, int64_t background,
                             int connectivity, int32_t *labels /*[dev][h,w] or NULL*/, int32_t *n_labels /*[dev][1]*/,
                             int32_t *stats /*[dev][max_labels,5] or NULL*/, double *centroids /*[dev][max_labels,2] or NULL*/,
                             int max_labels, void *workspace /*[dev] FFX_COMPONENTS_WORKSPACE_BYTES(h, w, max_labels)*/, ffx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Dataset path, the first step: a multi-octave Perlin base-colour texture.
 * Replaces the per-texel arithmetic of lerp_sampler.sample() at main.py:148-153 (fireflies/sampling/noise_texture_lerp.py); the lattice
 * angles stay host draws.  DESIGN.md 4.12 is the definition; in short, per octave o = 0..octaves-1 with R0 = r0 << o, R1 = r1 << o,
 * c0 = h / R0, c1 = w / R1 (integer divisions):
 *   angles: [R0+1][R1+1] binary32 lattice angles (2 pi torch.rand), the octaves packed one after the other;
 *   pos:    fy[h] then fx[w], the binary32 positions of every row / column inside its lattice cell AS THE HOST COMPUTED THEM
 *           ((torch.arange(0, R0, R0 / h) % 1)[:h]; they are inputs, not recomputed), the octaves packed one after the other;
 *   texel (i, j): cell cy = min(i / c0, R0-1), cx = min(j / c1, R1-1); py = fy[i], px = fx[j];
 *           n(dy,dx) = (py-dy) cos(ang[cy+dy][cx+dx]) + (px-dx) sin(ang[cy+dy][cx+dx]); fade(t) = 6t^5 - 15t^4 + 10t^3;
 *           octave = sqrt(2) lerp(lerp(n00, n10, fade(py)), lerp(n01, n11, fade(py)), fade(px));
 *   noise = sum_o float(persistence^o) octave_o;  t = (noise - min) / (max - min) over the whole plane (max == min is not special: the
 *   same IEEE division, a NaN texture);  out[c] = lerp(color_a[c], color_b[c], t).
 * layout 0 writes [3][h][w], layout 1 writes [h][w][3] (the renderer's).  Three launches (tile extremes, their reduction, the write
 * pass, which recomputes the noise with the same device function: the extremes come out as exactly color_a and color_b); no atomics,
 * no workgroup waits for another: two calls give the same bits.  No host synchronisation and no host read of device memory.
 * Limits: octaves 1..8, 1 <= h, w <= 32768, r0, r1 >= 1, every octave's cell at least one texel (c0, c1 >= 1), layout 0 / 1, workspace
 * 8-byte aligned.  Outside them, or with a NULL pointer: FFX_ERR_ARG before any launch, the parameter named in the message.
 * ---------------------------------------------------------------------------------------- */
/* bytes of `workspace`: the extremes of the plane (two floats, padded to 16 bytes) and two floats per 64 x 16 tile */
#define FFX_PERLIN_WORKSPACE_BYTES(h, w) ((size_t)16 + (size_t)8 * ((((size_t)(h) + 15) / 16) * (((size_t)(w) + 63) / 64)))

int ffx_perlin_texture(const float *angles /*[dev] packed per octave*/, const float *pos /*[dev] packed per octave: fy[h], fx[w]*/, int octaves, int r0,
                       int r1, double persistence, int h, int w, const float *color_a /*[dev][3]*/, const float *color_b /*[dev][3]*/, int layout,
                       float *out /*[dev][3,h,w] or [h,w,3]*/, void *workspace /*[dev] FFX_PERLIN_WORKSPACE_BYTES(h, w)*/, ffx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Sparse-depth route: the laser's hits as a differentiable sparse depth image.
 * Replaces the autograd graphs of rasterize_depth (fireflies/graphics/rasterization.py:66-104), of softor(rasterize_depth) in
 * subsampled_point_raster (:538-549) and of dr.wrap_ad around ray_intersect in cast_laser (fireflies/graphics/depth.py:16).
 * With p = (pts[n][0] size0, pts[n][1] size1) and the texel x = (j, i):
 *   e_n(x)     = exp(-(|x - p|^2 / sigma)^2), exactly 0 beyond the footprint ffx_splat_fwd cuts at;
 *   m_n        = e_n(x*), x* = rintf(p) clamped into the texture (ffx_splat_depth_fwd's statement of the layer maximum);
 *   layer_n(x) = (e_n(x) / m_n) depth[n]: the float ffx_splat_depth_fwd writes.
 * ffx_splat_depth_bwd         adjoint of ffx_splat_depth_fwd:  gdepth[n] = sum_x gout[n](x) e_n / m_n,
 *                             gpts[n] = (depth[n] / m_n) sum_x gout[n](x) (de_n/dp - (e_n / m_n) dm_n/dp), chained through the scaling by the
 *                             size; dm_n/dp at the FIXED x*.  At a rintf tie the layer is not differentiable: the value is that of the x* rintf picks.
 * ffx_splat_depth_softor_fwd  out = 1 - prod_n (1 - layer_n), the product in ascending point order in binary32: bit for bit what the host
 *                             forms from ffx_splat_depth_fwd's layers; the [n,size1,size0] stack never exists.  n = 0: a zero plane.
 * ffx_splat_depth_softor_bwd  its adjoint: the sums above with gout(x) prod_{k != n} (1 - layer_k(x)) for gout[n](x); the product is formed from
 *                             the other points' factors, never by dividing by the point's own.
 * A point whose m_n underflows to 0 (far outside the texture) has a NaN layer: the fused forward gives the NaN plane the layers give; the
 * adjoints on such input are unspecified.  depth is taken finite.
 * Per-texel terms binary32, their sums binary64; no atomics: two calls give the same bits.  Everything is written, nothing accumulated
 * (n = 0: the adjoints have nothing to write).  No host synchronisation.
 * Refused with FFX_ERR_ARG before any launch, the parameter named: n < 0, size0 / size1 < 1, sigma <= 0 (or NaN), a NULL pointer that
 * would be read or written.
 * ---------------------------------------------------------------------------------------- */
int ffx_splat_depth_bwd(const float *pts /*[dev][n,2]*/, const float *depth /*[dev][n]*/, int n, float sigma, int size0, int size1,
                        const float *gout /*[dev][n,size1,size0]*/, float *gpts /*[dev][n,2]*/, float *gdepth /*[dev][n]*/, ffx_stream stream);
int ffx_splat_depth_softor_fwd(const float *pts /*[dev][n,2]*/, const float *depth /*[dev][n]*/, int n, float sigma, int size0, int size1,
                               float *out /*[dev][size1,size0]*/, ffx_stream stream);
int ffx_splat_depth_softor_bwd(const float *pts /*[dev][n,2]*/, const float *depth /*[dev][n]*/, int n, float sigma, int size0, int size1,
                               const float *gout /*[dev][size1,size0]*/, float *gpts /*[dev][n,2]*/, float *gdepth /*[dev][n]*/, ffx_stream stream);

/* Adjoint of ffx_trace_rays's t with respect to the rays.  A hit stays on the plane of its triangle (current world vertices v0, v1, v2,
 * N = (v1 - v0) x (v2 - v0)):  t = N . (v0 - o) / (N . d) in units of the given d, so
 *   gorig[r] = -gt[r] N / (N . d),   gdir[r] = -gt[r] t[r] N / (N . d);   a miss (prim[r] < 0): zeros.
 * t and prim are the forward's outputs for the same rays on the same pose of the blob.  No term for a ray that crosses an edge or a
 * silhouette (Mitsuba's interior derivative has none), no gradient to the vertices.
 * Refused with FFX_ERR_ARG before any launch, the parameter named: n < 0, a NULL pointer, a bvh info ffx_trace_rays refuses. */
int ffx_trace_rays_bwd(const void *bvh /*[dev]*/, const ffx_bvh_info *info /*[host]*/, const float *origins /*[dev][n,3]*/,
                       const float *dirs /*[dev][n,3]*/, int n, const float *t /*[dev][n]*/, const int32_t *prim /*[dev][n]*/,
                       const float *gt /*[dev][n]*/, float *gorig /*[dev][n,3]*/, float *gdir /*[dev][n,3]*/, ffx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
