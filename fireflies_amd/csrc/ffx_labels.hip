// ffx_labels.hip — connected components of an integer image with statistics (include/ffx_labels.h): the acceptance
// step of the dataset path, main.py:168-180.  gfx950 only, plain HIP.
//
// Seven launches, fewer when outputs are NULL; no workgroup ever waits for another — phases are launch boundaries:
//   k_cc_tile     a 32 x 32 tile per workgroup: union-find in LDS, then parent[p] = image index of p's tile-local root (-1: background)
//   k_cc_seam     one thread per pixel of a tile's bottom or right edge: unions across the seam (device-scope atomics only)
//   k_cc_flatten  parent[p] = its root; the roots (parent[p] == p) of every 1024 consecutive pixels are counted
//   k_cc_scan     one workgroup: exclusive prefix sums of those counts, n_labels = total + 1
//   k_cc_rank     a root's rank among the roots in linear order is its component's number - 1 (a root IS its component's first raster
//                 pixel); the statistics' accumulators are reset here
//   k_cc_relabel  labels[p] = rank of p's root + 1; area / box / coordinate sums per tile-local component in LDS, one flush of integer
//                 atomics per (tile, component)
//   k_cc_finish   accumulators -> left, top, width, height, area and the two float64 divisions per row; the tail rows
#include "ffx_common.h"
#include "../../include/ffx_labels.h"

#define CC_T 32                   // tile side
#define CC_TILE (CC_T * CC_T)     // pixels of a tile = pixels of a linear chunk of the flatten / rank passes
#define CC_BLOCK 256              // threads; each takes four horizontally adjacent pixels
#define CC_SCAN_BLOCK 1024

struct CcAcc { unsigned long long sx, sy; int area, minx, miny, maxx, maxy, pad; }; // one statistics row in the workspace
static_assert(sizeof(CcAcc) == 40, "FFX_COMPONENTS_WORKSPACE_BYTES counts 40 bytes per row");

// foreground: px != background; a 1-byte pixel is zero-extended, 4- and 8-byte pixels are signed
__device__ __forceinline__ bool cc_fg(const void *img, int es, size_t p, long long bg) {
  const long long v = es == 1 ? (long long)((const uint8_t *)img)[p] : es == 4 ? (long long)((const int32_t *)img)[p] : (long long)((const int64_t *)img)[p];
  return v != bg;
}

// ---- LDS union-find of one tile.  The LDS is not cached: a relaxed load sees every earlier atomicMin of the workgroup.
__device__ __forceinline__ int cc_find_lds(int *P, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void cc_union_lds(int *P, int a, int b) {
  for (;;) { // the argument of cc_union_global, with LDS atomics
    a = cc_find_lds(P, a);
    b = cc_find_lds(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; } // a > b: hang the larger root under the smaller
    const int old = atomicMin(&P[a], b);
    if (old == a) return;
    a = old;
  }
}

// img -> parent[p] (image index of the tile-local root, -1 on the background) and, where slots != nullptr, slots[p] = the root's
// position in its tile (0..1023): the key under which k_cc_relabel sums a tile-local component
__global__ __launch_bounds__(CC_BLOCK) void k_cc_tile(const void *img, int es, int h, int w, long long bg, int conn8, int *parent, int *slots) {
  __shared__ int P[CC_TILE];
  __shared__ unsigned rows[CC_T]; // bit lx of rows[ly]: pixel (lx, ly) of the tile is foreground
  const int t = threadIdx.x, ly = t >> 3, lx0 = (t & 7) * 4;
  const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T, y = y0 + ly;
  if (t < CC_T) rows[t] = 0u;
  __syncthreads();
  unsigned nib = 0u;
  if (y < h)
    for (int j = 0; j < 4; ++j)
      if (x0 + lx0 + j < w && cc_fg(img, es, (size_t)y * w + x0 + lx0 + j, bg)) nib |= 1u << j; // lanes outside the image are background
  if (nib) atomicOr(&rows[ly], nib << lx0);
  __syncthreads();
  const unsigned m = rows[ly], up = ly ? rows[ly - 1] : 0u;
  // every pixel starts under the first pixel of its horizontal run: a forest with parent <= self
  for (int j = 0; j < 4; ++j) {
    const int lx = lx0 + j;
    const unsigned gap = ~m & ((1u << lx) - 1u); // background pixels left of lx
    P[ly * CC_T + lx] = ly * CC_T + (gap ? 32 - __clz(gap) : 0);
  }
  __syncthreads();
  // unions with the row above; a pair already joined through the left neighbour's union is left out
  for (int j = 0; j < 4; ++j) {
    const int lx = lx0 + j, i = ly * CC_T + lx;
    if (!((m >> lx) & 1u) || !ly) continue;
    const bool W = lx && ((m >> (lx - 1)) & 1u), N = (up >> lx) & 1u, NW = lx && ((up >> (lx - 1)) & 1u), NE = lx < CC_T - 1 && ((up >> (lx + 1)) & 1u);
    if (N) {
      if (!(W && NW)) cc_union_lds(P, i, i - CC_T);
    } else if (conn8) {
      if (NW && !W) cc_union_lds(P, i, i - CC_T - 1);
      if (NE) cc_union_lds(P, i, i - CC_T + 1);
    }
  }
  __syncthreads();
  if (y >= h) return;
  for (int j = 0; j < 4; ++j) {
    const int lx = lx0 + j, x = x0 + lx;
    if (x >= w) break;
    const size_t p = (size_t)y * w + x;
    if ((m >> lx) & 1u) {
      const int r = cc_find_lds(P, ly * CC_T + lx);
      parent[p] = (y0 + (r >> 5)) * w + x0 + (r & 31); // the tile's raster order is the image's: the smallest slot is the smallest index
      if (slots) slots[p] = r;
    } else {
      parent[p] = -1;
    }
  }
}

// ---- the seam pass: the only launch in which workgroups touch each other's words of `parent`
__device__ __forceinline__ int cc_find_global(int *P, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // never a plain load: an L1 line is not refreshed by other CUs
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void cc_union_global(int *P, int a, int b) {
  // Every access to P in this launch is a device-scope atomic, and the loop is right for ANY value a load returns that P held at
  // some time of this launch ("stale but once true"):
  //  - P[i] <= i always and a word only decreases (atomicMin), so a once-true P[i] = j < i says "i and j are in one set", which stays
  //    true: sets only merge.  A find therefore ends at a node of the start's set, after strictly falling indices (it terminates); the
  //    node may no longer be a root, which the atomicMin below finds out.
  //  - a == b: both starts reach one node, they are in one set already.
  //  - else atomicMin(&P[a], b) with a > b; its RETURN value, not a load, decides: old == a means a was a root at that instant and hangs
  //    under b now — done.  old < a means a had a parent old already (a and old in one set); whether the min replaced it (b < old) or not,
  //    uniting old with b finishes the job, and old < a: the pair falls strictly with every round, so the loop terminates.
  //  The partition at the end of the launch is the transitive closure of the united pairs whatever the dispatch order; the tree below each
  //  root differs from run to run, the root — the smallest index of the set, since links only point downwards — does not.
  for (;;) {
    a = cc_find_global(P, a);
    b = cc_find_global(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[a], b);
    if (old == a) return;
    a = old;
  }
}

// threads [0, n_hs * w): pixel x of the bottom row of tile row k (y = 32 k + 31, y + 1 < h) against (x - 1 | x | x + 1, y + 1);
// threads behind them: pixel y of the right column of tile column k (x = 32 k + 31, x + 1 < w) against (x + 1, y - 1 | y | y + 1).
// Every 4- / 8-neighbour pair that straddles a seam, a tile corner included, is covered.  Not every pair is united: with t the position along
// the seam, `mine(d)` the seam pixel at t + d on this side and `other(d)` the pixel across from it, a union is left out where the
// neighbouring thread's union implies it — mine(0) and mine(-1) are joined inside their tile when both are foreground and t is not the tile's
// first position, likewise other(0) and other(-1) — so a long run along a seam costs one union per tile edge, not three per pixel (all of
// which would meet at one root's word):
//   other(0) foreground:  unite with it unless mine(-1) and other(-1) are foreground in the same tiles (the thread at t - 1 unites those, or
//                         leaves it to t - 2: the chain ends at the tile's first position at the latest); other(-1) / other(+1) are joined
//                         to other(0) inside their tile unless they lie beyond the tile's corner: only then they are united too
//   other(0) background:  (8-connectivity) unite with other(-1) unless mine(-1) is foreground in this tile — other(-1) is ITS opposite —, and
//                         with other(+1) unless mine(+1) is
__global__ __launch_bounds__(CC_BLOCK) void k_cc_seam(int *parent, int h, int w, int conn8, long long n_h, long long n_all) {
  const long long i = (long long)blockIdx.x * CC_BLOCK + threadIdx.x;
  if (i >= n_all) return;
  const bool below = i < n_h; // the neighbours lie in row y + 1 (else in column x + 1)
  int x, y;
  if (below) { y = (int)(i / w) * CC_T + CC_T - 1; x = (int)(i % w); }
  else { const long long k = i - n_h; x = (int)(k / h) * CC_T + CC_T - 1; y = (int)(k % h); }
  const int t = below ? x : y, len = below ? w : h, c = t & (CC_T - 1);
  const int step = below ? 1 : w, p = y * w + x, q = p + (below ? w : 1); // index step along the seam; this pixel and the one across
  // foreground of the pixel d along the seam from index `at` (the sign of a word never changes: foreground stays >= 0)
  auto fg = [&](int at, int d) { return t + d >= 0 && t + d < len && __hip_atomic_load(&parent[at + d * step], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0; };
  if (!fg(p, 0)) return;
  const bool first = c == 0, last = c == CC_T - 1;
  if (fg(q, 0)) {
    if (first || !(fg(p, -1) && fg(q, -1))) cc_union_global(parent, p, q);
    if (conn8 && first && fg(q, -1)) cc_union_global(parent, p, q - step);
    if (conn8 && last && fg(q, 1)) cc_union_global(parent, p, q + step);
  } else if (conn8) {
    if (fg(q, -1) && (first || !fg(p, -1))) cc_union_global(parent, p, q - step);
    if (fg(q, 1) && (last || !fg(p, 1))) cc_union_global(parent, p, q + step);
  }
}

// ---- parent[p] = root; the roots of chunk b (pixels 1024 b ..) are counted.  Plain loads: the unions ended with the last launch.  Other
// threads compress the words this one walks over, but a word only ever moves from one ancestor to the root, and a root's word is never
// written with anything but itself: every value read leads to the same root.
__global__ __launch_bounds__(CC_BLOCK) void k_cc_flatten(int *parent, long long n, int *counts) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * CC_TILE + threadIdx.x * 4;
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    const long long p = p0 + j;
    if (p >= n) break;
    int r = parent[p];
    if (r < 0) continue;
    if (r == (int)p) { ++c; continue; }
    for (int q = parent[r]; q != r; q = parent[r]) r = q;
    parent[p] = r;
  }
  for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c); // (LDS, four waves)
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt;
}

// inclusive scan over the workgroup's threads (blockDim.x a multiple of 64, at most 1024) -> this thread's inclusive sum
__device__ __forceinline__ int cc_block_scan(int v, int *s_wave /*[16]*/) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_wave[wv] = v;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < wv; ++k) base += s_wave[k];
  __syncthreads();
  return v + base;
}

// counts[b] -> the number of roots in front of chunk b; n_labels = roots + 1.  One workgroup, each thread a run of consecutive chunks.
__global__ __launch_bounds__(CC_SCAN_BLOCK) void k_cc_scan(int *counts, int n_chunks, int *n_labels) {
  __shared__ int s_wave[16];
  const int per = (n_chunks + CC_SCAN_BLOCK - 1) / CC_SCAN_BLOCK, b0 = threadIdx.x * per, b1 = min(b0 + per, n_chunks);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += counts[b];
  const int incl = cc_block_scan(sum, s_wave);
  int run = incl - sum;
  for (int b = b0; b < b1; ++b) {
    const int c = counts[b];
    counts[b] = run;
    run += c;
  }
  if (threadIdx.x == CC_SCAN_BLOCK - 1) n_labels[0] = incl + 1;
}

// ranks[root] = ~(its rank): negative, so that k_cc_relabel tells it from a tile slot (a root's slot is its own position anyway).
// The grid also resets the statistics' accumulators.
__global__ __launch_bounds__(CC_BLOCK) void k_cc_rank(const int *parent, long long n, const int *offsets, int *ranks, CcAcc *acc, int max_labels) {
  __shared__ int s_wave[16];
  const long long p0 = (long long)blockIdx.x * CC_TILE + threadIdx.x * 4;
  bool root[4];
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    root[j] = p0 + j < n && parent[p0 + j] == (int)(p0 + j);
    c += root[j];
  }
  int rank = offsets[blockIdx.x] + cc_block_scan(c, s_wave) - c;
  for (int j = 0; j < 4; ++j)
    if (root[j]) ranks[p0 + j] = ~(rank++);
  if (acc)
    for (long long k = (long long)blockIdx.x * CC_BLOCK + threadIdx.x; k < max_labels; k += (long long)gridDim.x * CC_BLOCK) {
      CcAcc a;
      a.sx = a.sy = 0ull;
      a.area = 0; a.minx = a.miny = 0x7fffffff; a.maxx = a.maxy = -1; a.pad = 0;
      acc[k] = a;
    }
}

// labels and the statistics' sums of one 32 x 32 tile.  Slot 1024 is the tile's background.  Sums within a tile are relative to its
// origin (at most 1024 * 31: 32 bits in LDS); the flush adds origin * area in 64 bits.
template <bool STATS>
__global__ __launch_bounds__(CC_BLOCK) void k_cc_relabel(const int *parent, const int *ranks, int h, int w, int *labels, CcAcc *acc, int max_labels) {
  __shared__ int s_area[STATS ? CC_TILE + 1 : 1], s_sx[STATS ? CC_TILE + 1 : 1], s_sy[STATS ? CC_TILE + 1 : 1], s_lab[STATS ? CC_TILE + 1 : 1];
  __shared__ int s_minx[STATS ? CC_TILE + 1 : 1], s_maxx[STATS ? CC_TILE + 1 : 1], s_miny[STATS ? CC_TILE + 1 : 1], s_maxy[STATS ? CC_TILE + 1 : 1];
  const int t = threadIdx.x, ly = t >> 3, lx0 = (t & 7) * 4;
  const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T, y = y0 + ly;
  if (STATS) {
    for (int i = t; i <= CC_TILE; i += CC_BLOCK) {
      s_area[i] = s_sx[i] = s_sy[i] = 0;
      s_minx[i] = s_miny[i] = CC_T;
      s_maxx[i] = s_maxy[i] = -1;
    }
    __syncthreads();
  }
  // a thread's four pixels share a row; consecutive pixels of one slot are summed in registers and reach the LDS once
  int cur = -1, n = 0, sx = 0, fx = 0, lastx = 0;
  auto flush = [&]() {
    if (!STATS || cur < 0) return;
    atomicAdd(&s_area[cur], n);
    atomicAdd(&s_sx[cur], sx);
    atomicAdd(&s_sy[cur], n * ly);
    atomicMin(&s_minx[cur], fx);
    atomicMax(&s_maxx[cur], lastx);
    atomicMin(&s_miny[cur], ly);
    atomicMax(&s_maxy[cur], ly);
  };
  if (y < h)
    for (int j = 0; j < 4; ++j) {
      const int lx = lx0 + j, x = x0 + lx;
      if (x >= w) break;
      const size_t p = (size_t)y * w + x;
      const int g = parent[p];
      const int lab = g < 0 ? 0 : ~ranks[g] + 1;
      if (labels) labels[p] = lab;
      if (STATS) {
        int slot = CC_TILE;
        if (g >= 0) {
          slot = ranks[p]; // the tile pass's slot of p's tile-local root; a global root's word holds its rank instead: its slot is itself
          if (slot < 0) slot = ly * CC_T + lx;
        }
        if (slot != cur) {
          flush();
          cur = slot; n = 0; sx = 0; fx = lx;
          s_lab[slot] = lab; // (every pixel of the slot stores the same number)
        }
        ++n; sx += lx; lastx = lx;
      }
    }
  if (STATS) {
    flush();
    __syncthreads();
    for (int i = t; i <= CC_TILE; i += CC_BLOCK) {
      const int a = s_area[i];
      if (a <= 0) continue;
      const int lab = s_lab[i]; // (written by the slot's pixels: a > 0)
      if (lab >= max_labels) continue;
      CcAcc *r = acc + lab;
      atomicAdd(&r->area, a);
      atomicMin(&r->minx, x0 + s_minx[i]);
      atomicMin(&r->miny, y0 + s_miny[i]);
      atomicMax(&r->maxx, x0 + s_maxx[i]);
      atomicMax(&r->maxy, y0 + s_maxy[i]);
      atomicAdd(&r->sx, (unsigned long long)s_sx[i] + (unsigned long long)x0 * (unsigned long long)a);
      atomicAdd(&r->sy, (unsigned long long)s_sy[i] + (unsigned long long)y0 * (unsigned long long)a);
    }
  }
}

// the rows cv2 returns; rows without pixels and the rows behind n_labels: zeros and NaN
__global__ __launch_bounds__(CC_BLOCK) void k_cc_finish(const CcAcc *acc, const int *n_labels, int max_labels, int *stats, double *centroids) {
  const int k = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (k >= max_labels) return;
  const CcAcc a = acc[k];
  const bool on = k < n_labels[0] && a.area > 0;
  int *s = stats + 5 * (size_t)k;
  s[0] = on ? a.minx : 0;
  s[1] = on ? a.miny : 0;
  s[2] = on ? a.maxx - a.minx + 1 : 0;
  s[3] = on ? a.maxy - a.miny + 1 : 0;
  s[4] = on ? a.area : 0;
  if (centroids) {
    const double d = on ? (double)a.area : 0.0; // sums below 2^45: exact in float64; 0.0 / 0.0 = NaN where the row is empty
    centroids[2 * (size_t)k] = (on ? (double)a.sx : 0.0) / d;
    centroids[2 * (size_t)k + 1] = (on ? (double)a.sy : 0.0) / d;
  }
}

extern "C" int ffx_connected_components(const void *img, int elem_size, int h, int w, int64_t background, int connectivity, int32_t *labels, int32_t *n_labels,
                                        int32_t *stats, double *centroids, int max_labels, void *workspace, ffx_stream stream) {
  if (!img) FFX_FAIL(FFX_ERR_ARG, "connected_components: img is NULL");
  if (!n_labels) FFX_FAIL(FFX_ERR_ARG, "connected_components: n_labels is NULL");
  if (!workspace) FFX_FAIL(FFX_ERR_ARG, "connected_components: workspace is NULL");
  if (((uintptr_t)workspace & 7) != 0) FFX_FAIL(FFX_ERR_ARG, "connected_components: workspace must be 8-byte aligned"); // (the 64-bit sums of CcAcc)
  if (elem_size != 1 && elem_size != 4 && elem_size != 8) FFX_FAIL(FFX_ERR_ARG, "connected_components: elem_size %d (1, 4 or 8)", elem_size);
  if (h < 1) FFX_FAIL(FFX_ERR_ARG, "connected_components: h %d outside 1..32768", h);
  if (w < 1) FFX_FAIL(FFX_ERR_ARG, "connected_components: w %d outside 1..32768", w);
  // (the product first: 2^30 + 1 has no two factors within the sides' limit)
  if ((long long)h * w > (1ll << 30)) FFX_FAIL(FFX_ERR_ARG, "connected_components: h * w = %lld exceeds 2^30", (long long)h * w);
  if (h > 32768) FFX_FAIL(FFX_ERR_ARG, "connected_components: h %d outside 1..32768", h);
  if (w > 32768) FFX_FAIL(FFX_ERR_ARG, "connected_components: w %d outside 1..32768", w);
  if (connectivity != 4 && connectivity != 8) FFX_FAIL(FFX_ERR_ARG, "connected_components: connectivity %d (4 or 8)", connectivity);
  if (centroids && !stats) FFX_FAIL(FFX_ERR_ARG, "connected_components: centroids without stats");
  if (stats && max_labels < 1) FFX_FAIL(FFX_ERR_ARG, "connected_components: max_labels %d with stats (at least 1)", max_labels);
  const hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)h * w;
  const int n_chunks = (int)((n + CC_TILE - 1) / CC_TILE), conn8 = connectivity == 8;
  // the workspace: parents [n], slots / ranks [n], counts [n_chunks] padded to 16 bytes, statistics rows [max_labels]
  int *parent = (int *)workspace, *ranks = parent + n, *counts = ranks + n;
  CcAcc *acc = stats ? (CcAcc *)((char *)workspace + 8 * (size_t)n + 16 * (size_t)((n + 4095) / 4096)) : nullptr;
  const dim3 tiles(ffx_cdiv(w, CC_T), ffx_cdiv(h, CC_T));
  hipLaunchKernelGGL(k_cc_tile, tiles, dim3(CC_BLOCK), 0, s, img, elem_size, h, w, (long long)background, conn8, parent, stats ? ranks : nullptr);
  FFX_CHECK_LAUNCH("cc_tile");
  const long long n_h = (long long)((h - 1) / CC_T) * w, n_all = n_h + (long long)((w - 1) / CC_T) * h;
  if (n_all > 0) {
    hipLaunchKernelGGL(k_cc_seam, dim3((unsigned)((n_all + CC_BLOCK - 1) / CC_BLOCK)), dim3(CC_BLOCK), 0, s, parent, h, w, conn8, n_h, n_all);
    FFX_CHECK_LAUNCH("cc_seam");
  }
  hipLaunchKernelGGL(k_cc_flatten, dim3(n_chunks), dim3(CC_BLOCK), 0, s, parent, n, counts);
  FFX_CHECK_LAUNCH("cc_flatten");
  hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(CC_SCAN_BLOCK), 0, s, counts, n_chunks, n_labels);
  FFX_CHECK_LAUNCH("cc_scan");
  if (!labels && !stats) return FFX_OK;
  hipLaunchKernelGGL(k_cc_rank, dim3(n_chunks), dim3(CC_BLOCK), 0, s, parent, n, counts, ranks, acc, max_labels);
  FFX_CHECK_LAUNCH("cc_rank");
  if (stats) hipLaunchKernelGGL(k_cc_relabel<true>, tiles, dim3(CC_BLOCK), 0, s, parent, ranks, h, w, labels, acc, max_labels);
  else hipLaunchKernelGGL(k_cc_relabel<false>, tiles, dim3(CC_BLOCK), 0, s, parent, ranks, h, w, labels, acc, max_labels);
  FFX_CHECK_LAUNCH("cc_relabel");
  if (stats) {
    hipLaunchKernelGGL(k_cc_finish, dim3(ffx_cdiv(max_labels, CC_BLOCK)), dim3(CC_BLOCK), 0, s, acc, n_labels, max_labels, stats, centroids);
    FFX_CHECK_LAUNCH("cc_finish");
  }
  return FFX_OK;
}
