// The pixel rectangles of the camera's tile bins as tables: what bins_primary and traverse_bins (ffx_trace.hip) form per pixel from nothing but the
// pixel's column or row, the film's size and the camera grid's tile side — the same for every pixel of a column in every render of a run.  The
// plain-scene instance of k_render_fwd_pk reads them with two scalar 16-byte loads instead of forming them on the vector ALU and carrying them
// back into scalar registers (plain_scene / rect_tables, ffx_trace.hip).  Host code without a HIP dependency: a stand-alone program can include
// it (tests/test_pixel_rect_cpu.py does).
//
// Per column px (per row py likewise, with its_y), in float, operation for operation what the kernel's generic instance does:
//   x0  = (float)px * its_x                      (its: 1 / tile side, a power of two)
//   hx  = 0.5f * its_x - 0.25f * FFX_BIN_PAD     (the half pad of bins_primary's comment: the far side stops short of the next tile)
//   cx  = x0 + hx
//   rx0 = cx - hx,  rx1 = cx + hx                (traverse_bins' box bounds)
//   tx  = (int)x0                                (the tile)
// Single IEEE operations each: compile users of this header with -ffp-contract=off, as the library is.
// An entry is 16 bytes {cx, rx0, rx1, tx}; tx is stored as the INTEGER's bits in the fourth word: the kernel wants it in a scalar register as an
// integer, and gfx950 has no scalar float -> int conversion (a float there would cost the two vector instructions the table is meant to remove).
// The table of a film: W column entries, then H row entries.
#ifndef FFX_RECT_H
#define FFX_RECT_H
#include <cstdint>
#include <cstring>
#include <vector>

#define FFX_RECT_BIN_PAD 0.00390625f // == FFX_BIN_PAD (ffx_common.h; ffx_trace.hip asserts it)
#define FFX_RECT_MAX_SIDE 4096       // the library's cache keeps no table for a film wider or higher than this (such a film renders through the generic instance)

struct FfxRectEntry { float c, r0, r1; int32_t t; };
static_assert(sizeof(FfxRectEntry) == 16, "a rectangle entry is one 16-byte scalar load");

static inline float ffx_rect_half(float its) { return 0.5f * its - 0.25f * FFX_RECT_BIN_PAD; }

static inline FfxRectEntry ffx_rect_entry(int p, float its) {
  const float x0 = (float)p * its;
  const float h = ffx_rect_half(its);
  const float c = x0 + h;
  FfxRectEntry e;
  e.c = c;
  e.r0 = c - h;
  e.r1 = c + h;
  e.t = (int)x0;
  return e;
}

// -> the film's table (W + H entries: columns, then rows) and the two half extents; false (nothing written) for a film or a tile side no table is kept for
static inline bool ffx_rect_fill(int W, int H, float its_x, float its_y, std::vector<FfxRectEntry> &tab, float &hx, float &hy) {
  if (W < 1 || H < 1 || W > FFX_RECT_MAX_SIDE || H > FFX_RECT_MAX_SIDE) return false;
  if (!(its_x > 0.f) || !(its_y > 0.f) || its_x > 1.f || its_y > 1.f) return false;
  tab.resize((size_t)W + (size_t)H);
  for (int px = 0; px < W; ++px) tab[(size_t)px] = ffx_rect_entry(px, its_x);
  for (int py = 0; py < H; ++py) tab[(size_t)W + (size_t)py] = ffx_rect_entry(py, its_y);
  hx = ffx_rect_half(its_x);
  hy = ffx_rect_half(its_y);
  return true;
}
#endif
