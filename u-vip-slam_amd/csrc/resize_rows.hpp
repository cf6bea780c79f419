// Band schedule of k_resize_level_rows (pyramid.hip): which source rows a wavefront's walk down a band of output rows filters, in what order,
// and which it still holds.  Plain C++ shared by the kernel, its launcher and the host emulation (tests/emu/resize_rows_emu.cpp).
//
// A work item is 64 consecutive entries of the launch's flattened (frame, dword column) space times a band of UVO_RESIZE_BAND consecutive
// output rows.  A lane keeps two horizontally filtered source rows in two register sets ("slots").  Output row j of the band wants its upper
// source row in slot j & 1 and its lower one in the other slot: walking down, the lower row of one output row is the upper row of the next in
// about 1 / (scale - 1) cases of scale / (scale - 1), it is then already where the next row wants it, and only the new lower row is filtered --
// the slots swap roles from row to row and nothing is ever moved.  A step of two source rows misses both.  On the reflected pad rows, where
// the sequence runs backwards, the old upper row is the new lower one and hits the same way.
#pragma once
#include <stdint.h>

// Operating point (MI355X, 640 x 512, 257 frames, ring 4, every level forced onto this form; bench.py's k_resize_level_rows time inside the
// running step, two runs each: profiles/r13_resize_rows_ab.txt): 16 rows with 1 / 2 / 3 rows in flight 0.152 / 0.145 / 0.146 ms (frames/s
// 314 000 / 314 200 / 315 500 against the parent's 309 500), 32-row bands 0.158 - 0.160 (half the wavefronts: the small levels are ramp and
// tail); 24 rows with 4 in flight needs more than 64 registers and spills (0.26 ms).
#ifndef UVO_RESIZE_BAND
#define UVO_RESIZE_BAND 16  // output rows per band: 1.2 + 1 / band source rows filtered per output row at scale 1.2
#endif
#ifndef UVO_RESIZE_AHEAD
#define UVO_RESIZE_AHEAD 3  // output rows whose source rows are in flight while a row is computed
#endif

#if defined(__HIPCC__)
#define UVO_RR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UVO_RR_HD inline
#endif

namespace uvo {

constexpr int kResizeRowsPad = 16;  // EDGE_THRESHOLD: ROI origin inside a padded plane (kPad)

// The region of the padded plane a launch writes: dword columns wx0 .. wx0 + nwx - 1, rows row0 .. row_end - 1.  ring = 0: the whole plane;
// ring = 4, 8, 12: the ROI and that many pixels around it (the same region as launch_resize_level's).
struct ResizeRowsRegion {
  int wx0, nwx, row0, row_end, nbands;
};
UVO_RR_HD ResizeRowsRegion resize_rows_region(int dw, int dh, int dpitch, int ring) {
  ResizeRowsRegion r;
  r.wx0 = 0, r.nwx = dpitch / 4, r.row0 = 0, r.row_end = dh + 2 * kResizeRowsPad;
  if (ring > 0 && ring < kResizeRowsPad && (kResizeRowsPad - ring) % 4 == 0) {
    r.wx0 = (kResizeRowsPad - ring) / 4, r.row0 = kResizeRowsPad - ring, r.row_end = dh + kResizeRowsPad + ring;
    r.nwx = (dw + kResizeRowsPad + ring + 3) / 4 - r.wx0;
  }
  r.nbands = (r.row_end - r.row0 + UVO_RESIZE_BAND - 1) / UVO_RESIZE_BAND;
  return r;
}
// band b: rows py0 .. py0 + n - 1 (the last band may be shorter)
UVO_RR_HD void resize_rows_band(const ResizeRowsRegion& r, int b, int* py0, int* n) {
  *py0 = r.row0 + b * UVO_RESIZE_BAND;
  const int left = r.row_end - *py0;
  *n = left < UVO_RESIZE_BAND ? left : UVO_RESIZE_BAND;
}

// The walk's state: tag[p] = source row whose filtered form slot p holds (-1: nothing yet).
struct ResizeRowsState {
  int tag[2];
};
// Output row j of a band (p = j & 1) with source rows (sy0, sy1): the upper row is wanted in slot p, the lower one in slot p ^ 1.  eval0: the
// upper row has to be loaded and filtered because the slot holds another row.  eval1: the same for the lower row -- the kernel does NOT
// read it: it loads and filters the lower row always (pyramid.hip: rows_walk); the host emulation reads it, to count how often that repeats
// a row the lane held (only where the table clamps or turns round, never on the monotone part).
struct ResizeRowsStep {
  int eval0, eval1;
};
UVO_RR_HD ResizeRowsStep resize_rows_step(ResizeRowsState& st, int p, int sy0, int sy1) {
  ResizeRowsStep s;
  s.eval0 = (p ? st.tag[1] : st.tag[0]) != sy0;  // (no indexing by p: the tags stay in registers)
  s.eval1 = (p ? st.tag[0] : st.tag[1]) != sy1;
  st.tag[0] = p ? sy1 : sy0, st.tag[1] = p ? sy0 : sy1;
  return s;
}

// Frames per launch; 0: the level cannot take this form (a frame alone does not fit).  Three bounds:
//   lane -> (frame, dword column) by multiply-high with ceil(2^32 / nwx) is exact while entries * nwx < 2^32;
//   work item -> (column chunk, band) by multiply-high with ceil(2^32 / nbands) is exact while items * nbands < 2^32;
//   a lane addresses its frame by a 32-bit offset from the launch's base: frames * frame_bytes (the larger of the source's and the
//   destination's frame stride; a frame's own bytes lie inside its stride) stays below 2^32.
inline int64_t resize_rows_max_frames(int nwx, int nbands, int64_t frame_bytes) {
  if (frame_bytes <= 0 || nwx <= 0 || nbands <= 0) return 0;
  const int64_t a = 0xffffffffll / ((int64_t)nwx * nwx), b = 0xffffffffll / frame_bytes;
  const int64_t c = (0xffffffffll / ((int64_t)nbands * nbands) - 1) * 64 / nwx;
  int64_t m = a < b ? a : b;
  m = c < m ? c : m;
  m = m < 0 ? 0 : m;
  return m < (1 << 20) ? m : (1 << 20);
}

}  // namespace uvo
