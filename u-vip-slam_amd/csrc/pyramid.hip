// Pyramid build: level-0 border pad and the per-level bilinear down-scale with reflected pad.
// Replaces ORBextractor::ComputePyramid (src/ORBextractor.cc:963-1004): cv::copyMakeBorder(REFLECT_101) at
// level 0 (:996) and cv::resize(INTER_LINEAR) + copyMakeBorder(REFLECT_101|ISOLATED) at levels >= 1 (:982,:988).
//
// HBM-bound streaming kernels: every thread produces 4 consecutive bytes of one padded output row (one
// aligned dword store, rows are 64-B pitched).  Pad pixels are produced by evaluating the level at the
// reflected coordinate, so each level is written exactly once and no second border pass exists.
#include "common.hpp"
#include <algorithm>
#include <cstring>
#include <mutex>

namespace uvo {

__device__ __forceinline__ int reflect101(int p, int len) {
  // BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba ; pad (16) is always smaller than len here
  p = p < 0 ? -p : p;
  p = p >= len ? 2 * (len - 1) - p : p;
  return p;
}

// thread = 16 output bytes (one dwordx4 store).  Threads whose 16 columns lie inside the image copy one aligned
// dwordx4 (when the caller's rows are 16-B aligned, `vec_ok`); border / unaligned threads gather byte by byte with
// the reflected index.
__global__ __launch_bounds__(256) void k_pad_level0(const uint8_t* __restrict__ img, int w, int h, int64_t stride, int64_t frame_stride,
                                                    uint8_t* __restrict__ pyr, int64_t pyr_block, int64_t plane_off, int pitch, int ph,
                                                    int vec_ok) {
  const int qx = blockIdx.x * 64 + (threadIdx.x & 63);  // 16-byte group in the padded row
  const int py = blockIdx.y * 4 + wave_in_block();
  const int f = blockIdx.z;
  if (qx * 16 >= pitch || py >= ph) return;
  const int y = reflect101(py - kPad, h);
  const uint8_t* src = img + f * frame_stride + (int64_t)y * stride;
  const int x0 = qx * 16 - kPad;  // image column of byte 0
  uint4 v;
  // 16 columns that lie wholly in the left or right pad are a reversed run of 16 image columns (REFLECT_101): four
  // unaligned dword loads and a byte swap each, instead of sixteen reflected byte gathers that stall the whole wavefront
  const int r0 = x0 + 16 <= 0 ? -(x0 + 15) : 2 * (w - 1) - x0 - 15;  // first image column of that run
  if (vec_ok && x0 >= 0 && x0 + 16 <= w) {
    v = *reinterpret_cast<const uint4*>(src + x0);
  } else if ((x0 + 16 <= 0 || x0 >= w) && r0 >= 0 && r0 + 16 <= w) {
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t t;
      __builtin_memcpy(&t, src + r0 + 4 * j, 4);
      d[3 - j] = __builtin_bswap32(t);
    }
    v = make_uint4(d[0], d[1], d[2], d[3]);
  } else {
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int x = reflect101(x0 + j * 4 + i, w);
        x = x < 0 ? 0 : (x >= w ? w - 1 : x);  // columns past pw (row pitch slack) stay in range
        t |= (uint32_t)src[x] << (8 * i);
      }
      d[j] = t;
    }
    v = make_uint4(d[0], d[1], d[2], d[3]);
  }
  uint8_t* dst = pyr + f * pyr_block + plane_off + (int64_t)py * pitch;
  *reinterpret_cast<uint4*>(dst + qx * 16) = v;
}

// cv::resize INTER_LINEAR, 8-bit generic path: horizontal pass in 11-bit fixed point (INTER_RESIZE_COEF_SCALE
// = 2048) into int, vertical pass ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2.  The coefficient tables are built
// on the host exactly as resizeGeneric_ builds them (extractor_geom.cpp: build_resize_tables) and are indexed by *padded* output coordinates,
// i.e. the REFLECT_101 border is already folded into them: entry px of the column table holds (sx, a0, a1) of the
// level column reflect(px-16) with the weights scaled by 16, entry py of the row table (sy0, sy1, b0, b1).
// One thread = 4 output bytes x RZ_ROWS rows.  Each of the two source rows is fetched as three aligned dwords (the four tap
// pairs of a dword lie inside 12 bytes for scale factors up to ~1.33; checked per level when the tables are built); one
// v_perm_b32 with a per-thread selector gathers the four left taps, a second one on the window shifted by a byte the four
// right taps.  Levels that do not fit the window gather bytes instead.
// The column weights are stored scaled by 16 (a0 << 4, a1 << 4), so that a row sum comes out as r << 4 and `(r >> 4) << 8`
// -- the operand v_mul_hi_u32_u24 needs to give (b * (r >> 4)) >> 16 in one instruction -- is a single AND.
__device__ __forceinline__ uint32_t mulhi24(uint32_t a, uint32_t b) {  // v_mul_hi_u32_u24: bits [47:32] of the 48-bit product
  return (uint32_t)(((uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu)) >> 32);
}
// left / right tap bytes (bits [8i, 8i+8) of L, R) -> ((left*a0 + right*a1) >> 4) << 8
template <int I>
__device__ __forceinline__ uint32_t hrow(uint32_t L, uint32_t R, uint32_t a0s, uint32_t a1s) {
  const uint32_t r16 = __umul24((L >> (8 * I)) & 0xffu, a0s) + __umul24((R >> (8 * I)) & 0xffu, a1s);
  return r16 & 0xffffff00u;
}
__device__ __forceinline__ uint32_t vrow(uint32_t q0, uint32_t q1, uint32_t b0s, uint32_t b1s) {
  return ((mulhi24(b0s, q0) + mulhi24(b1s, q1) + 2u) >> 2) & 0xffu;  // ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2
}

constexpr int RZ_ROWS = 4;  // output rows per thread: one column-table fetch, RZ_ROWS x 2 independent row fetches in flight

#ifndef UVO_OCC_RESIZE
#define UVO_OCC_RESIZE 6  // six workgroups per CU (80 VGPRs): 0.208 -> 0.197 ms per step; eight (64 VGPRs) spill: 0.263 ms
#endif
__global__ __launch_bounds__(256, UVO_OCC_RESIZE) void k_resize_level(uint8_t* __restrict__ pyr, int64_t pyr_block, int64_t src_off, int src_pitch, int sw,
                                                      int64_t dst_off, int dst_pitch, int dst_ph, int dw, int fast_ok,
                                                      const ResizeCol* __restrict__ ctab, const ResizeRow* __restrict__ rtab,
                                                      uint32_t nwx_magic, Level0View l0, int sh, uint32_t per_frame, uint32_t per_frame_magic, uint32_t per_xcd,
                                                      int batch, uint32_t nwx, int wx0, int rg0, int row_end) {
  // flat index -> (row group, dword column): rows are a few dozen to 150 dwords long, so a (64 x rows) tiling would leave up to
  // a third of the lanes idle on some levels.  gid / nwx by multiply-high with ceil(2^32 / nwx) (exact for gid < 2^20).
  // (an XCD walks whole frames: neighbouring workgroups read the same source rows -- dealt round-robin, every XCD's L2 fetched its own
  // copy of them: 1.39 x the algorithmic bytes per launch)
  // workgroup b runs on XCD b & 7: it takes item (b & 7) * per_xcd + (b >> 3) of the frame-major list of (frame, workgroup of the frame)
  const uint32_t vb = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if (vb >= per_frame * (uint32_t)batch) return;
  const int f = (int)__umulhi(vb, per_frame_magic);  // vb / per_frame (exact: vb * per_frame < 2^32)
  const uint32_t gid = (vb - (uint32_t)f * per_frame) * 256u + threadIdx.x;
  // the launch covers dword columns wx0 .. wx0 + nwx - 1 and rows rg0 * 4 .. row_end - 1 of the padded plane: all of it, or the ROI and the
  // four pixels around it that anything ever reads (launch_resize_level)
  const uint32_t rgl = __umulhi(gid, nwx_magic);
  const int wx = (int)(gid - rgl * nwx) + wx0;
  const uint32_t rg = rgl + (uint32_t)rg0;
  const int py0 = (int)rg * RZ_ROWS;
  if (py0 >= row_end) return;
  dst_ph = row_end;
  // ROI origin of the source level; level 1 may read the caller's image in place (l0.vbase: the resize only looks at the ROI)
  const bool ip = l0.vbase != nullptr;
  if (ip) src_pitch = l0.pitch;
  const uint8_t* S = ip ? l0.vbase + f * l0.frame_stride + (int64_t)kPad * src_pitch + kPad : pyr + f * pyr_block + src_off + (int64_t)kPad * src_pitch + kPad;
  // The 12-byte tap window of the last columns reaches up to 8 bytes past the ROI's last pixel (taps of weight zero).  Inside a padded
  // plane those bytes are the pad; in place they are the next row, and behind the last row of the last frame nothing the caller owns: the
  // window of that row's last lanes is pulled back into the frame (the bytes it then misses carry no weight: see `edge` below).
  const int64_t s_end = ip ? (int64_t)(sh - 1) * src_pitch + sw : INT64_MAX;
  const uint4 c01 = reinterpret_cast<const uint4*>(ctab)[wx * 2];      // columns 4wx, 4wx+1
  const uint4 c23 = reinterpret_cast<const uint4*>(ctab)[wx * 2 + 1];  // columns 4wx+2, 4wx+3
  const uint32_t cw[8] = {c01.x, c01.y, c01.z, c01.w, c23.x, c23.y, c23.z, c23.w};
  uint32_t sx[4], a0[4], a1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sx[i] = cw[2 * i] & 0xffffu;
    a0[i] = cw[2 * i] >> 16;
    a1[i] = cw[2 * i + 1] & 0xffffu;
  }
  // window base and tap selector come ready-made from the table (pad fields of the four column entries); they cover the reflected
  // pad columns too (taps in decreasing order), so every thread of a level takes the same path
  const bool interior = fast_ok != 0;
  const uint32_t base = cw[1] >> 16;
  const uint32_t sel = (cw[3] >> 16) | (cw[5] & 0xffff0000u);
  // the row group's four table entries in two 16-byte loads (the table is padded to whole groups), then all eight source rows at once:
  // nothing here waits for anything but the two table fetches
  static_assert(RZ_ROWS == 4 && sizeof(ResizeRow) == 8, "the row group is read as 2 x uint4");
  const uint4 t01 = reinterpret_cast<const uint4*>(rtab)[rg * 2], t23 = reinterpret_cast<const uint4*>(rtab)[rg * 2 + 1];
  const uint32_t tw[8] = {t01.x, t01.y, t01.z, t01.w, t23.x, t23.y, t23.z, t23.w};
  ResizeRow rr[RZ_ROWS];
  uint32_t u[RZ_ROWS][3], w[RZ_ROWS][3];
#pragma unroll
  for (int j = 0; j < RZ_ROWS; ++j) {
    rr[j].sy0 = (int16_t)(tw[2 * j] & 0xffffu), rr[j].sy1 = (int16_t)(tw[2 * j] >> 16);
    rr[j].b0 = (int16_t)(tw[2 * j + 1] & 0xffffu), rr[j].b1 = (int16_t)(tw[2 * j + 1] >> 16);
  }
  // (in place, only a row group that reaches the frame's last source row has to look at the frame's end)
  const bool guard = ip && max(max((int)rr[0].sy1, (int)rr[1].sy1), max((int)rr[2].sy1, (int)rr[3].sy1)) >= sh - 1;
  if (interior && !guard) {
#pragma unroll
    for (int j = 0; j < RZ_ROWS; ++j) {
      const uint32_t* p0 = reinterpret_cast<const uint32_t*>(S + (int64_t)rr[j].sy0 * src_pitch + base);
      const uint32_t* p1 = reinterpret_cast<const uint32_t*>(S + (int64_t)rr[j].sy1 * src_pitch + base);
      u[j][0] = p0[0], u[j][1] = p0[1], u[j][2] = p0[2];
      w[j][0] = p1[0], w[j][1] = p1[1], w[j][2] = p1[2];
    }
  } else if (interior) {
#pragma unroll
    for (int j = 0; j < RZ_ROWS; ++j) {
      const int64_t o0 = (int64_t)rr[j].sy0 * src_pitch + base, o1 = (int64_t)rr[j].sy1 * src_pitch + base;
      const uint32_t* p0 = reinterpret_cast<const uint32_t*>(S + o0);
      const uint32_t* p1 = reinterpret_cast<const uint32_t*>(S + o1);
      // (a window dword behind the frame's last byte is not loaded: it holds no tap of non-zero weight; rows and the frame end are
      // dword-aligned in this mode)
      u[j][0] = p0[0], u[j][1] = o0 + 4 < s_end ? p0[1] : 0u, u[j][2] = o0 + 8 < s_end ? p0[2] : 0u;
      w[j][0] = p1[0], w[j][1] = o1 + 4 < s_end ? p1[1] : 0u, w[j][2] = o1 + 8 < s_end ? p1[2] : 0u;
    }
  }
  uint32_t vout[RZ_ROWS];
#pragma unroll
  for (int j = 0; j < RZ_ROWS; ++j) {
    uint32_t L0, R0, L1, R1;  // left / right taps of the four columns in the two source rows
    if (interior) {
      L0 = __builtin_amdgcn_perm(u[j][1], u[j][0], sel);
      R0 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(u[j][2], u[j][1], 1), __builtin_amdgcn_alignbyte(u[j][1], u[j][0], 1), sel);
      L1 = __builtin_amdgcn_perm(w[j][1], w[j][0], sel);
      R1 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w[j][2], w[j][1], 1), __builtin_amdgcn_alignbyte(w[j][1], w[j][0], 1), sel);
    } else {
      const uint8_t* S0 = S + (int64_t)rr[j].sy0 * src_pitch;
      const uint8_t* S1 = S + (int64_t)rr[j].sy1 * src_pitch;
      L0 = R0 = L1 = R1 = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t sx1 = sx[i] + 1 < (uint32_t)sw ? sx[i] + 1 : (uint32_t)sw - 1;
        L0 |= (uint32_t)S0[sx[i]] << (8 * i), R0 |= (uint32_t)S0[sx1] << (8 * i);
        L1 |= (uint32_t)S1[sx[i]] << (8 * i), R1 |= (uint32_t)S1[sx1] << (8 * i);
      }
    }
    const uint32_t b0s = (uint32_t)rr[j].b0 << 8, b1s = (uint32_t)rr[j].b1 << 8;
    uint32_t v = vrow(hrow<0>(L0, R0, a0[0], a1[0]), hrow<0>(L1, R1, a0[0], a1[0]), b0s, b1s);
    v |= vrow(hrow<1>(L0, R0, a0[1], a1[1]), hrow<1>(L1, R1, a0[1], a1[1]), b0s, b1s) << 8;
    v |= vrow(hrow<2>(L0, R0, a0[2], a1[2]), hrow<2>(L1, R1, a0[2], a1[2]), b0s, b1s) << 16;
    v |= vrow(hrow<3>(L0, R0, a0[3], a1[3]), hrow<3>(L1, R1, a0[3], a1[3]), b0s, b1s) << 24;
    vout[j] = v;
  }
  // all four rows of a group exist except in the plane's last group: one test per thread instead of one per row
  uint8_t* dst = pyr + f * pyr_block + dst_off + (int64_t)py0 * dst_pitch + wx * 4;
  if (py0 + RZ_ROWS <= dst_ph) {
#pragma unroll
    for (int j = 0; j < RZ_ROWS; ++j) *reinterpret_cast<uint32_t*>(dst + (uint32_t)(j * dst_pitch)) = vout[j];
  } else {
#pragma unroll
    for (int j = 0; j < RZ_ROWS; ++j)
      if (py0 + j < dst_ph) *reinterpret_cast<uint32_t*>(dst + (uint32_t)(j * dst_pitch)) = vout[j];
  }
}

void launch_pad_level0(hipStream_t s, const uint8_t* d_img, int w, int h, int64_t stride, int64_t frame_stride, uint8_t* d_pyr,
                       int64_t pyr_block, const LevelGeom& g0, int batch) {
  dim3 block(256);
  dim3 grid((g0.pitch / 16 + 63) / 64, (g0.ph + 3) / 4, batch);
  const int vec_ok = ((uintptr_t)d_img % 16 == 0 && stride % 16 == 0 && frame_stride % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_pad_level0, grid, block, 0, s, d_img, w, h, stride, frame_stride, d_pyr, pyr_block, g0.plane_off, g0.pitch, g0.ph,
                     vec_ok);
}

// ring = 0: the whole padded plane, as cv::copyMakeBorder of src/ORBextractor.cc:988 leaves it.  ring = 4 (the extractor's hot path): the ROI and
// the four pixels around it -- no stage reads further out (FAST and the orientation patch stay inside the ROI, the blur reaches 3 pixels and
// copies 4 into the blurred plane's ring, the next level's resize reads the ROI): a sixth fewer pixels to interpolate and to write.
void launch_resize_level(hipStream_t s, uint8_t* d_pyr, int64_t pyr_block, const LevelGeom& src, const LevelGeom& dst, const ResizeCol* d_ctab,
                         const ResizeRow* d_rtab, int fast_ok, int batch, Level0View l0, int ring) {
  dim3 block(256);
  uint32_t nwx = (uint32_t)dst.pitch / 4, groups = ((uint32_t)dst.ph + RZ_ROWS - 1) / RZ_ROWS;
  int wx0 = 0, rg0 = 0, row_end = dst.ph;
  if (ring > 0 && ring < kPad && (kPad - ring) % 4 == 0) {
    wx0 = (kPad - ring) / 4, rg0 = (kPad - ring) / RZ_ROWS, row_end = dst.h + kPad + ring;
    nwx = (uint32_t)((dst.w + kPad + ring + 3) / 4 - wx0), groups = (uint32_t)((row_end + RZ_ROWS - 1) / RZ_ROWS - rg0);
  }
  const uint32_t magic = (uint32_t)((0x100000000ull + nwx - 1) / nwx);
  const uint32_t per_frame = (nwx * groups + 255) / 256;
  const uint32_t pf_magic = (uint32_t)((0x100000000ull + per_frame - 1) / per_frame);
  // vb / per_frame by multiply-high with ceil(2^32 / per_frame) is exact while (items of the launch) * per_frame < 2^32; a launch beyond that
  // (4096^2 planes from batch ~500 on) goes out in slices of whole frames that each stay inside the bound
  const uint32_t max_frames = (uint32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(1, 0xffffffffull / ((uint64_t)per_frame * per_frame)));
  for (int f0 = 0; f0 < batch; f0 += (int)max_frames) {
    const int nb = std::min<int>(batch - f0, (int)max_frames);
    const uint32_t per_xcd = (per_frame * (uint32_t)nb + 7) / 8;
    Level0View v = l0;
    if (v.vbase) v.vbase += (int64_t)f0 * v.frame_stride;
    hipLaunchKernelGGL(k_resize_level, dim3(8 * per_xcd), block, 0, s, d_pyr + (int64_t)f0 * pyr_block, pyr_block, src.plane_off, src.pitch, src.w, dst.plane_off, dst.pitch,
                       dst.ph, dst.w, fast_ok, d_ctab, d_rtab, magic, v, src.h, per_frame, pf_magic, per_xcd, nb, nwx, wx0, rg0, row_end);
  }
}

// =====================================================================================================================
// k_resize_level_rows: the per-level resize of a batch as a walk down row bands (schedule: resize_rows.hpp).  k_resize_level's arithmetic and
// tables; what differs is who computes what.  A wavefront owns 64 consecutive entries of the launch's flattened (frame, dword column) space --
// no lane idles on rows of 51 - 136 dwords -- and UVO_RESIZE_BAND consecutive output rows.  A lane keeps the horizontal pass of two source
// rows in registers (two register sets that swap roles from row to row).  The upper source row of an output row is loaded and filtered only
// when the lane does not hold it; the lower one always (rows_walk says why).  At scale 1.2 and ring 4 that is 1.26 source rows filtered per
// output row where k_resize_level filters 2 (tests/emu/resize_rows_emu.cpp prints the figure per level).  Loads are more than that: the
// look-ahead behind a band's last row is issued and dropped (UVO_RESIZE_AHEAD rows of 1.2 source rows per 16-row band), so a lane loads
// (1.26 + 3 x 1.2 / 16) x 3 = 4.5 dwords per output dword against k_resize_level's 6 -- not the 3.6 a walk without look-ahead would have.
// Counters (profiles/r13_resize_rows_counters.json, level 1): vector instructions 19.3 M -> 14.2 M wave-instructions, fetched bytes 1.25 x
// k_resize_level's: the band's first source row and the look-ahead rows are the neighbouring bands' rows, fetched by both at the same time.
// Everything about a row is wave-uniform.  The band's row-table entries are fetched with ONE vector load (lane j holds row j's) and read
// back with v_readlane: a scalar load per row would put a wait for the scalar cache into every row of the walk.  The decision which rows to
// filter is scalar (resize_rows_step); a row's address is a scalar offset added to the lane's constant address.
struct ResizeRowsArgs {
  const uint8_t* src;  // ROI pixel (0, 0) of the source level of the launch's first frame (the padded plane's, or the caller's image in place)
  uint8_t* dst;        // padded plane of the launch's first frame
  uint32_t src_frame, dst_frame;  // frame strides in bytes (frames * stride < 2^32: resize_rows_max_frames)
  int src_pitch, dst_pitch, sh;
  int guard;           // the source is the caller's image: no load may pass guard_lim
  uint32_t guard_lim;  // offset from a frame's ROI origin of the frame's last whole dword
  const ResizeCol* ctab;
  const ResizeRow* rtab;
  int rtab_last;  // last entry of the (padded) row table
  ResizeRowsRegion r;
  uint32_t nwx_magic, nbands_magic, entries, nitems, per_xcd;
};

static_assert(UVO_RESIZE_AHEAD >= 1 && UVO_RESIZE_BAND >= 2 && UVO_RESIZE_BAND + UVO_RESIZE_AHEAD <= 64,
              "lane j of a wavefront holds the table entry of the band's row j, lanes n .. n + UVO_RESIZE_AHEAD - 1 the look-ahead's");

// the three window dwords of source row sy at the lane's columns.  GUARD (in place, a band that reaches the frame's last source row): a
// window dword behind the frame's last byte is not loaded -- the frame's last dword is, whose bytes carry no weight there (k_resize_level)
template <bool GUARD>
__device__ __forceinline__ void rows_load(const uint8_t* __restrict__ S, int sy, int pitch, uint32_t vsrc, uint32_t glim, uint32_t (&u)[3]) {
  const uint32_t ro = (uint32_t)sy * (uint32_t)pitch;  // scalar
  if (!GUARD) {
    const uint8_t* p = S + ro;  // scalar base + the lane's 32-bit offset: no vector address arithmetic
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = *reinterpret_cast<const uint32_t*>(p + (uint64_t)vsrc + 4 * k);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = *reinterpret_cast<const uint32_t*>(S + (uint64_t)(vsrc + min(ro + 4u * k, glim)));
  }
}
__device__ __forceinline__ void rows_hfilter(const uint32_t (&u)[3], uint32_t sel, const uint32_t (&a0)[4], const uint32_t (&a1)[4], uint32_t (&q)[4]) {
  const uint32_t L = __builtin_amdgcn_perm(u[1], u[0], sel);
  const uint32_t R = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(u[2], u[1], 1), __builtin_amdgcn_alignbyte(u[1], u[0], 1), sel);
  q[0] = hrow<0>(L, R, a0[0], a1[0]), q[1] = hrow<1>(L, R, a0[1], a1[1]), q[2] = hrow<2>(L, R, a0[2], a1[2]), q[3] = hrow<3>(L, R, a0[3], a1[3]);
}
__device__ __forceinline__ uint32_t rows_vfilter(const uint32_t (&q0)[4], const uint32_t (&q1)[4], uint32_t b0s, uint32_t b1s) {
  return vrow(q0[0], q1[0], b0s, b1s) | vrow(q0[1], q1[1], b0s, b1s) << 8 | vrow(q0[2], q1[2], b0s, b1s) << 16 | vrow(q0[3], q1[3], b0s, b1s) << 24;
}

struct RowsLane {  // what a lane keeps for the whole band
  uint32_t a0[4], a1[4], sel;
  uint32_t vsrc, glim, vdst;  // 32-bit offsets from the launch's source / destination base; GUARD: the lane's last loadable offset in a row
  uint32_t tsy, tb;           // lane j: (sy0 | sy1 << 16) and (b0 | b1 << 16) of the band's row j
};

// The walk.  Output row J of the band is computed from ring entry J % R of the raw window dwords (R = UVO_RESIZE_AHEAD + 1) while the loads of
// rows J + 1 .. J + UVO_RESIZE_AHEAD are in flight; the body is unrolled over lcm(2, R) rows, so that ring entries and the slots' roles (row
// parity) are constants of the code and nothing is moved.  The lower source row is loaded and filtered always: it is the one a monotone walk
// misses (it is held only where the table clamps or runs backwards, and filtering it again gives the same words), and a load whose use sits
// behind a branch makes the compiler drain every load in flight before it may reuse the registers.  The upper row (missed on a step of two
// source rows, one output row in five at scale 1.2) takes the branch.  The loads behind the band's last row (clamped into the table, so
// always inside the plane) are issued and dropped: they are the first rows of the band below, which runs next to this one.
template <bool GUARD>
__device__ __forceinline__ void rows_walk(const ResizeRowsArgs& A, const RowsLane& T, int py0, int n) {
  constexpr int AH = UVO_RESIZE_AHEAD, R = AH + 1, U = R % 2 ? 2 * R : R;
  const uint8_t* __restrict__ S = A.src;
  uint8_t* drow = A.dst + (int64_t)py0 * A.dst_pitch;  // scalar: advances by one row per output row
  const int spitch = A.src_pitch;
  uint32_t slot[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  ResizeRowsState st{{-1, -1}};
  uint32_t ua[R][3], ub[R][3];  // raw window dwords of the upper / lower source row
  ResizeRowsStep stp[R];
#pragma unroll
  for (int k = 0; k < AH; ++k) {
    const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)T.tsy, k);
    stp[k] = resize_rows_step(st, k & 1, (int)(e & 0xffffu), (int)(e >> 16));
    if (stp[k].eval0) rows_load<GUARD>(S, (int)(e & 0xffffu), spitch, T.vsrc, T.glim, ua[k]);
    rows_load<GUARD>(S, (int)(e >> 16), spitch, T.vsrc, T.glim, ub[k]);
  }
  for (int j = 0;; j += U) {
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int c = k % R, nx = (k + AH) % R, p = k & 1;
      const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)T.tsy, j + k + AH);
      stp[nx] = resize_rows_step(st, (k + AH) & 1, (int)(e & 0xffffu), (int)(e >> 16));
      if (stp[nx].eval0) rows_load<GUARD>(S, (int)(e & 0xffffu), spitch, T.vsrc, T.glim, ua[nx]);
      rows_load<GUARD>(S, (int)(e >> 16), spitch, T.vsrc, T.glim, ub[nx]);
      const uint32_t bw = (uint32_t)__builtin_amdgcn_readlane((int)T.tb, j + k);
      const uint32_t b0s = (bw & 0xffffu) << 8, b1s = (bw >> 16) << 8;
      if (stp[c].eval0) rows_hfilter(ua[c], T.sel, T.a0, T.a1, slot[p]);
      rows_hfilter(ub[c], T.sel, T.a0, T.a1, slot[p ^ 1]);
      *reinterpret_cast<uint32_t*>(drow + (uint64_t)T.vdst) = rows_vfilter(slot[p], slot[p ^ 1], b0s, b1s);
      drow += A.dst_pitch;
      if (j + k + 1 >= n) return;  // (n >= 1; the way out leaves the loop at once: a path that rejoined it would carry its unused loads along)
    }
  }
}

#ifndef UVO_OCC_RESIZE_ROWS
#define UVO_OCC_RESIZE_ROWS 8
#endif
__global__ __launch_bounds__(256, UVO_OCC_RESIZE_ROWS) void k_resize_level_rows(ResizeRowsArgs A) {
  // workgroup b runs on XCD b & 7 and takes item (b & 7) * per_xcd + (b >> 3) of the list of workgroups; the list is chunk-major, so an XCD
  // walks whole frames and the bands of one column chunk -- which share their boundary source row -- run next to each other
  const uint32_t vb = (blockIdx.x & 7u) * A.per_xcd + (blockIdx.x >> 3);
  const uint32_t item = vb * 4u + (uint32_t)wave_in_block();
  if (item >= A.nitems) return;
  const uint32_t chunk = __umulhi(item, A.nbands_magic);  // item / nbands (exact: resize_rows_max_frames)
  const int band = (int)(item - chunk * (uint32_t)A.r.nbands);
  int py0, n;
  resize_rows_band(A.r, band, &py0, &n);
  const uint32_t lane = threadIdx.x & 63u;
  RowsLane T;
  const uint32_t ent = chunk * 64u + lane;
  // (a lane past the end computes and stores the last entry again -- the same word to the same address: a store under a lane mask would sit
  // behind a branch, and the compiler then waits for the previous row's store before it touches the next row's loads)
  const uint32_t en = min(ent, A.entries - 1u);
  const uint32_t f = __umulhi(en, A.nwx_magic);         // en / nwx
  const int wx = (int)(en - f * (uint32_t)A.r.nwx) + A.r.wx0;
  const uint4 c01 = reinterpret_cast<const uint4*>(A.ctab)[wx * 2], c23 = reinterpret_cast<const uint4*>(A.ctab)[wx * 2 + 1];
  const uint32_t cw[8] = {c01.x, c01.y, c01.z, c01.w, c23.x, c23.y, c23.z, c23.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) T.a0[i] = cw[2 * i] >> 16, T.a1[i] = cw[2 * i + 1] & 0xffffu;
  const uint32_t base = cw[1] >> 16;
  T.sel = (cw[3] >> 16) | (cw[5] & 0xffff0000u);
  T.vsrc = f * A.src_frame + base;
  T.vdst = f * A.dst_frame + (uint32_t)wx * 4u;
  T.glim = A.guard_lim - base;
  // lane j: the table entry of the band's row j; lanes n ..: the look-ahead behind the band's last row (clamped into the table)
  const uint2 te = reinterpret_cast<const uint2*>(A.rtab)[min(py0 + (int)lane, A.rtab_last)];
  T.tsy = te.x, T.tb = te.y;
  // in place, a band that reaches the frame's last source row (its look-ahead included) keeps every load inside the frame
  const bool guard = A.guard && __ballot((int)lane < n + UVO_RESIZE_AHEAD && (int)(te.x >> 16) >= A.sh - 1) != 0ull;
  if (guard) rows_walk<true>(A, T, py0, n);
  else rows_walk<false>(A, T, py0, n);
}

#ifndef UVO_RESIZE_ROWS_MIN_ITEMS
// UVO_PYR_FORM_AUTO: launches of fewer work items (wavefronts) keep k_resize_level.  A level is a ramp, a walk and a tail: with a couple of
// thousand wavefronts on 256 CUs the walk's 16 rows in sequence take as long as k_resize_level's short-lived wavefronts.  640 x 512, 257
// frames, ring 4 (15 316, 10 442, 7 258, 5 152, 3 780, 2 700 and 1 890 items on levels 1 - 7), rocprofv3 at depth 1: levels 1 - 5 are 9.8, 2.1, 1.5,
// 0.4 and 0.8 us shorter as rows, levels 6 and 7 0.3 and 0.4 us longer; k_resize_level behind a level that the rows form wrote is 1.4 us
// longer than behind its own.  bench.py, seven runs a side on one box: thresholds 0 / 2048 / 3072 give medians of 319 200 / 318 900 /
// 317 100 frames/s against the parent's 313 700 -- 0 and 2048 are the same within the runs' spread.  2048 is kept: it gives the benchmark's
// levels 1 - 6 to the rows form and leaves the small launches of batches of 9 - 40 frames, which nobody measured, where they were
// (profiles/r13_resize_rows_ab.txt, profiles/LOG.md r13).
#define UVO_RESIZE_ROWS_MIN_ITEMS 2048
#endif

// frames per launch of the rows form for this level (0: the level keeps k_resize_level -- byte-gather levels, strides the 32-bit lane offsets do
// not cover)
static int64_t resize_rows_frames(const LevelGeom& src, const LevelGeom& dst, int fast_ok, Level0View l0, int ring, int64_t pyr_block) {
  if (!fast_ok) return 0;
  const ResizeRowsRegion r = resize_rows_region(dst.w, dst.h, dst.pitch, ring);
  int64_t frame_bytes = pyr_block;
  if (l0.vbase) {
    if (l0.frame_stride < (int64_t)(src.h - 1) * l0.pitch + src.w) return 0;  // (frames that overlap or run backwards)
    frame_bytes = std::max<int64_t>(frame_bytes, l0.frame_stride);
  }
  return resize_rows_max_frames(r.nwx, r.nbands, frame_bytes);
}

bool resize_level_rows_applies(const LevelGeom& src, const LevelGeom& dst, int fast_ok, int batch, Level0View l0, int ring, int64_t pyr_block, bool forced) {
  if (resize_rows_frames(src, dst, fast_ok, l0, ring, pyr_block) < 1) return false;
  if (forced) return true;
  const ResizeRowsRegion r = resize_rows_region(dst.w, dst.h, dst.pitch, ring);
  return ((int64_t)batch * r.nwx + 63) / 64 * r.nbands >= UVO_RESIZE_ROWS_MIN_ITEMS;
}

void launch_resize_level_rows(hipStream_t s, uint8_t* d_pyr, int64_t pyr_block, const LevelGeom& src, const LevelGeom& dst, const ResizeCol* d_ctab,
                              const ResizeRow* d_rtab, int batch, Level0View l0, int ring) {
  const int max_frames = (int)resize_rows_frames(src, dst, 1, l0, ring, pyr_block);  // >= 1: resize_level_rows_applies
  ResizeRowsArgs A;
  memset(&A, 0, sizeof(A));
  A.r = resize_rows_region(dst.w, dst.h, dst.pitch, ring);
  A.src_pitch = l0.vbase ? l0.pitch : src.pitch, A.dst_pitch = dst.pitch, A.sh = src.h;
  A.src_frame = (uint32_t)(l0.vbase ? l0.frame_stride : pyr_block), A.dst_frame = (uint32_t)pyr_block;
  A.guard = l0.vbase != nullptr;
  A.guard_lim = (uint32_t)((int64_t)(src.h - 1) * A.src_pitch + src.w - 4);  // (rows and the frame's end are dword-aligned in place)
  A.ctab = d_ctab, A.rtab = d_rtab, A.rtab_last = ((dst.ph + 3) & ~3) - 1;
  A.nwx_magic = (uint32_t)((0x100000000ull + (uint32_t)A.r.nwx - 1) / (uint32_t)A.r.nwx);
  A.nbands_magic = (uint32_t)((0x100000000ull + (uint32_t)A.r.nbands - 1) / (uint32_t)A.r.nbands);
  for (int f0 = 0; f0 < batch; f0 += max_frames) {
    const int nb = std::min(batch - f0, max_frames);
    A.src = l0.vbase ? l0.vbase + (int64_t)f0 * l0.frame_stride + (int64_t)kPad * l0.pitch + kPad
                     : d_pyr + (int64_t)f0 * pyr_block + src.plane_off + (int64_t)kPad * src.pitch + kPad;
    A.dst = d_pyr + (int64_t)f0 * pyr_block + dst.plane_off;
    A.entries = (uint32_t)nb * (uint32_t)A.r.nwx;
    A.nitems = (A.entries + 63u) / 64u * (uint32_t)A.r.nbands;
    A.per_xcd = ((A.nitems + 3u) / 4u + 7u) / 8u;
    hipLaunchKernelGGL(k_resize_level_rows, dim3(8 * A.per_xcd), dim3(256), 0, s, A);
  }
}

// =====================================================================================================================
// k_pyr_tiles: a GROUP of consecutive pyramid levels in one launch (plan: pyr_tiles.hpp).  Workgroup = (frame, tile); it walks the group's
// levels in turn: level l is computed from the tile of level l - 1 the workgroup left in LDS (the group's first level: from memory) over
// its own cell -- stored to the padded plane -- and the halo its cell of level l + 1 reads -- stored to LDS only; one workgroup barrier per
// level.  Work item = 4 rows x one dword column, exactly k_resize_level's arithmetic and tables (the 12-byte tap window, two v_perm per
// source row, 11-bit weights x 16), so the planes are the per-level launches' planes byte for byte.
struct PyrTilesArgs {
  uint8_t* pyr;
  int64_t pyr_block;
  const PyrTileLevel* plan;  // [tile][nlevels]
  const ResizeCol* ctab;
  const ResizeRow* rtab;
  Level0View l0;             // level 1 reads the caller's image in place (vbase != NULL)
  int nlevels, first, last, ntiles, batch;
  uint32_t ntiles_magic, per_xcd;
  // the group's source (level first - 1 in memory) and per-level constants of the handle's geometry
  int64_t src_plane_off;
  int src_pitch, src_w, src_h;
  int64_t plane_off[kMaxLevels];
  int pitch[kMaxLevels], xtab_off[kMaxLevels], ytab_off[kMaxLevels];
};

constexpr int kPyrTilesMaxGroup = 8;  // levels above the first whose tables one pass of the staging code covers (deeper groups loop)

// One level of a workgroup's walk.  FROM_LDS: the source is the LDS tile of level l - 1 (SP) and the coefficient tables are the copies
// staged in LDS; otherwise (the group's first level) source and tables are read from memory.  ROWS = output rows per work item: 4 (the
// column entries are fetched once per four rows: the throughput shape) or 1 (four times as many items: a handful of frames spread over
// 1024-thread workgroups, where a level is a latency chain and not a matter of instruction counts).
template <bool FROM_LDS, int ROWS>
__device__ __forceinline__ void pyr_tile_level(const PyrTilesArgs& A, const PyrTileLevel& T, const PyrTileLevel& SP, int l, int f, uint8_t* lds) {
  static_assert(ROWS == 1 || ROWS == RZ_ROWS, "items are single rows or row groups of the row table");
  const ResizeCol* __restrict__ ct = A.ctab + A.xtab_off[l];
  const ResizeRow* __restrict__ rt = A.rtab + A.ytab_off[l];
  const uint4* __restrict__ tabs = reinterpret_cast<const uint4*>(lds + T.tab_off);
  const int ncw = (int)T.ncw;
  const int nitems = ncw * (int)T.nrg * (RZ_ROWS / ROWS);
  // source: the LDS tile of level l - 1 (byte (0, 0) = ROI pixel (lx0, ly0)), or the ROI of level l - 1 in memory
  const bool ip = !FROM_LDS && l == 1 && A.l0.vbase != nullptr;
  const int src_pitch = FROM_LDS ? (int)SP.lw + kPyrTileSlack : (ip ? A.l0.pitch : A.src_pitch);
  const uint8_t* S = nullptr;
  if (!FROM_LDS) S = ip ? A.l0.vbase + f * A.l0.frame_stride + (int64_t)kPad * src_pitch + kPad : A.pyr + f * A.pyr_block + A.src_plane_off + (int64_t)kPad * src_pitch + kPad;
  const uint8_t* SLDS = lds + SP.lds_off - ((int)SP.ly0 * src_pitch + (int)SP.lx0);  // address of ROI pixel (0, 0) if the tile began there
  const int sw = A.src_w, sh = A.src_h;
  const int64_t s_end = ip ? (int64_t)(sh - 1) * src_pitch + sw : INT64_MAX;
  uint8_t* dplane = A.pyr + f * A.pyr_block + A.plane_off[l];
  const int dpitch = A.pitch[l];
  const int tpitch = (int)T.lw + kPyrTileSlack;
  uint8_t* TL = lds + T.lds_off;
  for (int it = (int)threadIdx.x; it < nitems; it += (int)blockDim.x) {
    const int rl = (int)__umulhi((uint32_t)it, T.ncw_magic);  // row group (ROWS = 4) or row (ROWS = 1) of the computed region
    const int cwl = it - rl * ncw;
    const int wx = (int)T.cx0w + cwl;
    const int py0 = (int)T.cy0 + rl * ROWS;
    uint4 c01, c23;
    uint32_t tw[2 * ROWS];
    if (FROM_LDS) {
      c01 = tabs[2 * cwl], c23 = tabs[2 * cwl + 1];
      if (ROWS == RZ_ROWS) {
        const uint4 t01 = tabs[2 * ncw + 2 * rl], t23 = tabs[2 * ncw + 2 * rl + 1];
        const uint32_t q[8] = {t01.x, t01.y, t01.z, t01.w, t23.x, t23.y, t23.z, t23.w};
#pragma unroll
        for (int j = 0; j < 2 * ROWS; ++j) tw[j] = q[j];
      } else {
        const uint2 t0 = reinterpret_cast<const uint2*>(tabs + 2 * ncw)[rl];
        tw[0] = t0.x, tw[1] = t0.y;
      }
    } else {
      c01 = reinterpret_cast<const uint4*>(ct)[wx * 2], c23 = reinterpret_cast<const uint4*>(ct)[wx * 2 + 1];
      if (ROWS == RZ_ROWS) {
        const int rg = py0 >> 2;
        const uint4 t01 = reinterpret_cast<const uint4*>(rt)[rg * 2], t23 = reinterpret_cast<const uint4*>(rt)[rg * 2 + 1];
        const uint32_t q[8] = {t01.x, t01.y, t01.z, t01.w, t23.x, t23.y, t23.z, t23.w};
#pragma unroll
        for (int j = 0; j < 2 * ROWS; ++j) tw[j] = q[j];
      } else {
        const uint2 t0 = reinterpret_cast<const uint2*>(rt)[py0];
        tw[0] = t0.x, tw[1] = t0.y;
      }
    }
    const uint32_t cw[8] = {c01.x, c01.y, c01.z, c01.w, c23.x, c23.y, c23.z, c23.w};
    uint32_t a0[4], a1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = cw[2 * i] >> 16, a1[i] = cw[2 * i + 1] & 0xffffu;
    const uint32_t base = cw[1] >> 16;
    const uint32_t sel = (cw[3] >> 16) | (cw[5] & 0xffff0000u);
    int sy0[ROWS], sy1[ROWS];
    uint32_t b0s[ROWS], b1s[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      sy0[j] = (int)(tw[2 * j] & 0xffffu), sy1[j] = (int)(tw[2 * j] >> 16);
      b0s[j] = (tw[2 * j + 1] & 0xffffu) << 8, b1s[j] = (tw[2 * j + 1] >> 16) << 8;
    }
    uint32_t u[ROWS][3], w[ROWS][3];
    if (FROM_LDS) {
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {
        const uint32_t* p0 = reinterpret_cast<const uint32_t*>(SLDS + sy0[j] * src_pitch + (int)base);
        const uint32_t* p1 = reinterpret_cast<const uint32_t*>(SLDS + sy1[j] * src_pitch + (int)base);
        u[j][0] = p0[0], u[j][1] = p0[1], u[j][2] = p0[2];
        w[j][0] = p1[0], w[j][1] = p1[1], w[j][2] = p1[2];
      }
    } else {
      // (in place, only an item that reaches the frame's last source row has to look at the frame's end: k_resize_level)
      int sy_max = sy1[0];
#pragma unroll
      for (int j = 1; j < ROWS; ++j) sy_max = max(sy_max, sy1[j]);
      const bool guard = ip && sy_max >= sh - 1;
      if (!guard) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
          const uint32_t* p0 = reinterpret_cast<const uint32_t*>(S + (int64_t)sy0[j] * src_pitch + base);
          const uint32_t* p1 = reinterpret_cast<const uint32_t*>(S + (int64_t)sy1[j] * src_pitch + base);
          u[j][0] = p0[0], u[j][1] = p0[1], u[j][2] = p0[2];
          w[j][0] = p1[0], w[j][1] = p1[1], w[j][2] = p1[2];
        }
      } else {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
          const int64_t o0 = (int64_t)sy0[j] * src_pitch + base, o1 = (int64_t)sy1[j] * src_pitch + base;
          const uint32_t* p0 = reinterpret_cast<const uint32_t*>(S + o0);
          const uint32_t* p1 = reinterpret_cast<const uint32_t*>(S + o1);
          u[j][0] = p0[0], u[j][1] = o0 + 4 < s_end ? p0[1] : 0u, u[j][2] = o0 + 8 < s_end ? p0[2] : 0u;
          w[j][0] = p1[0], w[j][1] = o1 + 4 < s_end ? p1[1] : 0u, w[j][2] = o1 + 8 < s_end ? p1[2] : 0u;
        }
      }
    }
    const bool own_x = wx >= (int)T.ox0w && wx < (int)T.ox1w;
    const int tx = wx * 4 - kPad - (int)T.lx0;  // byte column in this level's LDS tile
    const bool tile_x = tx >= 0 && tx < (int)T.lw;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const uint32_t L0 = __builtin_amdgcn_perm(u[j][1], u[j][0], sel);
      const uint32_t R0 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(u[j][2], u[j][1], 1), __builtin_amdgcn_alignbyte(u[j][1], u[j][0], 1), sel);
      const uint32_t L1 = __builtin_amdgcn_perm(w[j][1], w[j][0], sel);
      const uint32_t R1 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w[j][2], w[j][1], 1), __builtin_amdgcn_alignbyte(w[j][1], w[j][0], 1), sel);
      uint32_t v = vrow(hrow<0>(L0, R0, a0[0], a1[0]), hrow<0>(L1, R1, a0[0], a1[0]), b0s[j], b1s[j]);
      v |= vrow(hrow<1>(L0, R0, a0[1], a1[1]), hrow<1>(L1, R1, a0[1], a1[1]), b0s[j], b1s[j]) << 8;
      v |= vrow(hrow<2>(L0, R0, a0[2], a1[2]), hrow<2>(L1, R1, a0[2], a1[2]), b0s[j], b1s[j]) << 16;
      v |= vrow(hrow<3>(L0, R0, a0[3], a1[3]), hrow<3>(L1, R1, a0[3], a1[3]), b0s[j], b1s[j]) << 24;
      const int py = py0 + j;
      if (own_x && py >= (int)T.oy0 && py < (int)T.oy1) *reinterpret_cast<uint32_t*>(dplane + (int64_t)py * dpitch + wx * 4) = v;
      const int ty = py - kPad - (int)T.ly0;
      if (tile_x && ty >= 0 && ty < (int)T.lrows) *reinterpret_cast<uint32_t*>(TL + ty * tpitch + tx) = v;
    }
  }
}

template <int THREADS, int ROWS>
__global__ __launch_bounds__(THREADS) void k_pyr_tiles(PyrTilesArgs A) {
  extern __shared__ __align__(16) uint8_t pyr_lds[];
  // workgroup b runs on XCD b & 7; an XCD walks whole frames (a frame's tiles meet in one L2: the lines two tiles share are merged there)
  const uint32_t vb = (blockIdx.x & 7u) * A.per_xcd + (blockIdx.x >> 3);
  if (vb >= (uint32_t)A.ntiles * (uint32_t)A.batch) return;
  const int f = A.ntiles > 1 ? (int)__umulhi(vb, A.ntiles_magic) : (int)vb;
  const int t = (int)vb - f * A.ntiles;
  const PyrTileLevel* __restrict__ TP = A.plan + (size_t)t * A.nlevels;
  // The coefficient tables of the levels above the first go to LDS now -- every load in flight at once, beside the first level's own
  // fetches -- so that from the second level on nothing waits for memory: a level is LDS reads, arithmetic, stores and a barrier.
  // Per level (ncw + nrg) x 2 uint4: the column entries of the dword columns it computes, the row entries of its row groups.
  {
    uint4 v[kPyrTilesMaxGroup];
#pragma unroll
    for (int k = 0; k < kPyrTilesMaxGroup; ++k) {
      const int l = A.first + 1 + k;
      if (l <= A.last) {
        const PyrTileLevel& T = TP[l];
        const int nc = 2 * (int)T.ncw, n = nc + 2 * (int)T.nrg, i = (int)threadIdx.x;
        if (i < n)
          v[k] = i < nc ? reinterpret_cast<const uint4*>(A.ctab + A.xtab_off[l])[2 * (int)T.cx0w + i]
                        : reinterpret_cast<const uint4*>(A.rtab + A.ytab_off[l])[2 * ((int)T.cy0 >> 2) + (i - nc)];
      }
    }
    pyr_tile_level<false, ROWS>(A, TP[A.first], TP[A.first], A.first, f, pyr_lds);
#pragma unroll
    for (int k = 0; k < kPyrTilesMaxGroup; ++k) {
      const int l = A.first + 1 + k;
      if (l <= A.last) {
        const PyrTileLevel& T = TP[l];
        const int nc = 2 * (int)T.ncw, n = nc + 2 * (int)T.nrg;
        uint4* dst = reinterpret_cast<uint4*>(pyr_lds + T.tab_off);
        if ((int)threadIdx.x < n) dst[threadIdx.x] = v[k];
        for (int i = (int)threadIdx.x + THREADS; i < n; i += THREADS)  // (tiles wider than a workgroup has threads)
          dst[i] = i < nc ? reinterpret_cast<const uint4*>(A.ctab + A.xtab_off[l])[2 * (int)T.cx0w + i]
                          : reinterpret_cast<const uint4*>(A.rtab + A.ytab_off[l])[2 * ((int)T.cy0 >> 2) + (i - nc)];
      }
    }
    for (int l = A.first + 1 + kPyrTilesMaxGroup; l <= A.last; ++l) {  // (groups deeper than one pass covers)
      const PyrTileLevel& T = TP[l];
      const int nc = 2 * (int)T.ncw, n = nc + 2 * (int)T.nrg;
      uint4* dst = reinterpret_cast<uint4*>(pyr_lds + T.tab_off);
      for (int i = (int)threadIdx.x; i < n; i += THREADS)
        dst[i] = i < nc ? reinterpret_cast<const uint4*>(A.ctab + A.xtab_off[l])[2 * (int)T.cx0w + i]
                        : reinterpret_cast<const uint4*>(A.rtab + A.ytab_off[l])[2 * ((int)T.cy0 >> 2) + (i - nc)];
    }
  }
  for (int l = A.first + 1; l <= A.last; ++l) {
    __syncthreads();
    pyr_tile_level<true, ROWS>(A, TP[l], TP[l - 1], l, f, pyr_lds);
  }
}

// the tiles of a plan may take up to kPyrTilesMaxLds bytes of LDS: the kernels' limit is raised to it once per device (hipFuncSetAttribute
// sets the limit on the current device).  A device or runtime that refuses leaves the kernels at the 64 KB every launch may ask for: the
// tile pyramid is an optional launch shape, so *max_lds reports what plans may use and build_tile_set falls back to the per-level launches
// for plans that do not fit -- the extractor itself never fails over it.
int prepare_pyr_tiles(uint32_t* max_lds) {
  static std::mutex mu;
  static uint32_t limit[64] = {0};
  int dev = 0;
  UVO_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  uint32_t got = dev >= 0 && dev < 64 ? limit[dev] : 0;
  if (!got) {
    const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pyr_tiles<256, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, kPyrTilesMaxLds) == hipSuccess &&
                    hipFuncSetAttribute(reinterpret_cast<const void*>(k_pyr_tiles<1024, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, kPyrTilesMaxLds) == hipSuccess &&
                    hipFuncSetAttribute(reinterpret_cast<const void*>(k_pyr_tiles<1024, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, kPyrTilesMaxLds) == hipSuccess;
    if (!ok) (void)hipGetLastError();  // (not an error of the extractor: the plans are just held to the default limit)
    got = ok ? (uint32_t)kPyrTilesMaxLds : 64u * 1024u;
    if (dev >= 0 && dev < 64) limit[dev] = got;
  }
  if (max_lds) *max_lds = got;
  return UVO_OK;
}

int launch_pyr_tiles(hipStream_t s, uint8_t* d_pyr, int64_t pyr_block, const PyrTileLevel* d_plan, const Geom& g, const ResizeCol* d_ctab, const ResizeRow* d_rtab,
                     Level0View l0, int first, int last, int ntiles, uint32_t lds_bytes, int threads, int rows, int batch) {
  PyrTilesArgs A;
  memset(&A, 0, sizeof(A));
  A.pyr = d_pyr, A.pyr_block = pyr_block, A.plan = d_plan, A.ctab = d_ctab, A.rtab = d_rtab, A.l0 = first == 1 ? l0 : Level0View{nullptr, 0, 0, 0};
  A.nlevels = g.nlevels, A.first = first, A.last = last, A.ntiles = ntiles;
  A.src_plane_off = g.lv[first - 1].plane_off, A.src_pitch = g.lv[first - 1].pitch, A.src_w = g.lv[first - 1].w, A.src_h = g.lv[first - 1].h;
  for (int l = 0; l < g.nlevels; ++l) A.plane_off[l] = g.lv[l].plane_off, A.pitch[l] = g.lv[l].pitch, A.xtab_off[l] = g.lv[l].xtab_off, A.ytab_off[l] = g.lv[l].ytab_off;
  A.ntiles_magic = ntiles > 1 ? (uint32_t)((0x100000000ull + (uint32_t)ntiles - 1) / (uint32_t)ntiles) : 0u;  // (one tile per frame: the kernel takes f = vb)
  // (frame index by multiply-high: exact while items * ntiles < 2^32; larger launches go out in slices of whole frames)
  const int max_frames = (int)std::min<uint64_t>(1u << 20, std::max<uint64_t>(1, 0xffffffffull / ((uint64_t)ntiles * ntiles)));
  for (int f0 = 0; f0 < batch; f0 += max_frames) {
    const int nb = std::min(batch - f0, max_frames);
    A.batch = nb, A.per_xcd = ((uint32_t)ntiles * (uint32_t)nb + 7) / 8;
    PyrTilesArgs B = A;
    B.pyr = d_pyr + (int64_t)f0 * pyr_block;
    if (B.l0.vbase) B.l0.vbase += (int64_t)f0 * B.l0.frame_stride;
    if (threads >= 1024 && rows == 1) hipLaunchKernelGGL((k_pyr_tiles<1024, 1>), dim3(8 * B.per_xcd), dim3(1024), lds_bytes, s, B);
    else if (threads >= 1024) hipLaunchKernelGGL((k_pyr_tiles<1024, 4>), dim3(8 * B.per_xcd), dim3(1024), lds_bytes, s, B);
    else hipLaunchKernelGGL((k_pyr_tiles<256, 4>), dim3(8 * B.per_xcd), dim3(256), lds_bytes, s, B);
  }
  return 0;
}

}  // namespace uvo
