// What the two split-product convolutions share: conv5x5_bf16x6_kernel (conv_bf16.h, three bf16 pieces, option
// "precision" 2) and conv5x5_f16x3_kernel (conv_f16.h, two f16 pieces, "precision" 0).  Both are conv 5x5 (128 -> 512) +
// bias + 4-way maxout with every float32 operand split into 16-bit pieces and the piece products accumulated in float32
// on the matrix cores.  Their arithmetic, MFMA order, weight path and stage loop are their own; the frame around them -
// layouts, tile shape, block and lane maps, halo-tile plan, epilogue, weight packer - is stated here, once.
//
// Workgroup = 4 waves x 32 conv channels x one 16x16 (small L: 8x16, CsShape) pixel tile, for one of 4 channel splits;
// 8 input stages of 16 channels, whose 20 x 20 halo tile (all pieces) is brought into LDS by DMA and shared by the waves.
//
// Row reuse.  The 32 pixels of the MFMA N axis are 2 rows x 16 columns (one fragment), so accumulator q (rows 2q, 2q+1 of
// the tile) at tap (dy, dx) reads the B fragment "row pair r = 2q + dy at column offset dx": one fragment (x pieces)
// serves every (q, dy) with 2q + dy = r, and a wave loads 19 row pairs per tap column instead of 8 x 5 = 40.  Even r only
// meets even dy and odd r odd dy, so a tap column dx is two passes - taps dy = 0, 2, 4 against r = 0, 2, .., 18 and taps
// dy = 1, 3 against r = 1, 3, .., 17 - with the pass's weight fragments in registers.
//
// Layouts (one 16-byte load = one MFMA operand; NP pieces)
//   activations  xs[piece NP][c/8 16][P][P][8]   zero border (same geometry as the f32 planes)
//   weights      wq[split 4][cgrp 8][dx 5][wave 4][dy: 0 2 4 1 3][piece NP][cg 2][m 32][8]
//                (conv channel = split*128 + wave*32 + m, input channel = cgrp*16 + cg*8 + e): fragment (tap, piece) of a
//                wave is 1 KB, one pass of a tap column 3 or 2 taps contiguous
//   part         [tiles * tiles * 2 half tiles][CW][2] float64 - half tile h of 16 x 16 tile t at index 2 t + h, in both shapes
// Lane -> pixel of a fragment follows the lane groups ds_read_b128 is served in ({0-3,12-15,20-27} and {4-11,16-19,28-31}
// per half wave): each group reads the 16 consecutive slots of one row = every LDS bank once, at any row pitch >= 20.
#pragma once
#include "common.h"
#include <vector>

namespace dmp {

// Tile shapes (round 6).  NQ = accumulators per wave = row pairs of the pixel tile: 8 -> 16 x 16 pixels (the shape of
// rounds 1-5), 4 -> 8 rows x 16 columns.  Measured (profiles/r06_conv_tile_shapes.txt): the duration of a launch is
// ceil(workgroups / 256 CUs) x T1, T1 = 0.115 ms (f16x3) / 0.175 ms (bf16x6) the time of ONE 16 x 16 workgroup on a CU - a
// second workgroup on the CU doubles it, so what is lost at mid L is the rounding up (L = 200: 676 workgroups = 2.64 per
// CU -> 3; L = 300: 5.64 -> 6).  Half-height tiles halve the unit but cost 1.2 x per MFMA (1.8 instead of 2.1 MFMAs per
// LDS fragment, a 12-row halo for 8 rows, the weight stream per workgroup unchanged): ceil(2 x 2.64) x 0.6 = 3.6 > 3 -
// they LOSE wherever more than 256 half-height workgroups exist (L = 200: 0.399 against 0.356 ms; L = 82 .. 128: equal)
// and WIN where the 16 x 16 shape leaves half the CUs idle: L <= 80 (L = 48: 0.064 against 0.114 ms).  conv_split_rows
// picks them there.  The accumulation order of an output element does not depend on the shape (per stage and tap column:
// taps dy ascending, the products of a tap in the kernel's order), and the InstanceNorm partial sums are formed per
// 8-row half tile in both shapes: the same bits.
// NP = pieces per operand, PITCH = row pitch of the halo tile in LDS (16-byte slots, >= 20).
template <int NQ, int NP_, int PITCH_> struct CsShape {
  static constexpr int NP = NP_, PITCH = PITCH_;
  static constexpr int HCOLS = 20;                                      // columns of the halo tile
  static constexpr int ROWS = 2 * NQ;                                   // pixel rows of the tile
  static constexpr int HALO = ROWS + 4;                                 // rows of the halo tile (20 or 12)
  static constexpr int RP = ROWS + 3;                                   // row pairs r = 0 .. RP - 1 (19 or 11)
  static constexpr int PIECE = 2 * HALO * PITCH;                        // slots of one piece
  static constexpr int IN_SLOTS = NP * PIECE;                           // 16-byte slots of the tile
  static constexpr int IN_PAD = (IN_SLOTS + 63) / 64 * 64;              // the tile's DMA goes in whole waves of 64 slots
  static constexpr int IN_BYTES = IN_PAD * 16;
  static constexpr int WSLOT = NP * 2 * 32;                             // packed weights: slots per wave and tap
  static constexpr int WCOL = 5 * WSLOT;                                // one tap column of one wave
};
// row bands per 16-row tile row for `tiles` x `tiles` 16 x 16 tiles: 2 = the half-height shape, where its workgroups
// (2 x 4 x tiles^2) still find a CU each
inline int conv_split_rows(int tiles) { return 8 * tiles * tiles <= 256 ? 2 : 1; }

// block -> (tile, channel split) map (round 3, tools/r03_map.sh, profiles/r03_conv_block_maps.txt; block b runs on XCD
// b % 8).  Sustained ms per launch of the f16x3 kernel at L = 300 (one stream / two launches in flight), L2-fabric bytes
// per launch (2 x FETCH_SIZE + WRITE_SIZE, Infinity-Cache hits included; 98.7 MB algorithmic), scheduler throughput:
//   0  XCD x: splits {0,1} or {2,3} of a contiguous quarter of the tiles (rounds 1-2)   0.686 / 0.652   306 MB   7.22
//   1  XCD x: all four splits of an eighth of the tiles (a tile read by ONE XCD)         0.687 / 0.659   399 MB
//   2  XCD x: ONE split of half of the tiles (1.64 / 2.46 MB of weight pieces per XCD)    0.675 / 0.645   339 MB   7.28
// Fewer XCDs per tile do not lower the traffic - the weight set no longer fits the L2 beside the activations and comes
// back from the Infinity Cache - and the map with the MOST fabric bytes is the fastest: its weights stay in the 4 MB L2, and
// what the kernel waits for is the weight stream, not the bytes; a tile's input is read by four XCDs at about the same
// time (Infinity-Cache hits).  Map 2 is the one built; 0 and 1 are history.
// Tiles (bands of 2 NQ rows x 16 columns) per XCD half: XCDs 0-3 take the first half of the tiles, 4-7 the second.
__host__ __device__ constexpr int conv_split_tiles_per_xcd(int tiles, int bands) { return (tiles * tiles * bands + 1) >> 1; }
// number of workgroups to launch for tiles x tiles 16 x 16 pixel tiles cut into `bands` row bands each
inline int conv_split_grid(int tiles, int bands = 1) { return 8 * conv_split_tiles_per_xcd(tiles, bands); }

// w: [512][128][5][5] float32 -> packed 16-bit pieces (layout above); split(x, p) writes the NP pieces of one weight
template <int NP, class SPLIT>
inline std::vector<uint16_t> conv_split_pack_weights(const float* w, SPLIT split) {
  const int tap_row[5] = {0, 2, 4, 1, 3};              // slot order inside a column: even pass, then odd pass
  std::vector<uint16_t> q((size_t)4 * 8 * 25 * 4 * NP * 2 * 32 * 8);
  for (int sp = 0; sp < 4; ++sp)
    for (int g = 0; g < 8; ++g)
      for (int dx = 0; dx < 5; ++dx)
        for (int wave = 0; wave < 4; ++wave)
          for (int sl = 0; sl < 5; ++sl)
            for (int cg = 0; cg < 2; ++cg)
              for (int m = 0; m < 32; ++m)
                for (int e = 0; e < 8; ++e) {
                  const int oc = sp * 128 + wave * 32 + m, ic = g * 16 + cg * 8 + e;
                  uint16_t pc[NP];
                  split(w[((size_t)oc * 128 + ic) * 25 + tap_row[sl] * 5 + dx], pc);
                  for (int p = 0; p < NP; ++p)
                    q[(((((((((size_t)sp * 8 + g) * 5 + dx) * 4 + wave) * 5 + sl) * NP + p) * 2 + cg) * 32 + m) * 8) + e] = pc[p];
                }
  return q;
}

#ifdef __HIPCC__
typedef float cs_f32x16 __attribute__((ext_vector_type(16)));          // one accumulator: 32 conv channels x 32 pixels
extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];  // the workgroup's dynamic LDS

// LDS-DMA of 16 bytes per lane; destination = wave-uniform LDS byte address + lane*16.  Issued
// through inline asm so that hipcc does not serialise later LDS reads behind it; completion is
// waited for with cs_wait_vm<N>().
__device__ __forceinline__ void cs_dma16(const void* gsrc, unsigned lds_byte_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
template <int N> __device__ __forceinline__ void cs_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// thread -> wave (uniform), half wave kk (input channels kk*8 .. +7 of a fragment / conv channels of the accumulator),
// lane li of the half wave and its pixel (prow, px) of the 2 x 16 fragment.  cs_lane leaves the pixel at 0: the kernels
// fill it in with cs_lane_pixel(t.li, t.prow, t.px) behind their early exits (computed before them, or assigned to the
// fields without the references, it moves SGPRs inside the bf16 kernels' MFMA loops).
struct CsLane { int lane, wave, kk, li, prow, px; };
__device__ __forceinline__ CsLane cs_lane(int tid) {
  CsLane t;
  t.lane = tid & 63;
  t.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  t.kk = t.lane >> 5;
  t.li = t.lane & 31;
  t.prow = t.px = 0;
  return t;
}
__device__ __forceinline__ void cs_lane_pixel(int li, int& row, int& x) {
  const bool a = li < 4 || (li >= 12 && li < 16) || (li >= 20 && li < 28);
  row = a ? 0 : 1;
  if (a) x = li < 4 ? li : (li < 16 ? li - 8 : li - 12);
  else x = li < 12 ? li - 4 : (li < 20 ? li - 8 : li - 16);
}

// block of a conv_split_grid(tiles, 8 / NQ) launch -> its channel split and tile: XCD x = id & 7 works on ONE channel
// split (x & 3) of a contiguous half of the tiles
struct CsBlock {
  int split;          // conv channels split * 128 .. + 127
  int ty0, tx0;       // first pixel row / column of the tile; trow counts bands of 2 NQ rows
  int64_t half0;      // the tile's first half tile in `part`: 16 x 16 tile (trow / BANDS, tcol), half trow % BANDS
  bool none;          // the odd tile out of the second half: nothing to do
};
template <int NQ> __device__ __forceinline__ CsBlock cs_block(int id, int tiles) {
  constexpr int BANDS = 8 / NQ;                          // row bands per 16-row tile row
  const int xcd = id & 7, slot = id >> 3;
  const int tile = (xcd >> 2) * conv_split_tiles_per_xcd(tiles, BANDS) + slot;
  const int trow = tile / tiles, tcol = tile % tiles;
  CsBlock b;
  b.split = xcd & 3;
  b.none = tile >= tiles * tiles * BANDS;
  b.ty0 = trow * 2 * NQ;
  b.tx0 = tcol * CONV_TILE;
  b.half0 = ((int64_t)(trow / BANDS) * tiles + tcol) * 2 + (trow % BANDS);
  return b;
}

// A band below the last row (half-height shape, L % 16 in 1 .. 8) has nothing to convolve, but the reduction reads its
// half tile's sums: the kernel writes zeros with this and leaves.
__device__ __forceinline__ void cs_zero_sums(const CsBlock& b, const CsLane& t, double* __restrict__ part) {
  if (t.li == 0)
    for (int g4 = 0; g4 < 4; ++g4) {
      const int gch = b.split * 32 + t.wave * 8 + 2 * g4 + t.kk;
      part[(b.half0 * CW + gch) * 2 + 0] = 0.0;
      part[(b.half0 * CW + gch) * 2 + 1] = 0.0;
    }
}

// Halo-tile DMA plan: LDS slot s (of SH::IN_PAD; thread tid of the workgroup moves slots e * 256 + tid) -> uint4 index of
// its source in the planes of input stage 0.  The pad slots and the slots of the row pitch beyond the 20 halo columns
// re-read a valid pixel.
template <class SH> __device__ __forceinline__ int cs_halo_src(int s, int P, const CsBlock& b) {
  const int sc = s < SH::IN_SLOTS ? s : 0;
  const int p = sc / SH::PIECE, r = sc % SH::PIECE;
  const int cg = r / (SH::HALO * SH::PITCH), r2 = r % (SH::HALO * SH::PITCH);
  const int yy = r2 / SH::PITCH;
  int xx = r2 % SH::PITCH;
  xx = xx < SH::HCOLS ? xx : 0;
  return (int)(((int64_t)(p * 16 + cg) * P + b.ty0 + yy) * P + b.tx0 + xx);
}
// One halo tile into LDS at byte address dst (this wave's 64-slot pieces): src = the planes of the stage, in_src(e) =
// cs_halo_src of slot e * 256 + tid, from registers or recomputed - the kernel's choice
template <class SH, class SRC>
__device__ __forceinline__ void cs_tile_dma(const uint4* src, unsigned dst, int wave, SRC&& in_src) {
#pragma unroll
  for (int e = 0; e < SH::IN_PAD / 256; ++e) cs_dma16(src + in_src(e), dst + (wave * 64) * 16 + e * 4096);
  if (wave * 64 < SH::IN_PAD % 256)
    cs_dma16(src + in_src(SH::IN_PAD / 256), dst + (wave * 64) * 16 + (SH::IN_PAD / 256) * 4096);
}

// Epilogue: (SCALED: undo the operand scales,) bias, 4-way max, store, per-channel partial sums per 8-row half tile.  No
// cross-wave reduction: a wave owns its 32 conv channels = 8 maxout channels for all pixels of the tile.
template <bool SCALED, int NQ>
__device__ __forceinline__ void cs_epilogue(const cs_f32x16 (&acc)[NQ], const float* __restrict__ bias, const CsBlock& b,
                                            const CsLane& t, int L, float* __restrict__ u, double* __restrict__ part,
                                            float inv_scale = 0.f) {
  const float* bsp = bias + b.split * 128 + t.wave * 32;
  const int64_t LL = (int64_t)L * L;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int cl = 8 * g4 + 4 * t.kk;                            // first conv channel of the group in the wave
    const int gch = b.split * 32 + t.wave * 8 + 2 * g4 + t.kk;   // maxout channel
    const float bs[4] = {bsp[cl], bsp[cl + 1], bsp[cl + 2], bsp[cl + 3]};
#pragma unroll
    for (int hq = 0; hq < NQ / 4; ++hq) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int q = 4 * hq; q < 4 * hq + 4; ++q) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = acc[q][4 * g4 + j];
          if constexpr (SCALED) a = a * inv_scale + bs[j];
          else a = a + bs[j];
          v = j ? fmaxf(v, a) : a;
        }
        const int y = b.ty0 + 2 * q + t.prow, x = b.tx0 + t.px;
        if (y < L && x < L) {
          u[(int64_t)gch * LL + (int64_t)y * L + x] = v;
          s1 += v;
          s2 += v * v;
        }
      }
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, 32);
        s2 += __shfl_xor(s2, off, 32);
      }
      if (t.li == 0) {
        part[((b.half0 + hq) * CW + gch) * 2 + 0] = (double)s1;
        part[((b.half0 + hq) * CW + gch) * 2 + 1] = (double)s2;
      }
    }
  }
}
#endif  // __HIPCC__

}  // namespace dmp
