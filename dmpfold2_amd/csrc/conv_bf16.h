// conv 5x5 (128 -> 512) + bias + 4-way maxout with float32 semantics on the bf16 matrix cores.
//
// Every float32 operand is split EXACTLY into three bf16 pieces (x = x0 + x1 + x2: 3 x 8 significand
// bits = the 24 of a float32; round-to-nearest pieces, so a finite float32 is the exact sum).  Of the nine piece
// products w_i * x_j the six with i + j <= 2 are accumulated in float32 by v_mfma_f32_32x32x16_bf16; the three
// dropped ones are below 2^-24 of the product, i.e. below the rounding of a float32 multiply.  The result equals
// the float32 convolution to float32 rounding error (measured: max error vs float64 2e-6, the plain f32 kernel
// 5e-6) at 16/6 = 2.67x the f32 MFMA rate.  No range limit (bf16 has float32's exponent), no scales.
// This is the convolution of option "precision" = 2: full-width (24-bit) operands on the 16-bit matrix cores.
//
// Frame, layouts and row reuse: conv_split.h.  A pass's weight fragments are 9 / 6 x 16 bytes per lane; 72 LDS reads per
// tap column and wave instead of 135 for the same 240 MFMAs (the round-1 kernel went tap by tap: 3 weight + 24 activation
// fragments per tap).
//
// Weights go straight from global memory to registers: a wave owns its 32 conv channels, so nobody else would read a
// staged copy, and the packed layout already makes one 16-byte load one MFMA A operand.  Each pass's fragments are loaded
// one pass ahead (15 fragments = 60 registers at the peak), at the head of the pass that runs on the other set.  LDS holds
// nothing but the halo tile, twice: the tile of stage g + 1 is DMA'd into buffer (g + 1) & 1 from inside the first pass of
// stage g, and a stage begins with one wait + ONE barrier (all pieces of tile g have landed, and every wave is done
// reading the buffer that is overwritten next).
//
#pragma once
#include "conv_split.h"

namespace dmp {

typedef __bf16 cq_bf16x8 __attribute__((ext_vector_type(8)));

#ifndef CQ_PITCH_N
#define CQ_PITCH_N 20        // row pitch of the halo tile in LDS (16-byte slots)
#endif
// 2400 / 1440 16-byte slots at pitch 20, padded to 38912 / 23552 bytes; 192 weight slots = 3 KB per wave and tap
template <int NQ> using CqShape = CsShape<NQ, 3, CQ_PITCH_N>;
template <int NQ> constexpr int convq_lds_bytes() { return 2 * CqShape<NQ>::IN_BYTES; }     // two halo tiles: 77824 / 47104
constexpr int CONVQ_LDS_BYTES = convq_lds_bytes<8>();                 // two workgroups per CU (155648 of 163840 bytes)

// round-to-nearest-even float32 -> bf16 bits
__host__ __device__ inline uint16_t cq_bf16_rne(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__host__ __device__ inline float cq_bf16_f32(uint16_t h) {
  return __builtin_bit_cast(float, (uint32_t)h << 16);
}
// x == p[0] + p[1] + p[2] exactly (finite x)
__host__ __device__ inline void split3_bf16(float x, uint16_t p[3]) {
  p[0] = cq_bf16_rne(x);
  const float r1 = x - cq_bf16_f32(p[0]);
  p[1] = cq_bf16_rne(r1);
  const float r2 = r1 - cq_bf16_f32(p[1]);
  p[2] = cq_bf16_rne(r2);
}

// w: [512][128][5][5] float32 -> packed bf16 pieces (layout in conv_split.h)
inline std::vector<uint16_t> pack_conv_weights_bf16(const float* w) {
  return conv_split_pack_weights<3>(w, [](float x, uint16_t* p) { split3_bf16(x, p); });
}

#if defined(__HIPCC__) && defined(CONV_BF16_KERNELS)   // kernels: only the unit that launches them
__device__ __forceinline__ cs_f32x16 cq_mfma(uint4 a, uint4 b, cs_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cq_bf16x8, a),
                                                 __builtin_bit_cast(cq_bf16x8, b), c, 0, 0, 0);
}

// One pass of a tap column: NT taps (rows dy = PAR, PAR + 2, ..) whose weight fragments a[t][piece] sit in registers,
// against the row pairs r = PAR, PAR + 2, .. < 19 read from the halo tile at `il`; the next row pair's three pieces are
// requested before this one's MFMAs.  Per fragment the smallest products go first: w0 x2, w1 x1, w2 x0 (2^-16), then
// w0 x1, w1 x0 (2^-8), then w0 x0 - each product type over the pass's taps, i.e. over different accumulators.
// `mid` runs once between two row pairs, behind the first row pair that uses the pass's last tap: every weight fragment
// has been waited for by then, so what it issues to the vector-memory queue has no wait of this pass behind it.
template <int NQ, int NT, int PAR, class MID>
__device__ __forceinline__ void cq_column_pass(const uint4 (&a)[NT][3], const uint4* il, cs_f32x16 (&acc)[NQ], MID&& mid) {
  constexpr int PIECE = CqShape<NQ>::PIECE, RP = CqShape<NQ>::RP, PITCH = CqShape<NQ>::PITCH;
  uint4 bn0 = il[PAR * PITCH], bn1 = il[PAR * PITCH + PIECE], bn2 = il[PAR * PITCH + 2 * PIECE];
#pragma unroll
  for (int r = PAR; r < RP; r += 2) {
    const uint4 b0 = bn0, b1 = bn1, b2 = bn2;
    if (r + 2 < RP) {
      bn0 = il[(r + 2) * PITCH];
      bn1 = il[(r + 2) * PITCH + PIECE];
      bn2 = il[(r + 2) * PITCH + 2 * PIECE];
    }
#define CQ_TAPS(AP, BV)                                                           \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                              \
      const int q = (r - PAR - 2 * t) / 2;                                        \
      if (r - PAR - 2 * t >= 0 && q < NQ) acc[q] = cq_mfma(a[t][AP], BV, acc[q]); \
    }
    CQ_TAPS(0, b2)
    CQ_TAPS(1, b1)
    CQ_TAPS(2, b0)
    CQ_TAPS(0, b1)
    CQ_TAPS(1, b0)
    CQ_TAPS(0, b0)
#undef CQ_TAPS
    if (r == PAR + 2 * (NT - 1)) mid();
  }
}

// The weight fragments of one pass, straight from the packed weights into registers: fragment (tap t, piece p) of a
// wave is 64 consecutive 16-byte slots (one per lane) at slot t * WSLOT + p * 64 of the pass; `src` includes the lane.
template <int NT>
__device__ __forceinline__ void cq_load_weights(const uint4* __restrict__ src, uint4 (&a)[NT][3]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int p = 0; p < 3; ++p) a[t][p] = src[t * CqShape<8>::WSLOT + p * 64];
}

#ifdef CQ_CLOCK_STAMPS
// Diagnostic build only (-DCQ_CLOCK_STAMPS, never the library's): the first lane of every workgroup stamps the shader
// clock and the 100 MHz reference clock around the stage loop; cycles / ticks x 100 MHz is the clock the chip held under
// the kernel.  The stamps go to a buffer of their own that no kernel reads (dmp_debug_conv_clock copies it to the host).
constexpr int CQ_STAMP_BLOCKS = 2048;
__device__ unsigned long long cq_clock_stamps[CQ_STAMP_BLOCKS][2];
#endif

// grid: conv_split_grid(tiles, 8 / NQ) blocks   block: 256   dynamic LDS: convq_lds_bytes<NQ>() (two workgroups per CU)
template <int NQ>
__global__ __launch_bounds__(256, 2) void conv5x5_bf16x6_kernel(const uint16_t* __restrict__ xs,
                                                                const uint16_t* __restrict__ wq,
                                                                const float* __restrict__ bias, int L, int P,
                                                                int tiles, int nwork, float* __restrict__ u,
                                                                double* __restrict__ part) {
  using SH = CqShape<NQ>;
  const int id = blockIdx.x, tid = threadIdx.x;
  const CsBlock blk = cs_block<NQ>(id, tiles);
  if (blk.none) return;
  CsLane ln = cs_lane(tid);
  if (NQ == 4 && blk.ty0 >= L) {            // a band below the last row: nothing to convolve
    cs_zero_sums(blk, ln, part);
    return;
  }
  cs_lane_pixel(ln.li, ln.prow, ln.px);
  const int wave = ln.wave;
  const int64_t PP = (int64_t)P * P;

  const uint4* in_l = reinterpret_cast<const uint4*>(cs_smem);
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)cs_smem;

  // input-tile DMA plan (cs_halo_src), kept in registers for all stages
  const uint4* xs4 = reinterpret_cast<const uint4*>(xs);
  int in_src[SH::IN_PAD / 256 + 1];
#pragma unroll
  for (int e = 0; e <= SH::IN_PAD / 256; ++e) in_src[e] = cs_halo_src<SH>(e * 256 + tid, P, blk);
  // the halo tile of input stage g into LDS buffer g & 1
  auto tile_dma = [&](int g) {
    cs_tile_dma<SH>(xs4 + (int64_t)g * 2 * PP, lds_base + (g & 1) * SH::IN_BYTES, wave, [&](int e) { return in_src[e]; });
  };
  // tap column c = g * 5 + dx of this wave in the packed weights: even pass at + 0, odd pass at + 3 * WSLOT
  const uint4* wcol = reinterpret_cast<const uint4*>(wq) + (int64_t)blk.split * 8 * 5 * 4 * SH::WCOL +
                      (int64_t)wave * SH::WCOL + ln.lane;
  const int b_base = (ln.kk * SH::HALO + ln.prow) * SH::PITCH + ln.px;      // + r * PITCH + dx (+ piece stride)

  cs_f32x16 acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  // Weight fragments of the even (ae) and the odd (ao) pass of a tap column.  Each set is loaded one pass ahead, at the
  // head of the pass that uses the other one (sched_barrier: left to itself the compiler sinks the loads to the end of
  // that pass), so a load has a whole pass (>= 2300 MFMA cycles) to come back from L2.
  uint4 ae[3][3], ao[2][3];
  tile_dma(0);
  cq_load_weights<3>(wcol, ae);
  __builtin_amdgcn_sched_barrier(0);
#ifdef CQ_CLOCK_STAMPS
  const unsigned long long st_clk = __builtin_amdgcn_s_memtime(), st_real = __builtin_amdgcn_s_memrealtime();
#endif

  for (int g = 0; g < 8; ++g) {
    // Tile g was issued early in stage g - 1 and the first pass's weights one pass ago: nothing younger is in flight, so
    // this drains a queue that is already empty (g = 0: the prologue's loads).  ONE barrier per stage: every wave's pieces
    // of tile g are in LDS, and every wave is done reading buffer (g + 1) & 1, which tile g + 1 is about to overwrite.
    cs_wait_vm<0>();
    __syncthreads();
    const uint4* in_g = in_l + (g & 1) * SH::IN_PAD + b_base;
#pragma unroll 1
    for (int dx = 0; dx < 5; ++dx) {
      const uint4* il = in_g + dx;
      {
        __builtin_amdgcn_sched_barrier(0);
        cq_load_weights<2>(wcol + 3 * SH::WSLOT, ao);
        __builtin_amdgcn_sched_barrier(0);
        // The next tile goes out from inside the stage's first pass, behind the pass's last wait for a weight fragment:
        // vmcnt counts in issue order, so a wait for weights issued before the DMA does not wait for it, and the next
        // wait (head of the following pass) comes most of a pass later.
        cq_column_pass<NQ, 3, 0>(ae, il, acc, [&] {
          if (dx == 0 && g < 7) {
            __builtin_amdgcn_sched_barrier(0);
            tile_dma(g + 1);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
      }
      {
        // the next column's even pass (after the last column: the same column again, unused, instead of a branch)
        const uint4* wnext = wcol + (g * 5 + dx < 39 ? 4 * SH::WCOL : 0);
        __builtin_amdgcn_sched_barrier(0);
        cq_load_weights<3>(wnext, ae);
        __builtin_amdgcn_sched_barrier(0);
        cq_column_pass<NQ, 2, 1>(ao, il, acc, [] {});
        wcol = wnext;
      }
    }
  }
#ifdef CQ_CLOCK_STAMPS
  if (tid == 0 && id < CQ_STAMP_BLOCKS) {
    cq_clock_stamps[id][0] = __builtin_amdgcn_s_memtime() - st_clk;
    cq_clock_stamps[id][1] = __builtin_amdgcn_s_memrealtime() - st_real;
  }
#endif

  cs_epilogue<false>(acc, bias, blk, ln, L, u, part);     // no scales to undo
}
#endif  // __HIPCC__ && CONV_BF16_KERNELS

}  // namespace dmp
