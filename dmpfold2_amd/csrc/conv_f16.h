// conv 5x5 (128 -> 512) + bias + 4-way maxout with float32-grade accuracy on the f16 matrix cores.
//
// Every float32 operand is split into two f16 pieces, x = x0 + x1 with x0 = f16(x), x1 = f16(x - x0)
// (22 significand bits; the weights are first scaled by a power of two S so that their low pieces
// stay normal numbers: S*w = w0 + w1).  The three products w0 x0, w0 x1, w1 x0 are accumulated in
// float32 by v_mfma_f32_32x32x16_f16 and the accumulator is scaled back by 1/S (exact).  The dropped
// w1 x1 term is 2^-22 of the product.  Measured against a float64 convolution the result has the
// SAME error as a float32 convolution (CPU emulation: max 4.7e-6 vs 4.9e-6 for PyTorch's float32
// conv on the same data; GPU: tests/test_gpu_parity.py::test_conv_paths_error_vs_float64) because
// the float32 accumulation of the 3200-term sums dominates both.  Cost: 3 f16 MFMAs per float32
// MFMA-equivalent = 16/3 = 5.3x the f32 matrix-core rate.
//
// Range and activation scale (round 4).  The pieces are taken of 2^e x, with e chosen per residual block at
// dmp_weights_finalize (api.hip: the largest e that keeps a bound of the block's input, built from the InstanceNorm
// gamma / beta of the blocks before it, below 32768; undone exactly, together with the weight scale, in this kernel's
// epilogue), so the low pieces of the bulk of the activations are NORMAL f16 numbers whatever scale the trunk sits at
// (unscaled, a value below 0.125 has a subnormal low piece and one below 6e-5 a subnormal high piece: 25 x the
// float32 kernel's error at trunk scale 2^-16, tests/test_gpu_parity.py::
// test_unscaled_pieces_lose_precision_on_small_activations).  |2^e x| must stay below 65504 (f16 max): the producer
// kernels raise the context's fault flag at |2^e x| >= 60000; a trunk that would leave the range unscaled is scaled
// DOWN instead.  Option "act_scaling" = 0 restores unscaled pieces (e = 0).
//
// Frame, layouts and row reuse: conv_split.h.  The halo tile (both pieces) is 30 KB; the two passes of a tap column hold
// 24 and 16 weight registers and share a 6 KB weight buffer per wave (3 tap slots, refilled by LDS-DMA for the next pass as
// soon as the fragments are in registers).  240 LDS reads per stage and wave instead of 450 for the same 600 MFMAs:
// Sustained (tools/ubench_conv_sustained.hip; the chip sits at its power cap, 1340 W at 1.83 GHz, so a
// 35 ms burst flatters any change): 0.655-0.660 ms per launch at L = 300 against 0.676 for the tap-by-tap
// kernel it replaces, 0.628 against 0.648 with two launches in flight.
#pragma once
#include "conv_split.h"
#include <cmath>

namespace dmp {

typedef _Float16 ch_f16x8 __attribute__((ext_vector_type(8)));

#ifndef CH_PITCH_N
#define CH_PITCH_N 24        // row pitch of the halo tile in LDS (16-byte slots); any value >= 20 is conflict free.
                             // 24 -> 54 KB per workgroup: two per CU and room for other targets' kernels.  20 -> 50 KB
                             // lets a third workgroup in (3 waves per SIMD): sustained 0.665 against 0.667 ms - at
                             // the power cap more occupancy buys nothing, and the room beside the two is worth more
#endif
// 1920 / 1152 16-byte slots = 30720 / 18432 bytes at pitch 24; 128 weight slots = 2 KB per wave and tap
template <int NQ> using ChShape = CsShape<NQ, 2, CH_PITCH_N>;
constexpr int CH_WBUF = 3 * ChShape<8>::WSLOT;                        // per-wave LDS weight buffer: 3 tap slots
template <int NQ> constexpr int convh_lds_bytes() { return ChShape<NQ>::IN_BYTES + 4 * CH_WBUF * 16; }      // 55296 / 43008
constexpr int CONVH_LDS_BYTES = convh_lds_bytes<8>();

__host__ __device__ inline uint16_t ch_f16_bits(float f) {
  const _Float16 h = (_Float16)f;                                     // round to nearest even
  return __builtin_bit_cast(uint16_t, h);
}
__host__ __device__ inline float ch_f16_f32(uint16_t b) {
  return (float)__builtin_bit_cast(_Float16, b);
}
// x ~= p[0] + p[1]
__host__ __device__ inline void split2_f16(float x, uint16_t p[2]) {
  p[0] = ch_f16_bits(x);
  p[1] = ch_f16_bits(x - ch_f16_f32(p[0]));
}

// power-of-two scale that puts max|w| into [512, 1024)
inline float conv_weight_scale_f16(const float* w, size_t n) {
  float m = 0.f;
  for (size_t i = 0; i < n; ++i) m = std::fmax(m, std::fabs(w[i]));
  if (!(m > 0.f)) return 1.f;
  int e;
  std::frexp(m, &e);                    // m = f * 2^e, f in [0.5, 1)
  return std::ldexp(1.0f, 10 - e);      // m * scale in [512, 1024)
}

// w: [512][128][5][5] float32 -> packed f16 pieces of scale * w (layout in conv_split.h)
inline std::vector<uint16_t> pack_conv_weights_f16(const float* w, float scale) {
  return conv_split_pack_weights<2>(w, [scale](float x, uint16_t* p) { split2_f16(scale * x, p); });
}

#if defined(__HIPCC__) && defined(CONV_F16_KERNELS)   // kernels: only the unit that launches them
__device__ __forceinline__ cs_f32x16 ch_mfma(uint4 a, uint4 b, cs_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(ch_f16x8, a),
                                                __builtin_bit_cast(ch_f16x8, b), c, 0, 0, 0);
}
// Issue efficiency is NOT what bounds this kernel (round 3, gpurun_out r03d, profiles/r03_conv_variants.txt).  The
// compiler sinks a row pair's ds_reads down to their first use (a wait for a read issued two instructions earlier
// before every third to ninth MFMA: the LDS latency shows on every row pair).  Two variants were built and measured in
// round 3 (removed in round 4): "pinned" - a scheduling barrier behind the reads keeps them one row pair ahead (188
// VGPRs, lifting the 168 cap) - and "pipelined" - additionally the next pass's weight fragments and first B fragment
// fetched during the current one (206 VGPRs).  Sustained at L = 300, same box: 0.659 ms per launch as shipped, 0.654
// uncapped, 0.650 pinned, 0.647 pipelined (two launches in flight: 0.646 / 0.644 / 0.642 / 0.637): the stalls go and
// 1.8 % of the time with them - the chip sits at its power cap (section 4 of DESIGN.md) and gives the issue slots
// back as clock.  In the scheduler the shipped form is the fastest (6.95 structures/s against 6.82 .. 6.91): the
// larger footprints take registers from the kernels that run beside the convolutions.
// One pass of a tap column: NT taps (rows dy = PAR, PAR + 2, ..) whose weight fragments a[t][piece] sit in
// registers, against the row pairs r = PAR, PAR + 2, .. < 19 read from the halo tile at `il`.
// Per fragment the small products go first (w0 x1, w1 x0), then w0 x0.
template <int NQ, int NT, int PAR>
__device__ __forceinline__ void ch_column_pass(const uint4 (&a)[NT][2], const uint4* il, cs_f32x16 (&acc)[NQ]) {
  constexpr int PIECE = ChShape<NQ>::PIECE, RP = ChShape<NQ>::RP, PITCH = ChShape<NQ>::PITCH;
  uint4 bn0 = il[PAR * PITCH], bn1 = il[PAR * PITCH + PIECE];
#pragma unroll
  for (int r = PAR; r < RP; r += 2) {
    const uint4 b0 = bn0, b1 = bn1;
    if (r + 2 < RP) {
      bn0 = il[(r + 2) * PITCH];
      bn1 = il[(r + 2) * PITCH + PIECE];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int q = (r - PAR - 2 * t) / 2;
      if (r - PAR - 2 * t >= 0 && q < NQ) acc[q] = ch_mfma(a[t][0], b1, acc[q]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int q = (r - PAR - 2 * t) / 2;
      if (r - PAR - 2 * t >= 0 && q < NQ) acc[q] = ch_mfma(a[t][1], b0, acc[q]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int q = (r - PAR - 2 * t) / 2;
      if (r - PAR - 2 * t >= 0 && q < NQ) acc[q] = ch_mfma(a[t][0], b0, acc[q]);
    }
  }
}

// Footprint: the register budget is capped at 168 VGPRs (3 waves per SIMD; the input-tile DMA plan is
// recomputed per stage instead of living in registers - kept there, the cap parked it and some epilogue
// constants in 68 bytes of scratch per lane, 25 MB of extra writes per launch in WRITE_SIZE; 8 bytes remain),
// and 54 KB of LDS let exactly two workgroups share a CU (a third does not fit).  Two of them leave 176
// registers per SIMD lane and 52 KB of LDS to the kernels of other targets that run beside the convolutions in
// throughput mode (vertical GRU step 156 registers / 32 KB, norm 108, Gauss-Jordan update 92); uncapped
// (194 registers) the same kernel cost the scheduler 6 % although it is faster alone.
// grid: conv_split_grid(tiles, 8 / NQ) blocks   block: 256   dynamic LDS: convh_lds_bytes<NQ>()
template <int NQ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void conv5x5_f16x3_kernel(const uint16_t* __restrict__ xs,
                                                               const uint16_t* __restrict__ wq,
                                                               const float* __restrict__ bias, float inv_scale,
                                                               int L, int P, int tiles, int nwork,
                                                               float* __restrict__ u, double* __restrict__ part) {
  using SH = ChShape<NQ>;
  const int tid = threadIdx.x;
  const CsBlock blk = cs_block<NQ>(blockIdx.x, tiles);
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
  const uint4* w_l = reinterpret_cast<const uint4*>(cs_smem + SH::IN_BYTES) + wave * CH_WBUF;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)cs_smem;
  const unsigned w_lds_addr = lds_base + SH::IN_BYTES + wave * (CH_WBUF * 16);

  const uint4* xs4 = reinterpret_cast<const uint4*>(xs);
  const uint4* wq4 = reinterpret_cast<const uint4*>(wq) + (int64_t)blk.split * 8 * 5 * 4 * SH::WCOL +
                     (int64_t)wave * SH::WCOL + ln.lane;
  const int b_base = (ln.kk * SH::HALO + ln.prow) * SH::PITCH + ln.px;      // + r * PITCH + dx (+ piece stride)

  cs_f32x16 acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  // pass h = 2 * (g * 5 + dx) + odd: stream its 3 (even) or 2 (odd) tap slots into this wave's buffer
  auto wdma = [&](int h) {
    const int odd = h & 1;
    const uint4* src = wq4 + (int64_t)(h >> 1) * 4 * SH::WCOL + odd * 3 * SH::WSLOT;
    if (odd) {
#pragma unroll
      for (int i = 0; i < 4; ++i) cs_dma16(src + 64 * i, w_lds_addr + 1024 * i);
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) cs_dma16(src + 64 * i, w_lds_addr + 1024 * i);
    }
  };
  wdma(0);

  for (int g = 0; g < 8; ++g) {
    __syncthreads();                                   // every wave is done with the previous tile
    {
      // input-tile DMA plan (cs_halo_src): recomputed at every stage (a few dozen integer operations, 8 times per
      // workgroup) rather than kept in registers across the tap loops
      int t = tid;
      asm volatile("" : "+v"(t));                    // opaque per stage: the plan is not hoisted out of the loop
      cs_tile_dma<SH>(xs4 + (int64_t)g * 2 * PP, lds_base, wave, [&](int e) { return cs_halo_src<SH>(e * 256 + t, P, blk); });
    }
    cs_wait_vm<0>();
    __syncthreads();                                   // the tile of every wave has landed
#pragma unroll 1
    for (int dx = 0; dx < 5; ++dx) {
      const uint4* il = in_l + b_base + dx;
      const int h0 = 2 * (g * 5 + dx);
      {
        // this pass's weights: issued one pass ago (at the head of a stage everything was drained with the tile)
        cs_wait_vm<0>();
        uint4 a[3][2];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          a[t][0] = w_l[t * SH::WSLOT + ln.lane];
          a[t][1] = w_l[t * SH::WSLOT + 64 + ln.lane];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wdma(h0 + 1);                                  // the buffer is free: stream the next pass
        ch_column_pass<NQ, 3, 0>(a, il, acc);
      }
      {
        cs_wait_vm<0>();
        uint4 a[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          a[t][0] = w_l[t * SH::WSLOT + ln.lane];
          a[t][1] = w_l[t * SH::WSLOT + 64 + ln.lane];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (h0 + 2 < 80) wdma(h0 + 2);
        ch_column_pass<NQ, 2, 1>(a, il, acc);
      }
    }
  }

  cs_epilogue<true>(acc, bias, blk, ln, L, u, part, inv_scale);     // undoes the weight and activation scales
}
#endif  // __HIPCC__ && CONV_F16_KERNELS

}  // namespace dmp
