// gru_vertical in the REFERENCE'S ARITHMETIC (network.py:189, 223-224: nn.GRU(22, 512, num_layers=2) in float32): float32
// operands, float32 products and accumulation on v_mfma_f32_16x16x4_f32, gates on the device library's expf / tanhf
// (1-ulp functions, as ATen's vectorised sigmoid / tanh are) - no f16 pieces, no hardware v_exp / v_rcp approximations.
// Selected with option "precision" = 1 (together with the exact-f32 convolution, conv_mode 1) or "vgru_f32" = 1; the
// default path stays the split-f16 form of vgru.hip (three f16 MFMAs per float32 product, 5.3 x the matrix-core rate).
//
// Same decomposition as vgru_persist_kernel (vgru.hip), because a float32 weight is as many bytes as its two f16 pieces
// (what the kernels share as code - slice claim, tile table, reduction through LDS, GRU cell, row barrier, the launcher -
// is in vgru.h; this file holds the float32 products):
//   * weight-stationary and persistent: the group's column tiles are partitioned over the 8 XCDs, the hidden units over the
//     32 CUs of an XCD (CU u: units 16u .. 16u+15 of both layers, all gates, all three products), K over the 4 waves of a
//     CU; wave w keeps its K quarter of the two layer-1 products in 192 AGPRs (A operands of the MFMA straight from the
//     accumulation registers) and of the layer-0 recurrent product in 24 KB of LDS;
//   * the state of a column never leaves its XCD: row boundaries are XCD-local barriers (plain stores + sc1 loads);
//   * per row and 32-column tile a wave multiplies its K quarter: 8 super-steps of 16 k, 72 MFMAs each (3 products x 3 gates
//     x 2 column halves x 4 k quads) = 576 MFMAs of 32 cycles per tile = 7.7 us at the spec clock (the f16 form: 1.44);
//   * the four waves' partial sums meet in LDS, 256 threads finish 16 units x 32 columns x 2 layers.
// k order inside a super-step: the state is stored as float4 rows [k/4][column][k%4]; lane (column c, quad q) loads the
// float4 of k = 16 s + 4 q .. + 3 and MFMA i of the super-step takes component i from every lane, i.e. the k set
// {16 s + 4 q + i : q = 0..3} - the weights are laid out to match when they are loaded into the registers (once per launch).
// Summation order (K quarters in wave order, super-steps ascending, i ascending) does not depend on the grouping: a member's
// result is the same bits alone, in any group and as a rider.
//
// Fallback (the device is shared with another process and the 256 workgroups are not all resident -> row barrier time-out
// -> DMP_FAULT_VGRU_HANDOFF -> option "vgru_persistent" = 0): the same kernel, one launch per alignment row, no barrier,
// workgroup -> (XCD, unit slice) from the block id; every launch re-reads its weights, so this is slow (and correct).
#include "vgru.h"

namespace dmp {

// The inline-assembly MFMAs are invisible to the compiler's hazard recogniser in BOTH directions.  Found on the GPU (first
// build of this kernel, tools/debug_vgru_f32.py): the compiler sinks the zero-initialisation of an accumulator
// (v_mov_b64 v[98:99], 0) to just in front of its first MFMA, and that MFMA then accumulates onto the STALE lower
// half - columns 16..31, rows 4g and 4g+1 wrong by 2e-2, nothing else.  So (1) the accumulators are pinned behind a
// statement that takes all of them and pads wait states before the first MFMA can issue (vf_accumulators_ready), and
// (2) every assembly MFMA carries two wait states of its own in front, for whatever VALU write of an operand the
// compiler may schedule there (free: the matrix pipe is busy 32 cycles per instruction).
__device__ __forceinline__ vp_f32x4 vf_mfma_a(float a, float b, vp_f32x4 c) {                // A from an AGPR
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "a"(a), "v"(b));
  return c;
}
__device__ __forceinline__ void vf_accumulators_ready(vp_f32x4 (&a)[4][2]) {
  asm volatile("s_nop 3" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]),
                           "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]), "+v"(a[3][1]));
}
__device__ __forceinline__ vp_f32x4 vf_mfma_v(float a, float b, vp_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// the compiler does not see the inline-assembly MFMAs: 16 wait states before anything but an MFMA reads their results
// (an 8-pass MFMA needs 11)
__device__ __forceinline__ void vf_mfma_results_ready(vp_f32x4 (&a)[4][2]) {
  asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]),
                                       "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]), "+v"(a[3][1]));
}

constexpr int VF_SS = 8;                                  // super-steps (16 k) of a wave's K quarter
static_assert(4 * VF_SS * 3 * 64 == VP_WL0_SLOTS, "layer 0's float32 weights fill the LDS area of the f16 pieces");

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void vgru_persist_f32_kernel(VStaticF32 st, const VGroupRec* __restrict__ rec, VPSync* __restrict__ sync,
                             int* __restrict__ fault, int t_lo, int t_hi, int ntiles, int barrier) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vf_smem[];
  float4* wl0 = reinterpret_cast<float4*>(vf_smem);                                          // [wave][super-step][gate][lane]
  vp_f32x4* red = reinterpret_cast<vp_f32x4*>(vf_smem + VP_WL0_SLOTS * 16);
  float* tab = reinterpret_cast<float*>(vf_smem + (VP_WL0_SLOTS + VP_RED_SLOTS) * 16);
  __shared__ int sh_u, sh_abort;
  __shared__ int sh_tile[VP_MAX_XCD_TILES][4];
  __shared__ unsigned long long sh_msa[VG_MAX_MEMBERS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned xcc;
  int u;                                                 // this workgroup's hidden-unit slice on its XCD
  if (!vp_claim_slice(sync, fault, barrier, tid, &sh_u, &sh_abort, xcc, u)) return;
  const int j0 = 16 * u, lr = lane & 15, lq = lane >> 4;
  const int Lb = ntiles * VG_TB;
  const int c_lo = (int)(((long long)ntiles * xcc) / 8), c_hi = (int)(((long long)ntiles * (xcc + 1)) / 8);

  // ---- this wave's weights: K quarter w, rows j0 .. j0+15.  Register (s, g, i) of lane (row lr, quad lq) holds
  // W[g 512 + j0 + lr][128 w + 16 s + 4 lq + i] = component i of the float4 at k/4 = 32 w + 4 s + lq.
  float WA[VF_SS * 12], WB[VF_SS * 12];                  // layer-1 input (from h0) and recurrent (from h1) products
#pragma unroll
  for (int s = 0; s < VF_SS; ++s)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int64_t off = (int64_t)(g * 128 + 32 * w + 4 * s + lq) * 512 + j0 + lr;
      const float4 a = st.wx1[off], b = st.wh1[off];
      WA[(s * 3 + g) * 4 + 0] = a.x; WA[(s * 3 + g) * 4 + 1] = a.y; WA[(s * 3 + g) * 4 + 2] = a.z; WA[(s * 3 + g) * 4 + 3] = a.w;
      WB[(s * 3 + g) * 4 + 0] = b.x; WB[(s * 3 + g) * 4 + 1] = b.y; WB[(s * 3 + g) * 4 + 2] = b.z; WB[(s * 3 + g) * 4 + 3] = b.w;
      wl0[((w * VF_SS + s) * 3 + g) * 64 + lane] = st.wh0[off];
    }
  // one-hot input of layer 0: the term a residue code adds to a gate's sum is one weight
  for (int i = tid; i < 3 * 22 * 16; i += 256) {
    const int g = i / (22 * 16), code = (i / 16) % 22, row = i & 15;
    tab[(g * 24 + code) * 16 + row] = st.wx0[(g * 22 + code) * 512 + j0 + row];
  }
  // finishing thread: layer fl, rows j0 + 4 fg .. +3, column fc of the tile
  const int fl = __builtin_amdgcn_readfirstlane(tid >> 7), fg = (tid >> 5) & 3, fc = tid & 31;   // fl: uniform in a wave
  const int flane = 16 * fg + (fc & 15), fnt = fc >> 4;
  const int j4 = j0 + 4 * fg;
  const float4 bR = *reinterpret_cast<const float4*>(st.bias[fl] + j4);
  const float4 bZ = *reinterpret_cast<const float4*>(st.bias[fl] + 512 + j4);
  const float4 bI = *reinterpret_cast<const float4*>(st.bias[fl] + 1024 + j4);
  const float4 bH = *reinterpret_cast<const float4*>(st.bias[fl] + 1536 + j4);
  const int nmem = rec->nmem;
  if (!vp_tile_table(rec, nmem, c_lo, c_hi, tid, fault, sh_tile, sh_msa)) return;
  auto next_active = [&](int ct, int t) { return vp_next_active(sh_tile, c_lo, c_hi, ct, t); };
  typedef unsigned vf_u32x4v __attribute__((vector_size(16)));
  constexpr int VF_SC1 = 16;                             // cache-policy bit of the buffer loads: past the L1, served by the L2
  // super-step ss of a tile's state (both layers, both column halves) -> register slot
  auto load_ss = [&](__amdgpu_buffer_rsrc_t r0, __amdgpu_buffer_rsrc_t r1, int tcol, int ss, vp_f32x4 (&d0)[2], vp_f32x4 (&d1)[2]) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const unsigned off = (unsigned)(((32 * w + 4 * ss + lq) * Lb + tcol + nt * 16 + lr) * 16);
      const vf_u32x4v x0 = __builtin_amdgcn_raw_buffer_load_b128(r0, off, 0, VF_SC1);
      const vf_u32x4v x1 = __builtin_amdgcn_raw_buffer_load_b128(r1, off, 0, VF_SC1);
      d0[nt] = __builtin_bit_cast(vp_f32x4, x0);
      d1[nt] = __builtin_bit_cast(vp_f32x4, x1);
    }
  };
  const unsigned state_bytes = (unsigned)(128 * Lb * 16);          // [j/4 128][Lb] x float4

  float4 f[3];                                           // layer 0's weight fragments of the super-step ahead (from LDS)
#pragma unroll
  for (int g = 0; g < 3; ++g) f[g] = wl0[((w * VF_SS + 0) * 3 + g) * 64 + lane];
  for (int t = t_lo; t < t_hi; ++t) {
    const int par = t & 1;
    // layer 0 state at row t (both layers read it), layer 1 state at row t-1, this thread's layer's previous state
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(st.hT[0][par], 0, state_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(st.hT[1][par ^ 1], 0, state_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rh = fl ? r1 : r0;
    float* hnext = fl ? st.hT[1][par] : st.hT[0][par ^ 1];
    int ct = next_active(c_lo, t);
    // the state streams through four register slots three super-steps ahead of the MFMAs that read it (slot s & 3 holds
    // super-step s of whichever tile needs it next); a row's first tile cannot be requested before the row barrier
    vp_f32x4 b0[4][2], b1[4][2];
    if (ct < c_hi) {
#pragma unroll
      for (int s = 0; s < 3; ++s) load_ss(r0, r1, ct * VG_TB, s, b0[s], b1[s]);
    }
    while (ct < c_hi) {
      const int nx = next_active(ct + 1, t);
      const int ncol = (nx < c_hi ? nx : ct) * VG_TB;
      const int N = __builtin_amdgcn_readfirstlane(sh_tile[ct - c_lo][0]);
      const int L = __builtin_amdgcn_readfirstlane(sh_tile[ct - c_lo][1]);
      const bool act0 = t < N, act1 = t >= 1 && t <= N;
      const int tcol = ct * VG_TB;
      // what the finishing threads need of this tile - their previous state, layer 0's residue code - is requested now
      const int b = tcol + fc;
      const int64_t hoff = ((int64_t)(j4 >> 2) * Lb + b) * 4;
      // (four one-word loads: with ONE 16-byte load the compiler's packed-f32 gate arithmetic took element 0 for every
      // row in the f16 form of this kernel - v_pk_add_f32 ... op_sel_hi:[0,1]; vgru.hip)
      float hp[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        hp[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rh, (unsigned)(hoff * 4 + 4 * i), 0, VF_SC1));
      const int bm = sh_tile[ct - c_lo][2] + fc;                               // the column in ITS alignment
      const uint8_t* msa = reinterpret_cast<const uint8_t*>(sh_msa[sh_tile[ct - c_lo][3]]);
      const int code = (fl == 0 && act0 && bm < L) ? (int)msa[(int64_t)t * L + bm] : 0;
      vp_f32x4 a0[3][2], a1[4][2];                       // layer 0: r z hn; layer 1: r z hn in; x column half
#pragma unroll
      for (int g = 0; g < 3; ++g) { a0[g][0] = vp_f32x4{0, 0, 0, 0}; a0[g][1] = vp_f32x4{0, 0, 0, 0}; }
#pragma unroll
      for (int g = 0; g < 4; ++g) { a1[g][0] = vp_f32x4{0, 0, 0, 0}; a1[g][1] = vp_f32x4{0, 0, 0, 0}; }
      vf_accumulators_ready(a1);
#pragma unroll
      for (int s = 0; s < VF_SS; ++s) {
        // (unconditional - the row's last tile requests its own state again: behind a branch the compiler cannot count
        // the loads in flight and waits for all of them)
        load_ss(r0, r1, s + 3 < VF_SS ? tcol : ncol, (s + 3) & (VF_SS - 1), b0[(s + 3) & 3], b1[(s + 3) & 3]);
        __builtin_amdgcn_sched_barrier(0);               // the loads stay where they are issued
        if (act0) {
          // per k quad the six accumulators (gate x column half) take their MFMA one after the other: a dependent MFMA
          // is six instructions behind the one it waits for
          const float fr[3][4] = {{f[0].x, f[0].y, f[0].z, f[0].w}, {f[1].x, f[1].y, f[1].z, f[1].w}, {f[2].x, f[2].y, f[2].z, f[2].w}};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
              for (int g = 0; g < 3; ++g) a0[g][nt] = vf_mfma_v(fr[g][i], b0[s & 3][nt][i], a0[g][nt]);
        }
        // layer 0's weight fragments of the NEXT super-step (of the next tile after the last one: they do not depend on
        // the tile) leave the LDS under layer 1's MFMAs
#pragma unroll
        for (int g = 0; g < 3; ++g) f[g] = wl0[((w * VF_SS + ((s + 1) & (VF_SS - 1))) * 3 + g) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
        if (act1) {
          // recurrent product (into r, z, hn), then the input product (into r, z, in)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
              for (int g = 0; g < 3; ++g) a1[g][nt] = vf_mfma_a(WB[(s * 3 + g) * 4 + i], b1[s & 3][nt][i], a1[g][nt]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
              for (int g = 0; g < 3; ++g) {
                const int qa = g == 2 ? 3 : g;           // the third gate's input and recurrent sums stay apart
                a1[qa][nt] = vf_mfma_a(WA[(s * 3 + g) * 4 + i], b0[s & 3][nt][i], a1[qa][nt]);
              }
        }
      }
      vf_mfma_results_ready(a1);
      // ---- partial sums of the four K quarters meet in LDS
      vp_store_partials(red, w, lane, a0, a1);
      __syncthreads();
      if (fl ? act1 : act0) {
        const int nq = fl ? 4 : 3, base = fl ? 6 : 0;
        vp_f32x4 sum[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < nq) sum[q] = vp_quarter_sum(red, base + q * 2 + fnt, flane);
        }
        if (fl == 0) {
          sum[0] += vp_onehot_term(tab, 0, code, fg);
          sum[1] += vp_onehot_term(tab, 1, code, fg);
          sum[3] = vp_onehot_term(tab, 2, code, fg);
        }
        const float br[4] = {bR.x, bR.y, bR.z, bR.w}, bz[4] = {bZ.x, bZ.y, bZ.z, bZ.w};
        const float bi[4] = {bI.x, bI.y, bI.z, bI.w}, bh[4] = {bH.x, bH.y, bH.z, bH.w};
        float hn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          hn[i] = vp_gru_cell(sum[0][i], sum[1][i], sum[2][i], sum[3][i], br[i], bz[i], bi[i], bh[i], hp[i]);
        *reinterpret_cast<float4*>(hnext + hoff) = make_float4(hn[0], hn[1], hn[2], hn[3]);
      }
      __syncthreads();                                   // `red` is free for the next tile
      ct = nx;
    }
    if (!barrier) break;                                 // one row per launch: the kernel boundary is the barrier
    if (vp_row_barrier(sync, fault, xcc, u, w, lane, tid, t, t_lo, &sh_abort)) break;
  }
}

int vgru_f32_kernel_attrs(dmp_ctx* c) {
  (void)c;
  DMP_HIP(hipFuncSetAttribute((const void*)vgru_persist_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, VP_LDS_BYTES));
  return DMP_OK;
}

// rows [t_lo, t_hi) of the group set up on `lead` (vgru_group_setup), float32
int vgru_f32_group_steps(dmp_ctx* lead, int t_lo, int t_hi, hipStream_t s) {
  return vgru_f32_launch(vgru_persist_f32_kernel, lead, t_lo, t_hi, s);
}

}  // namespace dmp
