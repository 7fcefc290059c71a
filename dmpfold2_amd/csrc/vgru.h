// Shared by the three translation units of the vertical GRU (vgru.hip: split-f16 products, the fast mode; vgru_f32.hip:
// the reference's float32 instructions; vgru_x3.hip: full-width operands as three bf16 pieces, the default): the group
// record, the skeleton of the three persistent kernels (vp_*), and the launcher of the two float32-state kernels.
#pragma once
#include "common.h"

namespace dmp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 vg_f16x8 __attribute__((ext_vector_type(8)));

// Per-context constants of the step kernel (baked into the hipGraph nodes) ...
struct VStatic {
  const uint4* wx[2];       // [layer]: input weight pieces   [2][3][KQ][512] x 16 bytes (KQ = 4 / 64)
  const uint4* wh[2];       // [layer]: hidden weight pieces  [2][3][64][512] x 16 bytes
  const float* bias[2];     // [layer]: [4][512]: r (b_ir+b_hr), z (b_iz+b_hz), b_in, b_hn
  float inv_scale[2];
  float* hT[2][2];          // [layer][parity] float32 state [128][Lb][4]
  uint16_t* hH[2][2];       // [layer][parity] f16 pieces of 1024*state [2][64][Lb][8]
};
constexpr int VG_TB = 32;              // columns per tile


// column pitch of a member's state: whole 32-column tiles
__host__ __device__ inline int vgru_pitch(int L) { return (L + VG_TB - 1) / VG_TB * VG_TB; }

typedef unsigned vg_u32x4 __attribute__((ext_vector_type(4)));

constexpr int VG_MAX_MEMBERS = 8;                         // contexts served by one group launch

// The state of a group lives in the LEADER's buffers as one wide alignment: member m owns the column tiles
// [tile0, tile0 + ceil(L / 32)), the column pitch is 32 x (number of tiles of the group).  A step kernel therefore
// derives every address of its main loop from its kernel arguments; the record below (device memory, cold at
// every kernel start) is only needed for what happens after the loop: is the tile active at this row, and which
// residue codes does layer 0 read.
struct VMember { const uint8_t* msa; int N, L, tile0, pad; };
struct VGroupRec { int t0, t_end, nmem, pad; VMember mem[VG_MAX_MEMBERS]; };
static_assert(sizeof(VGroupRec) <= 256, "dmp_ctx_create sizes vgru_run for 256 bytes");

typedef float vp_f32x4 __attribute__((ext_vector_type(4)));
constexpr int VP_WL0_SLOTS = 4 * 4 * 6 * 64;                 // [wave][k-step][piece x gate][lane] 16-byte slots: 98 304 B
constexpr int VP_RED_SLOTS = 4 * 14 * 64;                    // [wave][accumulator][lane] float4: 57 344 B
constexpr int VP_TAB_FLOATS = 3 * 24 * 16;                   // [gate][code][row] one-hot input terms: 4 608 B
constexpr int VP_LDS_BYTES = (VP_WL0_SLOTS + VP_RED_SLOTS) * 16 + VP_TAB_FLOATS * 4;     // 160 256 of 163 840
constexpr int VP_MAX_XCD_TILES = 64;                           // (+ 1.1 KB of static LDS: the XCD's tile table)
constexpr int VP_GRID = 256;                                 // one workgroup per CU, 32 per XCD
struct VPSync { unsigned count[8]; unsigned pad[24]; unsigned flag[8][32]; };              // zeroed before every launch
static_assert(sizeof(VPSync) == 128 + 1024, "VPSync layout");
// polls of a row barrier before it gives up (about 0.3 us each: a quarter of a second).  The FIRST barrier of a launch is
// also the residency wait - its 256 workgroups become resident as the kernels of other engines leave the CUs, and a
// float32 convolution at L ~ 2048 runs for 0.1-0.2 s - so it gets eight times the bound (two seconds); later rows only
// wait for workgroups that are known to be running.
constexpr unsigned VP_BARRIER_SPINS = 800000u;
constexpr unsigned VP_BARRIER_SPINS_FIRST = 8u * VP_BARRIER_SPINS;

// ---------------------------------------------------------------------------------------------------------------
// The skeleton of the persistent kernels: what does not depend on the arithmetic of the products.  A kernel keeps its
// own product loop, its prefetch schedule and the order of its statements; every __syncthreads() of the skeleton is
// inside the function that needs it.  vgru_persist_kernel and vgru_persist_f32_kernel are built from all of it;
// vgru_persist_x3_kernel (256 + 256 registers, 14 of them spilled) takes vp_row_barrier, which leaves its instruction
// stream as it was, and keeps its own text of the rest: with every function below its registers were allocated
// differently and its chain ran 4 % slower (profiles/vgru_skeleton_refactor.txt).
// ---------------------------------------------------------------------------------------------------------------
// Which XCD this workgroup works for and which hidden-unit slice (16 u .. 16 u + 15) it takes there; false = leave the
// kernel (all threads together).  With the row barrier on, the XCD is the one the workgroup really runs on (its L2 is
// where the barrier's plain stores stop) and the slice is the order of arrival; with one row per launch nothing
// depends on the placement and both come from the block id.
__device__ __forceinline__ bool vp_claim_slice(VPSync* __restrict__ sync, int* __restrict__ fault, int barrier, int tid,
                                               int* sh_u, int* sh_abort, unsigned& xcc, int& u) {
  if (barrier) {
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 7u;
    if (tid == 0) {
      *sh_u = (int)__hip_atomic_fetch_add(&sync->count[xcc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *sh_abort = 0;
    }
  } else {
    xcc = blockIdx.x & 7u;
    if (tid == 0) { *sh_u = (int)(blockIdx.x >> 3); *sh_abort = 0; }
  }
  __syncthreads();
  u = *sh_u;
  if (u >= 32) {                                         // more than 32 workgroups landed on this XCD: another one is short
    if (tid == 0) atomicOr(fault, DMP_FAULT_VGRU_HANDOFF);
    return false;
  }
  return true;
}

// This XCD's column tiles [c_lo, c_hi): {rows N, columns L, first column of the tile in ITS alignment, member} and the
// members' alignments - from the group record in global memory once per launch (a tile's bookkeeping was a chain of
// four to six dependent scalar loads at the head of every tile before).  false = leave the kernel.
// (The bf16 kernel builds its own table: rotated by the slice number, with a fifth column that names the tile.)
__device__ __forceinline__ bool vp_tile_table(const VGroupRec* __restrict__ rec, int nmem, int c_lo, int c_hi, int tid,
                                              int* __restrict__ fault, int (*sh_tile)[4], unsigned long long* sh_msa) {
  if (c_hi - c_lo > VP_MAX_XCD_TILES) {                  // (the host never builds such a group: 8 x 2048 columns = 64 tiles per XCD)
    if (tid == 0) atomicOr(fault, DMP_FAULT_VGRU_HANDOFF);
    return false;
  }
  for (int i = tid; i < c_hi - c_lo; i += 256) {
    const int tile = c_lo + i;
    int mi = 0;
    for (int m = 1; m < VG_MAX_MEMBERS; ++m)
      if (m < nmem && tile >= rec->mem[m].tile0) mi = m;
    sh_tile[i][0] = rec->mem[mi].N;
    sh_tile[i][1] = rec->mem[mi].L;
    sh_tile[i][2] = (tile - rec->mem[mi].tile0) * VG_TB;
    sh_tile[i][3] = mi;
  }
  if (tid < VG_MAX_MEMBERS) sh_msa[tid] = tid < nmem ? (unsigned long long)rec->mem[tid].msa : 0ull;
  __syncthreads();
  return true;
}

// first entry >= ct of the table that is computed at row t (layer 0: t < N; layer 1, one row behind: 1 <= t <= N), or c_hi
__device__ __forceinline__ int vp_next_active(const int (*sh_tile)[4], int c_lo, int c_hi, int ct, int t) {
  for (; ct < c_hi; ++ct) {
    const int N = __builtin_amdgcn_readfirstlane(sh_tile[ct - c_lo][0]);
    if (t < N || (t >= 1 && t <= N)) break;
  }
  return ct;
}

// the partial sums of wave w's K quarter go to LDS: accumulators 0..5 = layer 0 (r z hn x column half), 6..13 = layer 1
// (r z hn in x column half)
__device__ __forceinline__ void vp_store_partials(vp_f32x4* red, int w, int lane, const vp_f32x4 (&a0)[3][2],
                                                  const vp_f32x4 (&a1)[4][2]) {
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) red[(w * 14 + g * 2 + nt) * 64 + lane] = a0[g][nt];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) red[(w * 14 + 6 + g * 2 + nt) * 64 + lane] = a1[g][nt];
}

// accumulator `a` of the finishing thread's lane: the four K quarters in wave order
__device__ __forceinline__ vp_f32x4 vp_quarter_sum(const vp_f32x4* red, int a, int flane) {
  return ((red[(0 * 14 + a) * 64 + flane] + red[(1 * 14 + a) * 64 + flane]) + red[(2 * 14 + a) * 64 + flane]) +
         red[(3 * 14 + a) * 64 + flane];
}

// the one-hot input of layer 0: what residue code `code` adds to gate g's sums of rows 4 fg .. 4 fg + 3
__device__ __forceinline__ vp_f32x4 vp_onehot_term(const float* tab, int g, int code, int fg) {
  const float* t = tab + (g * 24 + code) * 16 + 4 * fg;
  return vp_f32x4{t[0], t[1], t[2], t[3]};
}

// network.py:224 -> ATen's GRU cell: r = sigmoid(i_r + h_r), z = sigmoid(i_z + h_z), n = tanh(i_n + r * h_n),
// h' = (h - n) * z + n, on the device library's expf / tanhf (the float32 kernel; the bf16 kernel repeats it; the f16
// kernel's cell - scaled sums, hardware gate functions, piece stores - is a different algorithm)
__device__ __forceinline__ float vp_gru_cell(float s_r, float s_z, float s_hn, float s_in, float b_r, float b_z, float b_in,
                                             float b_hn, float h) {
  const float rg = 1.0f / (1.0f + expf(-(s_r + b_r)));
  const float zg = 1.0f / (1.0f + expf(-(s_z + b_z)));
  const float ng = tanhf((s_in + b_in) + rg * (s_hn + b_hn));
  return (h - ng) * zg + ng;
}

// Row boundary: every workgroup of this XCD has written its rows of the new state.  true = leave the row loop.
// A workgroup of this XCD is missing for good (not resident, or one XCD got a 33rd workgroup and another is short):
// the fault bit is raised and the outputs of this prediction become NaN - leave the row loop now, the whole
// workgroup together, instead of waiting the full bound again at each of the up to 3001 rows that are left
// (seconds per row = a GPU that looks hung for hours before dmp_sync_faults returns).
__device__ __forceinline__ bool vp_row_barrier(VPSync* __restrict__ sync, int* __restrict__ fault, unsigned xcc, int u, int w,
                                               int lane, int tid, int t, int t_lo, int* sh_abort) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's stores have reached the L2
  __syncthreads();
  const unsigned epoch = (unsigned)(t - t_lo + 1);
  if (tid == 0) asm volatile("global_store_dword %0, %1, off" :: "v"(&sync->flag[xcc][u]), "v"(epoch) : "memory");
  if (w == 0) {
    const unsigned* fp = &sync->flag[xcc][lane & 31];
    bool ok = false;
    const unsigned bound = t == t_lo ? VP_BARRIER_SPINS_FIRST : VP_BARRIER_SPINS;      // the first barrier is the residency wait
    for (unsigned spins = 0; spins < bound && !ok; ++spins) {
      unsigned v;
      asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(fp) : "memory");
      ok = __builtin_amdgcn_ballot_w64(v < epoch) == 0ull;
    }
    if (!ok && lane == 0) { atomicOr(fault, DMP_FAULT_VGRU_HANDOFF); *sh_abort = 1; }
  }
  __syncthreads();
  return *sh_abort != 0;
}


// Per-launch constants of the float32 and the three-piece bf16 kernel: the float32 weight pack and the float32 state
struct VStaticF32 {
  const float4* wh0;        // layer-0 recurrent weights  [gate 3][k/4 = 128][512 j] x float4 (k % 4)
  const float4* wx1;        // layer-1 input weights      (same layout)
  const float4* wh1;        // layer-1 recurrent weights
  const float* wx0;         // layer-0 input weights with the embedding folded in: [gate 3][code 22][512 j]
  const float* bias[2];     // [layer]: [4][512]: r (b_ir+b_hr), z (b_iz+b_hz), b_in, b_hn
  float* hT[2][2];          // [layer][parity] float32 state [128][Lb][4]
  uint4* wq;                // vgru_x3.hip only: the weight pieces a wave streams instead of holding: [workgroup 256][wave 4][K step 4][6][lane 64]
};
typedef void (*vgru_f32_kernel_t)(VStaticF32, const VGroupRec*, VPSync*, int*, int, int, int, int);

// rows [t_lo, t_hi) of the group set up on `lead` (vgru_group_setup) with one of the two float32-state kernels
inline int vgru_f32_launch(vgru_f32_kernel_t kernel, dmp_ctx* lead, int t_lo, int t_hi, hipStream_t s) {
  const int nt = lead->vg_ntiles;
  if (t_hi > lead->vg_maxN + 1) t_hi = lead->vg_maxN + 1;
  if (t_lo < 0) t_lo = 0;
  if (t_lo >= t_hi) return DMP_OK;
  const Weights& W = lead->W;
  VStaticF32 st{};
  st.wh0 = reinterpret_cast<const float4*>(W.v_f32[0]);
  st.wx1 = reinterpret_cast<const float4*>(W.v_f32[1]);
  st.wh1 = reinterpret_cast<const float4*>(W.v_f32[2]);
  st.wx0 = W.v_wx0f;
  st.bias[0] = W.v_b0; st.bias[1] = W.v_b1;
  for (int l = 0; l < 2; ++l)
    for (int p = 0; p < 2; ++p) st.hT[l][p] = lead->hT[l][p];
  st.wq = reinterpret_cast<uint4*>(lead->vgru_wq);
  const VGroupRec* rec = reinterpret_cast<const VGroupRec*>(lead->vgru_run);
  VPSync* sync = reinterpret_cast<VPSync*>(lead->vgru_sync);
  // A device without 256 CUs in 8 XCDs (partitioned / CPX modes: vgru_persist_ok is false) gets the launch-per-row form
  // below: with the barrier off the kernel takes its (XCD, slice) from the block id and depends on no placement.
  if (lead->vgru_persist && lead->vgru_persist_ok) {
    // needs every one of its 256 workgroups resident (row barriers): ordered against the process's other persistent
    // launches and cluster kernels on this device (CoResident, common.h)
    CoResident guard(lead, s, true);
    if (guard.status()) return guard.status();
    DMP_HIP(hipMemsetAsync(sync, 0, sizeof(VPSync), s));
    hipLaunchKernelGGL(kernel, dim3(VP_GRID - (lead->vgru_debug_drop_wg ? 1 : 0)), dim3(256), VP_LDS_BYTES, s, st, rec, sync,
                       lead->seq_abort, t_lo, t_hi, nt, 1);
    DMP_LAUNCH_CHECK();
    return guard.done();
  }
  for (int t = t_lo; t < t_hi; ++t)
    hipLaunchKernelGGL(kernel, dim3(VP_GRID), dim3(256), VP_LDS_BYTES, s, st, rec, sync, lead->seq_abort, t, t + 1, nt, 0);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// vgru_f32.hip: rows [t_lo, t_hi) of the group set up on `lead` in float32 (option "vgru_f32")
int vgru_f32_group_steps(dmp_ctx* lead, int t_lo, int t_hi, hipStream_t s);
int vgru_f32_kernel_attrs(dmp_ctx* c);
// vgru_x3.hip: the same rows with every float32 operand as three exact bf16 pieces (option "vgru_f32" = 2)
int vgru_x3_group_steps(dmp_ctx* lead, int t_lo, int t_hi, hipStream_t s);
int vgru_x3_kernel_attrs(dmp_ctx* c);

}  // namespace dmp
