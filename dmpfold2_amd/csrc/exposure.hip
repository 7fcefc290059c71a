// option "exposure": solvent exposure of the final backbone, and of the native's where option "score_native" holds a whole
// native trace (include/dmpfold_hip.h has the layout of the exposure block and the only definition of every count).
// Two launches in dmp_predict_end behind assign_ss, the entity (0 model, 1 native) as blockIdx.y of both.  The alignment's first
// row (a glycine has no side-chain atom), whether the native is whole (whole_x: no NaN x) and its rebuilt backbone come from the
// native entity (entity.hip), prepared in front of these launches:
//   exposure_surface      one workgroup per (residue, entity), thread k owns sphere point k of the residue's five atoms.
//                         Stage A: the threads scan all 5L atoms, 256 at a time, and compact those that can reach one of the
//                         five (centre distance below R_a + R_j + 0.01) into an LDS list of (x, y, z, R^2) doubles - wave
//                         ballots and a prefix give every candidate its slot.  Stage B, whenever the list holds a chunk and
//                         at the end: every wave walks the list in step (all lanes read the same entry: an LDS broadcast)
//                         until all of its points are buried.  The buried bits stay in registers across chunks, so where
//                         a chunk ends changes nothing.  The residue's own atoms are tested first, from their own slots:
//                         the list never holds the atom a point belongs to.  The five counts are popcounts of the waves'
//                         ballots; integer sums go thread 0 -> one integer atomic per workgroup and counter; the last
//                         arriver (ticket, as mapscore.hip and ss.hip) writes the header.
//   exposure_pairs        one thread per residue: the two half-sphere counts and the CB contact number over tiles of 256
//                         C-alpha / C-beta positions in LDS.
// No float atomics, no waiting between workgroups; the same bits on every run.  Contraction is off (score_common.h): float64
// from the float32 coordinates, every operation in the order the header writes it.
#include "score_common.h"

namespace dmp {

constexpr int EXP_THREADS = 256, EXP_WAVES = EXP_THREADS / 64;
constexpr int EXP_POINTS = 256;           // one per thread
constexpr int EXP_LIST = 1024;            // entries of the LDS list: 32 KiB, four workgroups to a CU
constexpr int EXP_PER = 7, EXP_COUNTERS = 2 * EXP_PER;   // per entity: atoms present, five sums, atoms with n = 0
constexpr int EXP_GLYCINE = 7;            // the residue code of G (dmp_msa_encode)
constexpr double EXP_MARGIN = 0.01;       // of the neighbour filter: far above any rounding of the point test
static_assert(EXP_POINTS == EXP_THREADS, "thread k owns point k");

__device__ const float exposure_points_dev[3 * EXP_POINTS] = {
#include "exposure_points.h"
};

// The scratch of a context, whatever its capacity: the head alone - the counters and the ticket (zero between launches).
struct ExpScratch { int64_t total; };
constexpr int64_t EXP_HEAD_BYTES = 256;
inline ExpScratch exposure_scratch(int) { return {EXP_HEAD_BYTES}; }
ScratchNeed exposure_need(int max_L) { return {exposure_scratch(max_L).total, EXP_HEAD_BYTES}; }

struct ExpArgs {
  const float* bb[2];         // [L][5][3] N, CA, C, O, CB of the model / of the native (the native entity's)
  const unsigned char* row;   // [L] the residue codes of the alignment's first row (the native entity's)
  const int* whole;           // the native entity's whole_x; read only where entities == 2
  float* out;                 // the exposure block, 32 + 16L floats
  int L, entities, chunk;     // chunk: entries of the list walked at a time (1 .. EXP_LIST)
  unsigned* cnt;              // [EXP_COUNTERS]
  unsigned* ticket;           // zero between launches
};

// atom radius + the 1.4 A probe (Kabsch & Sander 1983): N, CA, C, O, a side-chain atom
__device__ inline double exp_radius(int atom) {
  return atom == 0 ? 3.05 : (atom == 1 ? 3.27 : (atom == 2 ? 3.16 : (atom == 3 ? 2.80 : 3.20)));
}

// ---------------------------------------------------------------------------------------
// exposure_surface
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(EXP_THREADS) void exposure_surface_kernel(ExpArgs a) {
  __shared__ double list[EXP_LIST][4];       // x, y, z, R^2 of the candidates
  __shared__ double own[5][4];               // x, y, z, R of the residue's atoms
  __shared__ int own_ok[5];
  __shared__ int wave_tot[EXP_WAVES];
  __shared__ unsigned wave_bur[5][EXP_WAVES];
  const int L = a.L, own_res = blockIdx.x, e = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float nan = __builtin_nanf("");
  float* o = a.out + EXPOSURE_HEADER + (e ? 8 * (int64_t)L : 0);
  if (e == 0 && a.entities == 1 && tid < 5) a.out[EXPOSURE_HEADER + (8 + tid) * (int64_t)L + own_res] = nan;
  const bool skip = e == 1 && !*a.whole;                   // uniform
  if (skip) {
    if (tid < 5) o[tid * (int64_t)L + own_res] = nan;
  } else {
    const float* bb = a.bb[e];
    if (tid < 5) {
      const float* p = bb + 15 * (int64_t)own_res + 3 * tid;
      own[tid][0] = (double)p[0]; own[tid][1] = (double)p[1]; own[tid][2] = (double)p[2];
      own[tid][3] = exp_radius(tid);
      own_ok[tid] = !(tid == 4 && a.row[own_res] == EXP_GLYCINE);
    }
    __syncthreads();
    const double ux = (double)exposure_points_dev[3 * tid], uy = (double)exposure_points_dev[3 * tid + 1],
                 uz = (double)exposure_points_dev[3 * tid + 2];
    bool bur[5];
    // the residue's own atoms against each other
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      bur[k] = false;
      if (!own_ok[k]) continue;
      const double R = own[k][3];
      const double px = own[k][0] + R * ux, py = own[k][1] + R * uy, pz = own[k][2] + R * uz;
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        if (b == k || !own_ok[b]) continue;
        const double dx = px - own[b][0], dy = py - own[b][1], dz = pz - own[b][2], Rb = own[b][3];
        if ((dx * dx + dy * dy) + dz * dz < Rb * Rb) bur[k] = true;
      }
    }
    // Stage B over list[0, count): every wave in step, until all of its points of atom k are buried
    auto walk = [&](int count) {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (!own_ok[k]) continue;
        const double R = own[k][3];
        const double px = own[k][0] + R * ux, py = own[k][1] + R * uy, pz = own[k][2] + R * uz;
        bool b = bur[k];
        for (int t = 0; t < count; ++t) {
          if (__ballot(!b) == 0ull) break;
          const double dx = px - list[t][0], dy = py - list[t][1], dz = pz - list[t][2];
          if ((dx * dx + dy * dy) + dz * dz < list[t][3]) b = true;
        }
        bur[k] = b;
      }
    };
    // Stage A: all atoms of the other residues, 256 at a time
    const int chunk = a.chunk;
    int count = 0;
    for (int b0 = 0; b0 < 5 * L; b0 += EXP_THREADS) {
      const int g = b0 + tid, r = g / 5, at = g - 5 * r;
      bool cand = false;
      double cx = 0.0, cy = 0.0, cz = 0.0, Rj = 0.0;
      if (g < 5 * L && r != own_res && !(at == 4 && a.row[r] == EXP_GLYCINE)) {
        const float* p = bb + 3 * (int64_t)g;
        cx = (double)p[0]; cy = (double)p[1]; cz = (double)p[2];
        Rj = exp_radius(at);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const double dx = cx - own[k][0], dy = cy - own[k][1], dz = cz - own[k][2], reach = (own[k][3] + Rj) + EXP_MARGIN;
          if (own_ok[k] && (dx * dx + dy * dy) + dz * dz < reach * reach) cand = true;
        }
      }
      const unsigned long long m = __ballot(cand);
      if (lane == 0) wave_tot[wv] = __popcll(m);
      __syncthreads();
      int rank = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < EXP_WAVES; ++w) {
        if (w < wv) rank += wave_tot[w];
        total += wave_tot[w];
      }
      // the round's candidates go into the list in rank order, as many at a time as the chunk has room for (all uniform)
      int taken = 0;
      while (taken < total) {
        const int room = chunk - count, n = room < total - taken ? room : total - taken;
        if (cand && rank >= taken && rank < taken + n) {
          double* q = list[count + rank - taken];
          q[0] = cx; q[1] = cy; q[2] = cz; q[3] = Rj * Rj;
        }
        count += n;
        taken += n;
        __syncthreads();
        if (count == chunk) {
          walk(count);
          count = 0;
          __syncthreads();
        }
      }
      __syncthreads();                       // wave_tot is written again in the next round
    }
    if (count) walk(count);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned long long m = __ballot(bur[k]);
      if (lane == 0) wave_bur[k][wv] = (unsigned)__popcll(m);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (!skip) {
    unsigned present = 0u, zero = 0u, sums[5];
    for (int k = 0; k < 5; ++k) {
      unsigned buried = 0u;
      for (int w = 0; w < EXP_WAVES; ++w) buried += wave_bur[k][w];
      const unsigned n = EXP_POINTS - buried;
      sums[k] = own_ok[k] ? n : 0u;
      present += own_ok[k] ? 1u : 0u;
      zero += own_ok[k] && n == 0u ? 1u : 0u;
      o[k * (int64_t)L + own_res] = own_ok[k] ? (float)n : -1.f;
    }
    unsigned* cnt = a.cnt + EXP_PER * e;
    __hip_atomic_fetch_add(&cnt[0], present, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int k = 0; k < 5; ++k)
      if (sums[k]) __hip_atomic_fetch_add(&cnt[1 + k], sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (zero) __hip_atomic_fetch_add(&cnt[6], zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!ticket_take_last(a.ticket, gridDim.x * gridDim.y)) return;
  // the last arriver: the header (the native's counters are zero where its leg did not run)
  a.out[0] = (float)EXP_POINTS;
  for (int k = 0; k < EXP_COUNTERS; ++k) a.out[k < EXP_PER ? 1 + k : 2 + k] = (float)counter_drain(&a.cnt[k]);   // offsets 1 .. 7 and 9 .. 15
  a.out[8] = a.entities == 2 && *a.whole ? 1.f : 0.f;
  for (int k = 16; k < EXPOSURE_HEADER; ++k) a.out[k] = 0.f;
  ticket_reset(a.ticket);
}

// ---------------------------------------------------------------------------------------
// exposure_pairs
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(EXP_THREADS) void exposure_pairs_kernel(ExpArgs a) {
  __shared__ double ca[EXP_THREADS][3], cb[EXP_THREADS][3];
  const int L = a.L, e = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * EXP_THREADS + tid;
  const float nan = __builtin_nanf("");
  float* o = a.out + EXPOSURE_HEADER + (e ? 8 * (int64_t)L : 0) + 5 * (int64_t)L;
  if (e == 0 && a.entities == 1 && i < L)
    for (int k = 0; k < 3; ++k) a.out[EXPOSURE_HEADER + (13 + k) * (int64_t)L + i] = nan;
  if (e == 1 && !*a.whole) {                               // uniform
    if (i < L)
      for (int k = 0; k < 3; ++k) o[k * (int64_t)L + i] = nan;
    return;
  }
  const float* bb = a.bb[e];
  double ax = 0.0, ay = 0.0, az = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
  if (i < L) {
    const float* p = bb + 15 * (int64_t)i;
    ax = (double)p[3]; ay = (double)p[4]; az = (double)p[5];
    bx = (double)p[12]; by = (double)p[13]; bz = (double)p[14];
  }
  const double vx = bx - ax, vy = by - ay, vz = bz - az;
  unsigned up = 0u, down = 0u, cn = 0u;
  for (int j0 = 0; j0 < L; j0 += EXP_THREADS) {
    __syncthreads();
    if (j0 + tid < L) {
      const float* p = bb + 15 * (int64_t)(j0 + tid);
      ca[tid][0] = (double)p[3]; ca[tid][1] = (double)p[4]; ca[tid][2] = (double)p[5];
      cb[tid][0] = (double)p[12]; cb[tid][1] = (double)p[13]; cb[tid][2] = (double)p[14];
    }
    __syncthreads();
    if (i >= L) continue;
    const int n = L - j0 < EXP_THREADS ? L - j0 : EXP_THREADS;
    for (int t = 0; t < n; ++t) {
      if (j0 + t == i) continue;
      const double wx = ca[t][0] - ax, wy = ca[t][1] - ay, wz = ca[t][2] - az;
      if ((wx * wx + wy * wy) + wz * wz < 169.0) {
        if ((vx * wx + vy * wy) + vz * wz > 0.0) ++up;
        else ++down;
      }
      const double dx = cb[t][0] - bx, dy = cb[t][1] - by, dz = cb[t][2] - bz;
      if ((dx * dx + dy * dy) + dz * dz < 100.0) ++cn;
    }
  }
  if (i >= L) return;
  o[i] = (float)up;
  o[(int64_t)L + i] = (float)down;
  o[2 * (int64_t)L + i] = (float)cn;
}

int exposure(dmp_ctx* c, const float* d_coords, int L, const float* d_native, float* d_block, hipStream_t s) {
  const NativeEntity nat = native_entity(c);
  unsigned char* ws = c->exposure_ws.p;
  ExpArgs a{};
  a.bb[0] = d_coords;
  a.bb[1] = nat.bb;
  a.row = nat.row;
  a.whole = nat.whole_x;
  a.out = d_block;
  a.L = L;
  a.entities = d_native ? 2 : 1;
  a.chunk = c->run.exposure_chunk > 0 && c->run.exposure_chunk < EXP_LIST ? c->run.exposure_chunk : EXP_LIST;
  a.cnt = (unsigned*)ws;
  a.ticket = (unsigned*)ws + EXP_COUNTERS;
  hipLaunchKernelGGL(exposure_surface_kernel, dim3(L, a.entities), dim3(EXP_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(exposure_pairs_kernel, dim3(cdiv(L, EXP_THREADS), a.entities), dim3(EXP_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// the native's rebuilt backbone, the native entity's (dmp_debug_fetch "exposure_native_backbone")
const float* exposure_native_backbone(const dmp_ctx* c) { return native_entity(c).bb; }

// the table as the device holds it (dmp_debug_fetch "exposure_points"): read by a kernel, as the surface kernel reads it
__global__ void exposure_points_copy_kernel(float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * EXP_POINTS) dst[i] = exposure_points_dev[i];
}
int64_t exposure_points_fetch(float* d_dst, int64_t capacity, hipStream_t s) {
  const int64_t n = 3 * EXP_POINTS;
  if (n > capacity) { set_error("capacity %lld too small for exposure_points (%lld)", (long long)capacity, (long long)n); return DMP_ERR_ARG; }
  hipLaunchKernelGGL(exposure_points_copy_kernel, dim3(cdiv((int)n, 256)), dim3(256), 0, s, d_dst);
  DMP_LAUNCH_CHECK();
  return n;
}

}  // namespace dmp
