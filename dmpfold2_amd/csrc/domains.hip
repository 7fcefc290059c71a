// option "domains": the final C-alpha trace, and the native's where option "score_native" holds a whole native trace, split
// into structural domains by recursive contact-density bisection (include/dmpfold_hip.h has the layout of the domain block
// and the only definition of every count and of the choice of a cut).  Everything behind the contact test is integer
// arithmetic; nothing waits between workgroups and nothing is read back by the host between the levels: the launches of one
// prediction are stream-ordered and the same whatever the trace holds.  The entity (0 model, 1 native) is the last grid
// dimension of every launch; a native leg that is absent returns at once.  Whether the native is whole (whole_xyz: no NaN
// coordinate) comes from the native entity (entity.hip), prepared in front of these launches; its C-alpha are read from the
// score block itself.
//
// A residue carries the node of a binary tree: 1 the chain, 2k and 2k + 1 the parts A and B of node k.  Level v examines the
// nodes 2^v .. 2^(v+1) - 1, one per slot; a domain that was not split keeps a node below 2^(v+1) and is met by no later slot.
//   domains_prep     one workgroup per entity: every node = 1, the counters zero
//   domains_contacts the L x L contact table as bytes, and the chain's contact pairs (one integer atomic per workgroup)
// per level v = 0 .. 3, the slot as blockIdx.y:
//   domains_compact  one workgroup per slot: the sizes of the level's domains (LDS histogram), the slot's place in the lists
//                    and in the table area, its residues compacted in ascending order by ballot prefix sums
//   domains_rows     one wave per row of the slot's summed-area table: the row's prefix sums by wave scans of 64
//   domains_cols     one thread per column: the running sum down the rows (coalesced across the threads)
//   domains_cuts     one workgroup per I: every admissible J from five table reads, reduced to the row's best cut by the
//                    int64 cross-multiplied comparison with the (I, J) tie-break
//   domains_split    one workgroup per slot: the best of the rows, the tau rule, the children's nodes
// then
//   domains_count    one workgroup per residue: its contacts inside and outside its domain (two integer atomics)
//   domains_final    one workgroup per entity: the domains numbered by their lowest residue, labels, table, header
// 24 launches.  No float atomics: the same bits on every run.  Contraction is off (score_common.h).
#include "score_common.h"

namespace dmp {

constexpr int DOM_THREADS = 256, DOM_WAVES = DOM_THREADS / 64;
constexpr int DOM_LEVELS = 4, DOM_MAX = 1 << DOM_LEVELS, DOM_NODES = 2 * DOM_MAX;
constexpr int DOM_HEAD_INTS = 256;        // [2 + e] contact pairs, [16 + 2 (32 e + node) + k] inside / outside
constexpr int64_t DOM_HEAD_BYTES = 4 * DOM_HEAD_INTS;
static_assert(DOMAINS_HEADER == 32 && DOMAINS_ROW == 8 && DOMAINS_MAX == DOM_MAX, "the block of include/dmpfold_hip.h");

struct DomSlot { int n, start, live, pad; long long sat; long long pad2; };      // 32 bytes
struct DomCut { int ext, den, I, J; };                                           // den = 0: none

// The scratch of a context of capacity `cap` (bytes from its start, every part 16-aligned): the head | per entity the
// nodes, the compacted lists, the slots, the cuts that made the nodes, the rows' best cuts, the contact table, the
// summed-area tables of one level - (n_s + 1)^2 int32 per slot, together at most (cap + 16)^2.
struct DomScratch { int64_t node, idx, slot, made, part, con, sat, total; };
inline DomScratch domains_scratch(int cap) {
  auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  const int64_t c = cap;
  DomScratch s;
  s.node = DOM_HEAD_BYTES;
  s.idx = s.node + up(2 * 4 * c);
  s.slot = s.idx + up(2 * 4 * c);
  s.made = s.slot + 2 * DOM_MAX * (int64_t)sizeof(DomSlot);
  s.part = s.made + 2 * DOM_NODES * 8;
  s.con = s.part + 2 * 16 * c;
  s.sat = s.con + up(2 * c * c);
  s.total = s.sat + 2 * 4 * (c + 16) * (c + 16);
  return s;
}
ScratchNeed domains_need(int max_L) { return {domains_scratch(max_L).total, DOM_HEAD_BYTES}; }
static_assert(sizeof(DomSlot) == 32 && sizeof(DomCut) == 16, "the scratch is carved in these sizes");

struct DomArgs {
  const float* xyz[2];        // the first C-alpha of the model / of the native ...
  int pitch[2];               // ... and the floats from one residue's to the next's
  const int* whole;           // the native entity's whole_xyz; read only where entities == 2
  float* out;                 // the domain block, 32 + 2L + 256 floats
  int L, entities, tau_milli, min_size, min_segment;
  int* head;                  // [DOM_HEAD_INTS]
  int* node;                  // [2][L]
  int* idx;                   // [2][L]: the lists of a level's slots, slot s at its `start`
  DomSlot* slot;              // [2][16]
  int* made;                  // [2][32][2]: ext and denominator of the cut that made a node
  DomCut* part;               // [2][L]: the best cut of row I of slot s at start + I
  unsigned char* con;         // [2][L][L]
  int* sat;                   // [2][(L + 16)^2]
};

__device__ inline bool dom_active(const DomArgs& a, int e) { return e == 0 || (a.entities == 2 && *a.whole != 0); }
__device__ inline int64_t dom_sat_pitch(int L) { return (int64_t)(L + 16) * (L + 16); }

// a is the better cut: the smaller ext / den, exactly; of equal ones the smaller (I, J).  Every product is below 2^44.
__device__ inline bool dom_better(const DomCut& a, const DomCut& b) {
  if (a.den == 0) return false;
  if (b.den == 0) return true;
  const long long l = (long long)a.ext * b.den, r = (long long)b.ext * a.den;
  if (l != r) return l < r;
  return a.I != b.I ? a.I < b.I : a.J < b.J;
}
// the best cut of the workgroup, in every thread (`wbest`: DOM_WAVES entries of LDS)
__device__ inline DomCut dom_block_best(DomCut c, DomCut* wbest) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    DomCut o;
    o.ext = __shfl_xor(c.ext, off, 64); o.den = __shfl_xor(c.den, off, 64);
    o.I = __shfl_xor(c.I, off, 64); o.J = __shfl_xor(c.J, off, 64);
    if (dom_better(o, c)) c = o;
  }
  __syncthreads();
  if (lane == 0) wbest[wv] = c;
  __syncthreads();
  c = wbest[0];
#pragma unroll
  for (int w = 1; w < DOM_WAVES; ++w)
    if (dom_better(wbest[w], c)) c = wbest[w];
  return c;
}
// the sum of two counts over the workgroup, in thread 0 (`wsum`: 2 DOM_WAVES ints of LDS)
__device__ inline void dom_block_sum2(int& u, int& v, int* wsum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) { u += __shfl_xor(u, off, 64); v += __shfl_xor(v, off, 64); }
  if (lane == 0) { wsum[2 * wv] = u; wsum[2 * wv + 1] = v; }
  __syncthreads();
  if (threadIdx.x == 0) {
    u = 0; v = 0;
    for (int w = 0; w < DOM_WAVES; ++w) { u += wsum[2 * w]; v += wsum[2 * w + 1]; }
  }
}

__global__ __launch_bounds__(DOM_THREADS) void domains_prep_kernel(DomArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x, L = a.L;
  for (int k = tid; k < L; k += DOM_THREADS) a.node[(int64_t)e * L + k] = 1;
  if (tid == 0) a.head[2 + e] = 0;
  if (tid < 2 * DOM_NODES) {
    a.head[16 + 2 * DOM_NODES * e + tid] = 0;
    a.made[2 * DOM_NODES * e + tid] = 0;
  }
}

__global__ __launch_bounds__(DOM_THREADS) void domains_contacts_kernel(DomArgs a) {
  __shared__ int pairs;
  const int e = blockIdx.z, i = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * DOM_THREADS + tid, L = a.L;
  if (!dom_active(a, e)) return;                          // uniform
  if (tid == 0) pairs = 0;
  __syncthreads();
  bool c = false;
  if (j < L) {
    const int sep = i > j ? i - j : j - i;
    if (sep >= 3) {
      const float* p = a.xyz[e] + (int64_t)a.pitch[e] * i;
      const float* q = a.xyz[e] + (int64_t)a.pitch[e] * j;
      const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
      c = (dx * dx + dy * dy) + dz * dz < 100.0;
    }
    a.con[((int64_t)e * L + i) * L + j] = c ? 1 : 0;
  }
  const unsigned long long m = __ballot(c && j > i);
  if ((tid & 63) == 0 && m) atomicAdd(&pairs, __popcll(m));
  __syncthreads();
  if (tid == 0 && pairs) atomicAdd(&a.head[2 + e], pairs);
}

__global__ __launch_bounds__(DOM_THREADS) void domains_compact_kernel(DomArgs a, int level) {
  __shared__ int cnt[DOM_MAX];
  __shared__ int wave_tot[DOM_WAVES];
  const int e = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, L = a.L, base = 1 << level;
  if (!dom_active(a, e)) return;                          // uniform
  const int* node = a.node + (int64_t)e * L;
  if (tid < DOM_MAX) cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < L; i += DOM_THREADS) {
    const int t = node[i] - base;
    if (t >= 0 && t < base) atomicAdd(&cnt[t], 1);
  }
  __syncthreads();
  int start = 0;
  long long sat = 0;
  for (int t = 0; t < s; ++t) {
    start += cnt[t];
    sat += (long long)(cnt[t] + 1) * (cnt[t] + 1);
  }
  const int n = cnt[s], live = n >= 2 * a.min_size ? 1 : 0;
  if (tid == 0) a.slot[e * DOM_MAX + s] = DomSlot{n, start, live, 0, sat, 0};
  if (!live) return;                                      // uniform
  int* idx = a.idx + (int64_t)e * L + start;
  int done = 0;
  for (int i0 = 0; i0 < L; i0 += DOM_THREADS) {
    const int i = i0 + tid;
    const bool mine = i < L && node[i] == base + s;
    const unsigned long long m = __ballot(mine);
    if (lane == 0) wave_tot[wv] = __popcll(m);
    __syncthreads();
    int rank = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < DOM_WAVES; ++w) {
      if (w < wv) rank += wave_tot[w];
      total += wave_tot[w];
    }
    if (mine) idx[done + rank] = i;                       // done + rank < n: the ranks of the slot's n residues
    done += total;
    __syncthreads();                                      // wave_tot is written again in the next round
  }
}

// Row r of the slot's table (n + 1 columns): row 0 is zero, row r >= 1 the prefix sums of the contacts of list position r - 1.
__global__ __launch_bounds__(DOM_THREADS) void domains_rows_kernel(DomArgs a) {
  const int e = blockIdx.z, s = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * DOM_WAVES + (threadIdx.x >> 6), L = a.L;
  if (!dom_active(a, e)) return;
  const DomSlot sl = a.slot[e * DOM_MAX + s];
  if (!sl.live || r > sl.n) return;                       // uniform in the wave; no barrier below
  const int n = sl.n;
  int* row = a.sat + e * dom_sat_pitch(L) + sl.sat + (int64_t)r * (n + 1);
  if (r == 0) {
    for (int q = lane; q <= n; q += 64) row[q] = 0;
    return;
  }
  const int* idx = a.idx + (int64_t)e * L + sl.start;
  const unsigned char* crow = a.con + ((int64_t)e * L + idx[r - 1]) * L;
  if (lane == 0) row[0] = 0;
  int carry = 0;
  for (int q0 = 0; q0 < n; q0 += 64) {
    const int q = q0 + lane;
    int v = q < n ? (int)crow[idx[q]] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(v, off, 64);
      if (lane >= off) v += t;
    }
    v += carry;
    if (q < n) row[q + 1] = v;
    carry = __shfl(v, 63, 64);
  }
}

__global__ __launch_bounds__(DOM_THREADS) void domains_cols_kernel(DomArgs a) {
  const int e = blockIdx.z, s = blockIdx.y, q = blockIdx.x * DOM_THREADS + threadIdx.x, L = a.L;
  if (!dom_active(a, e)) return;
  const DomSlot sl = a.slot[e * DOM_MAX + s];
  if (!sl.live || q > sl.n) return;
  const int n = sl.n;
  const int64_t W = n + 1;
  int* col = a.sat + e * dom_sat_pitch(L) + sl.sat + q;
  int acc = 0, r = 0;
  for (; r + 4 <= n + 1; r += 4) {                        // the four loads do not wait for the sum
    const int v0 = col[r * W], v1 = col[(r + 1) * W], v2 = col[(r + 2) * W], v3 = col[(r + 3) * W];
    acc += v0; col[r * W] = acc;
    acc += v1; col[(r + 1) * W] = acc;
    acc += v2; col[(r + 2) * W] = acc;
    acc += v3; col[(r + 3) * W] = acc;
  }
  for (; r <= n; ++r) {
    acc += col[r * W];
    col[r * W] = acc;
  }
}

__global__ __launch_bounds__(DOM_THREADS) void domains_cuts_kernel(DomArgs a) {
  __shared__ DomCut wbest[DOM_WAVES];
  const int e = blockIdx.z, s = blockIdx.y, I = blockIdx.x, tid = threadIdx.x, L = a.L;
  if (!dom_active(a, e)) return;
  const DomSlot sl = a.slot[e * DOM_MAX + s];
  if (!sl.live || I >= sl.n) return;                      // uniform
  const int n = sl.n;
  const int64_t W = n + 1;
  DomCut best{0, 0, I, 0};
  if (I == 0 || I >= a.min_segment) {                     // uniform
    const int* S = a.sat + e * dom_sat_pitch(L) + sl.sat;
    const int T = S[n * W + n] / 2, SII = S[I * W + I], SIn = S[I * W + n];
    for (int J = I + 1 + tid; J <= n; J += DOM_THREADS) {
      const int size = J - I;
      if (size < a.min_size || n - size < a.min_size || !(J == n || n - J >= a.min_segment)) continue;
      const int full_a = S[J * W + J] - 2 * S[I * W + J] + SII;          // both orders of every pair inside A
      const int ext = (S[J * W + n] - SIn) - full_a;
      const int int_a = full_a / 2, int_b = T - int_a - ext;
      const int least = int_a < int_b ? int_a : int_b;
      if (least <= 0) continue;
      const DomCut c{ext, least + ext, I, J};
      if (dom_better(c, best)) best = c;
    }
  }
  best = dom_block_best(best, wbest);
  if (tid == 0) a.part[(int64_t)e * L + sl.start + I] = best;
}

__global__ __launch_bounds__(DOM_THREADS) void domains_split_kernel(DomArgs a, int level) {
  __shared__ DomCut wbest[DOM_WAVES];
  const int e = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, L = a.L;
  if (!dom_active(a, e)) return;
  const DomSlot sl = a.slot[e * DOM_MAX + s];
  if (!sl.live) return;                                   // uniform
  const int n = sl.n, k = (1 << level) + s;
  const DomCut* part = a.part + (int64_t)e * L + sl.start;
  DomCut best{0, 0, 0, 0};
  for (int I = tid; I < n; I += DOM_THREADS) {
    const DomCut c = part[I];
    if (dom_better(c, best)) best = c;
  }
  best = dom_block_best(best, wbest);
  if (best.den == 0 || !((long long)best.ext * 1000 < (long long)a.tau_milli * best.den)) return;     // uniform
  const int* idx = a.idx + (int64_t)e * L + sl.start;
  int* node = a.node + (int64_t)e * L;
  for (int p = tid; p < n; p += DOM_THREADS) node[idx[p]] = 2 * k + (p >= best.I && p < best.J ? 0 : 1);
  if (tid < 4) a.made[2 * (DOM_NODES * e + 2 * k) + tid] = tid & 1 ? best.den : best.ext;     // of nodes 2k and 2k + 1
}

__global__ __launch_bounds__(DOM_THREADS) void domains_count_kernel(DomArgs a) {
  __shared__ int wsum[2 * DOM_WAVES];
  const int e = blockIdx.y, i = blockIdx.x, tid = threadIdx.x, L = a.L;
  if (!dom_active(a, e)) return;
  const int* node = a.node + (int64_t)e * L;
  const unsigned char* crow = a.con + ((int64_t)e * L + i) * L;
  const int k = node[i];
  int same = 0, other = 0;
  for (int j = tid; j < L; j += DOM_THREADS)
    if (crow[j]) {
      if (node[j] == k) ++same;
      else ++other;
    }
  dom_block_sum2(same, other, wsum);
  if (tid == 0) {
    int* cnt = a.head + 16 + 2 * (DOM_NODES * e + k);
    if (same) atomicAdd(&cnt[0], same);                   // both ends of a pair inside: twice the pairs
    if (other) atomicAdd(&cnt[1], other);
  }
}

__global__ __launch_bounds__(DOM_THREADS) void domains_final_kernel(DomArgs a) {
  __shared__ int cnt[DOM_NODES], low[DOM_NODES], seg[DOM_NODES], label[DOM_NODES];
  const int e = blockIdx.x, tid = threadIdx.x, L = a.L;
  float* hdr = a.out + 16 * e;
  float* lab = a.out + DOMAINS_HEADER + (int64_t)e * L;
  float* tab = a.out + DOMAINS_HEADER + 2 * (int64_t)L + DOM_MAX * DOMAINS_ROW * e;
  if (!dom_active(a, e)) {                                // uniform: no native leg
    const float nan = __builtin_nanf("");
    if (tid < 16) hdr[tid] = 0.f;
    for (int i = tid; i < L; i += DOM_THREADS) lab[i] = nan;
    if (tid < DOM_MAX * DOMAINS_ROW) tab[tid] = 0.f;
    return;
  }
  const int* node = a.node + (int64_t)e * L;
  if (tid < DOM_NODES) { cnt[tid] = 0; low[tid] = INT32_MAX; seg[tid] = 0; }
  __syncthreads();
  for (int i = tid; i < L; i += DOM_THREADS) {
    const int k = node[i];
    atomicAdd(&cnt[k], 1);
    atomicMin(&low[k], i);
    if (i == 0 || node[i - 1] != k) atomicAdd(&seg[k], 1);
  }
  __syncthreads();
  if (tid < DOM_NODES) {
    int before = 0;
    for (int t = 1; t < DOM_NODES; ++t) before += cnt[t] > 0 && low[t] < low[tid] ? 1 : 0;
    label[tid] = cnt[tid] > 0 ? before : -1;
  }
  __syncthreads();
  for (int i = tid; i < L; i += DOM_THREADS) lab[i] = (float)label[node[i]];
  if (tid < DOM_MAX) {                                    // row `tid` of the table: the domain of that label, or zeros
    int k = 0;
    for (int t = 1; t < DOM_NODES; ++t)
      if (label[t] == tid) k = t;
    float* row = tab + DOMAINS_ROW * tid;
    const int* c = a.head + 16 + 2 * (DOM_NODES * e + k);
    const int* made = a.made + 2 * (DOM_NODES * e + k);
    row[0] = k ? (float)cnt[k] : 0.f;
    row[1] = k ? (float)seg[k] : 0.f;
    row[2] = k ? (float)low[k] : 0.f;
    row[3] = k ? (float)(c[0] / 2) : 0.f;
    row[4] = k ? (float)c[1] : 0.f;
    row[5] = k ? (float)made[0] : 0.f;
    row[6] = k ? (float)made[1] : 0.f;
    row[7] = k ? (float)(31 - __clz(k)) : 0.f;
  }
  if (tid != 0) return;
  int domains = 0, several = 0, deepest = 0, large = 0;
  for (int t = 1; t < DOM_NODES; ++t) {
    if (cnt[t] == 0) continue;
    ++domains;
    several += seg[t] > 1 ? 1 : 0;
    const int level = 31 - __clz(t);
    deepest = level > deepest ? level : deepest;
    large |= t >= DOM_MAX && cnt[t] >= 2 * a.min_size ? 1 : 0;
  }
  hdr[0] = (float)domains;
  hdr[1] = (float)a.head[2 + e];
  hdr[2] = (float)a.tau_milli;
  hdr[3] = (float)a.min_size;
  hdr[4] = (float)a.min_segment;
  hdr[5] = (float)several;
  hdr[6] = (float)deepest;
  hdr[7] = (float)large;
  for (int t = 8; t < 16; ++t) hdr[t] = 0.f;
}

int domains(dmp_ctx* c, const float* d_coords, int L, const float* d_native, float* d_block, hipStream_t s) {
  const DomScratch sc = domains_scratch(c->max_L);
  unsigned char* ws = c->domains_ws.p;
  DomArgs a{};
  a.xyz[0] = d_coords + 3;            // the C-alpha of [L][5][3] N, CA, C, O, CB
  a.pitch[0] = 15;
  a.xyz[1] = d_native;                // the score block's native trace [L][3], or null
  a.pitch[1] = 3;
  a.whole = native_entity(c).whole_xyz;
  a.out = d_block;
  a.L = L;
  a.entities = d_native ? 2 : 1;
  a.tau_milli = c->run.dom_tau;
  a.min_size = c->run.dom_min_size;
  a.min_segment = c->run.dom_min_segment;
  a.head = (int*)ws;
  a.node = (int*)(ws + sc.node);
  a.idx = (int*)(ws + sc.idx);
  a.slot = (DomSlot*)(ws + sc.slot);
  a.made = (int*)(ws + sc.made);
  a.part = (DomCut*)(ws + sc.part);
  a.con = ws + sc.con;
  a.sat = (int*)(ws + sc.sat);
  const unsigned E = (unsigned)a.entities;
  const dim3 T(DOM_THREADS);
  hipLaunchKernelGGL(domains_prep_kernel, dim3(2), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domains_contacts_kernel, dim3(cdiv(L, DOM_THREADS), L, E), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  for (int level = 0; level < DOM_LEVELS; ++level) {
    const unsigned slots = 1u << level;
    hipLaunchKernelGGL(domains_compact_kernel, dim3(slots, E), T, 0, s, a, level);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(domains_rows_kernel, dim3(cdiv(L + 1, DOM_WAVES), slots, E), T, 0, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(domains_cols_kernel, dim3(cdiv(L + 1, DOM_THREADS), slots, E), T, 0, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(domains_cuts_kernel, dim3(L, slots, E), T, 0, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(domains_split_kernel, dim3(slots, E), T, 0, s, a, level);
    DMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(domains_count_kernel, dim3(L, E), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domains_final_kernel, dim3(2), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
