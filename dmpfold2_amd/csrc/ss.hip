// option "assign_ss": secondary structure of the final backbone, and of the native's where option "score_native" holds a
// whole native trace (include/dmpfold_hip.h has the layout of the SS block and the only definition of every predicate).
// Three launches in dmp_predict_end behind score_passes, the entity (0 model, 1 native) as blockIdx.y of the first two.  The
// alignment's first row, whether the native is whole (whole_x: no NaN x) and its rebuilt backbone come from the native entity
// (entity.hip), prepared in front of these launches:
//   ss_prep         the amide hydrogens and the donor flags (no donor where the first row has a proline) in float64
//   ss_hbond        one workgroup per (residue, entity, side).  Side 0: residue i accepts - the energies E(i, j) over j, their
//                   minimum with its partner, row i of the bit matrix R (bit j = hb(i, j)).  Side 1: residue j donates - the
//                   same function over i, the column's minimum, row j of the transposed matrix T (bit i = hb(i, j)).  Every
//                   energy is evaluated twice by the same device function (the same bits) so that both matrices are written
//                   by rows: a wave's ballot is two words, stored by its first lane.  The minimum of (E, index) pairs is
//                   order-free.
//   ss_assign       one thread per residue, both entities in turn.  With R and T every look-up of the definition reads a row
//                   within two of the thread's own.  The turn and helix flags of the workgroup's residues and a halo of 16
//                   go through LDS (t3 t4 t5 -> Hf -> Gf -> If); the bridges are found from the set bits of rows i - 1 and i of
//                   R alone (each of the four disjuncts of P and A needs one of them).  Integer counts go thread -> LDS -> one
//                   integer atomic per workgroup and counter; the last arriver (ticket, as mapscore.hip) writes the header.
// No float atomics; the same bits on every run.  Contraction is off (score_common.h): float64 from the float32 coordinates,
// every operation in the order the header writes it.
#include "score_common.h"

namespace dmp {

constexpr int SS_THREADS = 256;
constexpr int SS_HALO = 16, SS_WIN = SS_THREADS + 2 * SS_HALO;
// counters of the context (unsigned, zero between launches)
constexpr int SS_CNT_HB = 0, SS_CNT_CODE = 1, SS_CNT_PAR = 9, SS_CNT_ANTI = 10, SS_CNT_Q3 = 11, SS_CNT_Q8 = 12, SS_CNT_NAT = 13,
              SS_COUNTERS = 21;
constexpr int SS_PROLINE = 14;         // the residue code of P (dmp_msa_encode)

// The scratch of a context of capacity `cap` (bytes from its start, every part 16-aligned).  head: the counters and the ticket
// (zero between launches); then per entity the hydrogens, the donor flags and the two bit matrices (rows of 2 ceil(cap / 64)
// words).
struct SsScratch { int64_t h[2], donor[2], R[2], T[2], total; };
__host__ __device__ inline int ss_row_words(int L) { return 2 * ((L + 63) / 64); }
constexpr int64_t SS_HEAD_BYTES = 256;
inline SsScratch ss_scratch(int cap) {
  auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  SsScratch s;
  int64_t at = SS_HEAD_BYTES;
  for (int e = 0; e < 2; ++e) {
    s.h[e] = at; at += up(24 * (int64_t)cap);
    s.donor[e] = at; at += up(cap);
    s.R[e] = at; at += up(4 * (int64_t)cap * ss_row_words(cap));
    s.T[e] = at; at += up(4 * (int64_t)cap * ss_row_words(cap));
  }
  s.total = at;
  return s;
}
ScratchNeed assign_ss_need(int max_L) { return {ss_scratch(max_L).total, SS_HEAD_BYTES}; }

struct SsEntity {
  const float* bb;         // [L][5][3] N, CA, C, O, CB
  double* h;               // [L][3] amide hydrogens (rows of donors only)
  unsigned char* donor;    // [L]
  unsigned* R;             // [L][words] bit j of row i = hb(i, j)
  unsigned* T;             // [L][words] bit i of row j = hb(i, j)
};
struct SsArgs {
  SsEntity ent[2];
  const unsigned char* row;   // [L] the residue codes of the alignment's first row (the native entity's)
  const int* whole;           // the native entity's whole_x; read only where entities == 2
  float* out;                 // the SS block, 32 + 8L floats
  int L, words, entities;
  unsigned* cnt;              // [SS_COUNTERS]
  unsigned* ticket;           // zero between launches
};

__device__ inline void ss_atom(const float* bb, int i, int atom, double* p) {
  const float* a = bb + 15 * (int64_t)i + 3 * atom;
  p[0] = (double)a[0]; p[1] = (double)a[1]; p[2] = (double)a[2];
}
__device__ inline double ss_dist(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}
// E(i, j): the C=O of i (c, o) accepts the N-H of j (n, h)
__device__ inline double ss_energy(const double* c, const double* o, const double* n, const double* h) {
  const double don = ss_dist(o, n), dch = ss_dist(c, h), doh = ss_dist(o, h), dcn = ss_dist(c, n);
  if (don < 0.5 || dch < 0.5 || doh < 0.5 || dcn < 0.5) return -9.9;
  const double e = 27.888 * (((1.0 / don + 1.0 / dch) - 1.0 / doh) - 1.0 / dcn);
  return e < -9.9 ? -9.9 : e;
}

// ---------------------------------------------------------------------------------------
// ss_prep
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void ss_prep_kernel(SsArgs a) {
  const int L = a.L, e = blockIdx.y, i = blockIdx.x * SS_THREADS + threadIdx.x;
  const SsEntity& en = a.ent[e];
  if (i >= L) return;
  bool donor = false;
  double h[3] = {0.0, 0.0, 0.0};
  if (i >= 1) {
    double c[3], o[3], n[3];
    ss_atom(en.bb, i - 1, 2, c);
    ss_atom(en.bb, i - 1, 3, o);
    ss_atom(en.bb, i, 0, n);
    const double vx = c[0] - o[0], vy = c[1] - o[1], vz = c[2] - o[2];
    const double vv = (vx * vx + vy * vy) + vz * vz;
    donor = a.row[i] != SS_PROLINE && vv > 0.0;
    if (donor) {
      const double s = sqrt(vv);
      h[0] = n[0] + vx / s; h[1] = n[1] + vy / s; h[2] = n[2] + vz / s;
    }
  }
  en.donor[i] = donor ? 1 : 0;
  en.h[3 * i] = h[0]; en.h[3 * i + 1] = h[1]; en.h[3 * i + 2] = h[2];
}

// ---------------------------------------------------------------------------------------
// ss_hbond
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void ss_hbond_kernel(SsArgs a) {
  __shared__ double red_e[SS_THREADS / 64];
  __shared__ int red_p[SS_THREADS / 64];
  const int L = a.L, own = blockIdx.x, e = blockIdx.y, side = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (e == 1 && !*a.whole) return;            // uniform
  const SsEntity& en = a.ent[e];
  // side 0: `own` accepts (its C, O); side 1: `own` donates (its N, H)
  double p0[3], p1[3];
  ss_atom(en.bb, own, side == 0 ? 2 : 0, p0);
  if (side == 0) ss_atom(en.bb, own, 3, p1);
  else { p1[0] = en.h[3 * own]; p1[1] = en.h[3 * own + 1]; p1[2] = en.h[3 * own + 2]; }
  const bool own_ok = side == 0 || en.donor[own] != 0;
  unsigned* row = (side == 0 ? en.R : en.T) + (int64_t)own * a.words;
  double best = 0.0;
  int partner = -1;
  for (int b0 = 0; b0 < L; b0 += SS_THREADS) {
    const int b = b0 + tid;                        // ascending per thread: the strict '<' keeps the lower of equals
    bool bond = false;
    if (b < L && own_ok && (b - own >= 2 || own - b >= 2) && (side == 1 || en.donor[b] != 0)) {
      double q0[3], q1[3], E;
      if (side == 0) {
        ss_atom(en.bb, b, 0, q0);
        q1[0] = en.h[3 * b]; q1[1] = en.h[3 * b + 1]; q1[2] = en.h[3 * b + 2];
        E = ss_energy(p0, p1, q0, q1);
      } else {
        ss_atom(en.bb, b, 2, q0);
        ss_atom(en.bb, b, 3, q1);
        E = ss_energy(q0, q1, p0, p1);
      }
      bond = E < -0.5;
      if (partner < 0 || E < best) { best = E; partner = b; }
    }
    const unsigned long long m = __ballot(bond);
    const int wb = b0 + wv * 64;                   // the wave's first bit; every word of the row is written by one wave
    if (lane == 0 && (wb >> 5) < a.words) {
      row[wb >> 5] = (unsigned)m;
      row[(wb >> 5) + 1] = (unsigned)(m >> 32);
    }
  }
  if (e != 0) return;                              // the native's energies are not handed out
  // the minimum of (E, index) pairs, an absent one behind every present one
  for (int off = 32; off > 0; off >>= 1) {
    const double oe = __shfl_xor(best, off, 64);
    const int op = __shfl_xor(partner, off, 64);
    if (op >= 0 && (partner < 0 || oe < best || (oe == best && op < partner))) { best = oe; partner = op; }
  }
  if (lane == 0) { red_e[wv] = best; red_p[wv] = partner; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < SS_THREADS / 64; ++k) {
      const double oe = red_e[k];
      const int op = red_p[k];
      if (op >= 0 && (partner < 0 || oe < best || (oe == best && op < partner))) { best = oe; partner = op; }
    }
    float* o = a.out + 32 + (side == 0 ? L : 3 * L);
    o[own] = partner < 0 ? 0.f : (float)best;
    o[L + own] = (float)partner;
  }
}

// ---------------------------------------------------------------------------------------
// ss_assign
// ---------------------------------------------------------------------------------------
struct SsBits {
  const unsigned* R;
  const unsigned* T;
  int L, words;
  // hb(i, j) read from row i of R / from row j of T; false where an index is outside [0, L)
  __device__ bool r(int i, int j) const {
    if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L) return false;
    return (R[(int64_t)i * words + (j >> 5)] >> (j & 31)) & 1u;
  }
  __device__ bool t(int i, int j) const {
    if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L) return false;
    return (T[(int64_t)j * words + (i >> 5)] >> (i & 31)) & 1u;
  }
  __device__ unsigned rword(int i, int w) const {
    return (unsigned)i < (unsigned)L && (unsigned)w < (unsigned)words ? R[(int64_t)i * words + w] : 0u;
  }
  __device__ bool domain(int x, int y) const { return x >= 1 && y >= 1 && x <= L - 2 && y <= L - 2 && (x - y >= 3 || y - x >= 3); }
  // the bridges of (x, y): rows x - 1, x of R and rows x, x + 1 of T
  __device__ bool par(int x, int y) const {
    return domain(x, y) && ((r(x - 1, y) && t(y, x + 1)) || (t(y - 1, x) && r(x, y + 1)));
  }
  __device__ bool anti(int x, int y) const {
    return domain(x, y) && ((r(x, y) && t(y, x)) || (r(x - 1, y + 1) && t(y - 1, x + 1)));
  }
};

__device__ inline int ss_three(int code) { return (code == 7 || code == 4 || code == 3) ? 2 : ((code == 6 || code == 5) ? 1 : 0); }

__global__ __launch_bounds__(SS_THREADS) void ss_assign_kernel(SsArgs a) {
  __shared__ unsigned char t3[SS_WIN], t4[SS_WIN], t5[SS_WIN], hf[SS_WIN], gf[SS_WIN];
  __shared__ unsigned icnt[SS_COUNTERS];
  const int L = a.L, tid = threadIdx.x, r0 = blockIdx.x * SS_THREADS, i = r0 + tid, w0 = r0 - SS_HALO;
  const bool native = a.entities == 2 && *a.whole != 0;
  if (tid < SS_COUNTERS) icnt[tid] = 0u;
  // a flag of residue x from the window, 0 outside it
  auto at = [&](const unsigned char* f, int x) -> bool { return x >= w0 && x < w0 + SS_WIN && f[x - w0] != 0; };
  int code0 = 0;
  const float nan = __builtin_nanf("");
  for (int e = 0; e < (native ? 2 : 1); ++e) {
    const SsEntity& en = a.ent[e];
    const SsBits m{en.R, en.T, L, a.words};
    __syncthreads();
    for (int x = tid; x < SS_WIN; x += SS_THREADS) {
      const int k = w0 + x;
      t3[x] = m.r(k, k + 3); t4[x] = m.r(k, k + 4); t5[x] = m.r(k, k + 5);
    }
    __syncthreads();
    for (int x = tid; x < SS_WIN; x += SS_THREADS) {
      const int k = w0 + x;
      bool f = false;
      for (int s = (k - 3 > 1 ? k - 3 : 1); s <= k && s <= L - 5; ++s) f = f || (at(t4, s - 1) && at(t4, s));
      hf[x] = f;
    }
    __syncthreads();
    for (int x = tid; x < SS_WIN; x += SS_THREADS) {
      const int k = w0 + x;
      bool f = false;
      for (int s = (k - 2 > 1 ? k - 2 : 1); s <= k && s <= L - 4; ++s)
        f = f || (at(t3, s - 1) && at(t3, s) && !at(hf, s) && !at(hf, s + 1) && !at(hf, s + 2));
      gf[x] = f;
    }
    __syncthreads();
    if (i >= L) continue;
    bool If = false, Tf = false, Sf = false, Ef = false;
    for (int s = (i - 4 > 1 ? i - 4 : 1); s <= i && s <= L - 6; ++s) {
      bool free5 = at(t5, s - 1) && at(t5, s);
      for (int k = s; k <= s + 4; ++k) free5 = free5 && !at(hf, k) && !at(gf, k);
      If = If || free5;
    }
    for (int s = 1; s <= 4; ++s)
      Tf = Tf || (s <= 2 && at(t3, i - s)) || (s <= 3 && at(t4, i - s)) || at(t5, i - s);
    if (i >= 2 && i <= L - 3) {
      double p[3], c[3], n[3];
      ss_atom(en.bb, i - 2, 1, p);
      ss_atom(en.bb, i, 1, c);
      ss_atom(en.bb, i + 2, 1, n);
      const double ax = c[0] - p[0], ay = c[1] - p[1], az = c[2] - p[2], bx = n[0] - c[0], by = n[1] - c[1], bz = n[2] - c[2];
      const double ab = (ax * bx + ay * by) + az * bz, aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz;
      Sf = ab < 0.3420201433256687 * (sqrt(aa) * sqrt(bb));
    }
    // bridges: each disjunct of P(i, j) and A(i, j) holds one of hb(i-1, j), hb(i, j+1), hb(i, j), hb(i-1, j+1)
    int bp1 = -1, bp2 = -1;
    unsigned npar = 0u, nanti = 0u, nhb = 0u;
    for (int w = 0; w < a.words; ++w) {
      const unsigned u0 = m.rword(i - 1, w), u1 = m.rword(i, w), v0 = m.rword(i - 1, w + 1), v1 = m.rword(i, w + 1);
      nhb += __popc(u1);
      unsigned cand = u0 | u1 | ((u0 >> 1) | (v0 << 31)) | ((u1 >> 1) | (v1 << 31));
      while (cand) {
        const int j = 32 * w + __ffs(cand) - 1;
        cand &= cand - 1u;
        const bool p = m.par(i, j), q = m.anti(i, j);
        if (!p && !q) continue;
        if (bp1 < 0) bp1 = j;
        else if (bp2 < 0) bp2 = j;
        npar += p && j > i ? 1u : 0u;
        nanti += q && j > i ? 1u : 0u;
        Ef = Ef || (p && (m.par(i - 1, j - 1) || m.par(i + 1, j + 1))) || (q && (m.anti(i - 1, j + 1) || m.anti(i + 1, j - 1)));
      }
    }
    const int code = at(hf, i) ? 7 : (Ef ? 6 : (bp1 >= 0 ? 5 : (at(gf, i) ? 4 : (If ? 3 : (Tf ? 2 : (Sf ? 1 : 0))))));
    if (e == 0) {
      code0 = code;
      a.out[32 + i] = (float)code;
      a.out[32 + 5 * L + i] = (float)bp1;
      a.out[32 + 6 * L + i] = (float)bp2;
      atomicAdd(&icnt[SS_CNT_CODE + code], 1u);
      if (nhb) atomicAdd(&icnt[SS_CNT_HB], nhb);
      if (npar) atomicAdd(&icnt[SS_CNT_PAR], npar);
      if (nanti) atomicAdd(&icnt[SS_CNT_ANTI], nanti);
    } else {
      a.out[32 + 7 * L + i] = (float)code;
      atomicAdd(&icnt[SS_CNT_NAT + code], 1u);
      if (code == code0) atomicAdd(&icnt[SS_CNT_Q8], 1u);
      if (ss_three(code) == ss_three(code0)) atomicAdd(&icnt[SS_CNT_Q3], 1u);
    }
  }
  if (!native && i < L) a.out[32 + 7 * L + i] = nan;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 0; k < SS_COUNTERS; ++k)
    if (icnt[k]) __hip_atomic_fetch_add(&a.cnt[k], icnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!ticket_take_last(a.ticket, gridDim.x)) return;
  // the last arriver: the header
  // counters 0 .. 10 are offsets 0 .. 10; q3, q8 offsets 12, 13; the native's codes offsets 14 .. 21
  for (int k = 0; k < SS_COUNTERS; ++k) a.out[k < SS_CNT_Q3 ? k : k + 1] = (float)counter_drain(&a.cnt[k]);
  a.out[11] = native ? 1.f : 0.f;
  for (int k = 22; k < 32; ++k) a.out[k] = 0.f;
  ticket_reset(a.ticket);
}

int assign_ss(dmp_ctx* c, const float* d_coords, int L, const float* d_native, float* d_block, hipStream_t s) {
  const SsScratch sc = ss_scratch(c->max_L);
  const NativeEntity nat = native_entity(c);
  unsigned char* ws = c->ss_ws.p;
  SsArgs a{};
  for (int e = 0; e < 2; ++e) {
    a.ent[e].h = (double*)(ws + sc.h[e]);
    a.ent[e].donor = ws + sc.donor[e];
    a.ent[e].R = (unsigned*)(ws + sc.R[e]);
    a.ent[e].T = (unsigned*)(ws + sc.T[e]);
  }
  a.ent[0].bb = d_coords;
  a.ent[1].bb = nat.bb;
  a.row = nat.row;
  a.whole = nat.whole_x;
  a.out = d_block;
  a.L = L;
  a.words = ss_row_words(L);
  a.entities = d_native ? 2 : 1;
  a.cnt = (unsigned*)ws;
  a.ticket = (unsigned*)ws + SS_COUNTERS;
  hipLaunchKernelGGL(ss_prep_kernel, dim3(cdiv(L, SS_THREADS), a.entities), dim3(SS_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ss_hbond_kernel, dim3(L, a.entities, 2), dim3(SS_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ss_assign_kernel, dim3(cdiv(L, SS_THREADS)), dim3(SS_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
