// option "score_map": the chosen pass's predicted distance map scored against the native trace of option "score_native"
// (include/dmpfold_hip.h has the layout of the map-score block and the definition of every number).  Two launches in
// dmp_predict_end behind score_native, reading c->best_dm and the score block's inputs (the native trace, lnorm):
//   mapscore_count   rows dealt to the workgroups.  Per residue and in total the distance agreement (the pair set of
//                    score_native's lDDT, the model's distance replaced by dm), per class the candidates, the native contacts
//                    and the contacts at the 8 A threshold.  Integer counts go thread -> LDS -> one integer atomic per workgroup
//                    and counter (integers: order-free); the three float64 error sums go through grid_sum_f64 (common.h), whose
//                    last arriver of the third sum writes the header and puts the counters back to zero.
//   mapscore_select  one workgroup per (class, list): the t-th smallest key bits(dm) << 22 | (i L + j) of the class by a radix
//                    select - digit histograms in LDS, the class's pairs re-read once per 8-bit digit, the three digits of
//                    the pair index only where the list ends inside a run of equal values - then h = the native contacts
//                    among the keys <= that one.  The keys are unique, so ties are no separate path.
//                    A template over what it ranks by: MsByDistance is this option's, MsByCoupling option "msa_report"'s
//                    (mapscore_select_couplings, the DCA contact map strongest first).
// No float atomics; every float64 sum has a fixed order: the same bits on every run.  Contraction is off (score_common.h) so
// that the float32 contact test rounds every operation, as the definition says.
#include "score_common.h"

namespace dmp {

static_assert((int64_t)DMP_MAX_L * DMP_MAX_L <= (1 << 22), "the pair index i L + j takes 22 bits of the key");

constexpr int MS_MAX_WG = 64;          // = the partial sums a context holds per error sum
constexpr int MS_SEL_THREADS = 1024;
constexpr int MS_SEL_BATCH = 4;        // pairs a thread loads before it looks at any of them
// counters of the context (unsigned, zero between launches): 4 per class 0..2, then preserved, pairs
constexpr int MS_CNT_N = 0, MS_CNT_NAT = 1, MS_CNT_TP = 2, MS_CNT_PRED = 3, MS_CNT_PRES = 12, MS_CNT_PAIRS = 13, MS_COUNTERS = 14;

struct MapScoreArgs {
  const float* dm;       // [L][L] c->best_dm
  const float* nat;      // the score block: [0, 3L) native trace, [3L] lnorm
  float* out;            // the map-score block, 64 + L floats
  int L;
  unsigned* cnt;         // [MS_COUNTERS]
  double* partial;       // [3][MS_MAX_WG]
  double* sums;          // [3] sum |e|, sum e^2, sum e
  unsigned* ticket;      // [3] zero between launches
};

__device__ inline double ms_dist(const float* a, const float* b) {
  const double ux = (double)a[0] - (double)b[0], uy = (double)a[1] - (double)b[1], uz = (double)a[2] - (double)b[2];
  return sqrt((ux * ux + uy * uy) + uz * uz);
}
// the native contact test: float32, every operation rounded
__device__ inline bool ms_native_contact(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz < 64.0f;
}
__host__ __device__ inline int mapscore_groups(int L) {
  const int g = L / 16;
  return g < 1 ? 1 : (g > MS_MAX_WG ? MS_MAX_WG : g);
}

// ---------------------------------------------------------------------------------------
// mapscore_count
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void mapscore_count_kernel(MapScoreArgs a) {
  extern __shared__ float q[];           // 3L native coordinates
  __shared__ double red[SC_THREADS];
  __shared__ unsigned icnt[MS_COUNTERS];
  __shared__ int ired[SC_WAVES][2];
  const int L = a.L, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < 3 * L; i += SC_THREADS) q[i] = a.nat[i];
  if (tid < MS_COUNTERS) icnt[tid] = 0u;
  __syncthreads();
  const float nan = __builtin_nanf("");
  unsigned cls[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double s_abs = 0.0, s_sq = 0.0, s_e = 0.0;
  unsigned tot_pres = 0u, tot_part = 0u;           // thread 0
  for (int i = blockIdx.x; i < L; i += gridDim.x) {
    if (!(q[3 * i] == q[3 * i])) {                 // uniform: the row is absent
      if (tid == 0) a.out[64 + i] = nan;
      continue;
    }
    const float* row = a.dm + (int64_t)i * L;
    int pres = 0, part = 0;
    for (int j = tid; j < L; j += SC_THREADS) {
      if (j == i || !(q[3 * j] == q[3 * j])) continue;
      const float d = row[j];
      const double dn = ms_dist(q + 3 * i, q + 3 * j);
      if (dn < 15.0) {
        const double e = (double)d - dn, ae = fabs(e);
        part += 1;
        pres += (ae < 0.5 ? 1 : 0) + (ae < 1.0 ? 1 : 0) + (ae < 2.0 ? 1 : 0) + (ae < 4.0 ? 1 : 0);
        s_abs += ae;
        s_sq += e * e;
        s_e += e;
      }
      const int s = j - i;
      if (s >= 6) {
        const int c = s <= 11 ? 0 : (s <= 23 ? 1 : 2);
        const bool nc = ms_native_contact(q + 3 * i, q + 3 * j), pc = d < 8.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {              // (constant indices: the counters stay in registers)
          if (k == c) {
            cls[4 * k + MS_CNT_N] += 1u;
            cls[4 * k + MS_CNT_NAT] += nc ? 1u : 0u;
            cls[4 * k + MS_CNT_TP] += (nc && pc) ? 1u : 0u;
            cls[4 * k + MS_CNT_PRED] += pc ? 1u : 0u;
          }
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      pres += __shfl_xor(pres, off, 64);
      part += __shfl_xor(part, off, 64);
    }
    __syncthreads();
    if (lane == 0) { ired[wv][0] = pres; ired[wv][1] = part; }
    __syncthreads();
    if (tid == 0) {
      pres = part = 0;
      for (int k = 0; k < SC_WAVES; ++k) { pres += ired[k][0]; part += ired[k][1]; }
      a.out[64 + i] = part > 0 ? (float)((double)pres / (4.0 * (double)part)) : 0.f;
      tot_pres += (unsigned)pres;
      tot_part += (unsigned)part;
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    unsigned v = cls[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0 && v) atomicAdd(&icnt[k], v);
  }
  __syncthreads();
  if (tid == 0) {
    icnt[MS_CNT_PRES] = tot_pres;
    icnt[MS_CNT_PAIRS] = tot_part;
    for (int k = 0; k < MS_COUNTERS; ++k)
      if (icnt[k]) __hip_atomic_fetch_add(&a.cnt[k], icnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // thread 0's atomics above are in front of its three tickets; whoever arrives last at the third finds every workgroup's
  // counts, and the first two totals behind the tickets their writers took afterwards
  double total = 0.0;
  if (grid_sum_f64<SC_THREADS>(s_abs, red, a.partial, a.ticket, &total)) agent_store_f64(&a.sums[0], total);
  if (grid_sum_f64<SC_THREADS>(s_sq, red, a.partial + MS_MAX_WG, a.ticket + 1, &total)) agent_store_f64(&a.sums[1], total);
  if (!grid_sum_f64<SC_THREADS>(s_e, red, a.partial + 2 * MS_MAX_WG, a.ticket + 2, &total)) return;
  // the last arriver (one thread): the header
  const double sum_abs = agent_load_f64(&a.sums[0]), sum_sq = agent_load_f64(&a.sums[1]), sum_e = total;
  unsigned cn[MS_COUNTERS];
  for (int k = 0; k < MS_COUNTERS; ++k) cn[k] = counter_drain(&a.cnt[k]);
  int n = 0;
  for (int i = 0; i < L; ++i) n += q[3 * i] == q[3 * i] ? 1 : 0;
  const float lnorm = a.nat[3 * L];
  float* out = a.out;
  out[0] = (float)n;
  out[1] = lnorm > 0.f ? lnorm : (float)n;
  for (int c = 0; c < 4; ++c) {
    float* o = out + 2 + 12 * c;
    // class 3 = medium + long; slots 2..7 (h, t) are mapscore_select's
    const unsigned* u = cn + 4 * (c < 3 ? c : 1);
    const unsigned* w = cn + 4 * 2;
    const bool both = c == 3;
    o[0] = (float)(u[MS_CNT_N] + (both ? w[MS_CNT_N] : 0u));
    o[1] = (float)(u[MS_CNT_NAT] + (both ? w[MS_CNT_NAT] : 0u));
    o[8] = (float)(u[MS_CNT_TP] + (both ? w[MS_CNT_TP] : 0u));
    o[9] = (float)(u[MS_CNT_PRED] + (both ? w[MS_CNT_PRED] : 0u));
    o[10] = 0.f;
    o[11] = 0.f;
  }
  const double pairs = (double)cn[MS_CNT_PAIRS];
  out[50] = (float)pairs;
  if (n < 2) {
    out[51] = out[52] = out[53] = out[54] = nan;
  } else {
    out[51] = cn[MS_CNT_PAIRS] > 0u ? (float)((double)cn[MS_CNT_PRES] / (4.0 * pairs)) : 0.f;
    out[52] = cn[MS_CNT_PAIRS] > 0u ? (float)(sum_abs / pairs) : nan;
    out[53] = cn[MS_CNT_PAIRS] > 0u ? (float)sqrt(sum_sq / pairs) : nan;
    out[54] = cn[MS_CNT_PAIRS] > 0u ? (float)(sum_e / pairs) : nan;
  }
  for (int k = 55; k < 64; ++k) out[k] = 0.f;
}

// ---------------------------------------------------------------------------------------
// mapscore_select
// ---------------------------------------------------------------------------------------
// The candidates of a class as a flat range [0, total): classes 0 and 1 are bands of W separations, idx = i W + w; classes 2
// and 3 (every separation from `lo` on) are a triangle of R = L - lo rows, row r holding R - r pairs, folded into a rectangle
// of (R + 1) / 2 rows by R + 1 columns - row r, then row R - 1 - r.
struct MsClass { int lo, W, R, total; };
__device__ inline MsClass ms_class(int c, int L) {
  MsClass k;
  k.lo = c == 0 ? 6 : (c == 2 ? 24 : 12);
  k.W = c == 0 ? 6 : (c == 1 ? 12 : 0);
  k.R = L - k.lo > 0 ? L - k.lo : 0;
  k.total = k.W ? L * k.W : ((k.R + 1) / 2) * (k.R + 1);
  return k;
}
// pair `idx` of the range: false where the rectangle holds none (past the chain's end, the middle row's second half)
__device__ inline bool ms_pair(const MsClass& k, int L, int idx, int& i, int& j) {
  if (k.W) {
    i = idx / k.W;
    j = i + k.lo + (idx - i * k.W);
    return j < L;
  }
  const int r = idx / (k.R + 1), col = idx - r * (k.R + 1);
  if (col < k.R - r) {
    i = r;
    j = i + k.lo + col;
    return true;
  }
  i = k.R - 1 - r;
  j = i + k.lo + (col - (k.R - r));
  return i != r;
}

// What a select ranks by, and where its block keeps ln: the 32 bits in front of the pair index, ascending.  MsByDistance is
// "score_map"'s (dm is not negative: its bits are its order; the block's offsets 0, 1 are n, ln and the classes follow at 2).
// MsByCoupling is "msa_report"'s (msareport.hip): the DCA contact map DESCENDING - an order-preserving map of the float's
// bits, inverted, every NaN last; the classes at the report block's offset 76 have "score_map"'s slots, so `out` is handed
// over as the block + 74 and n, ln (124, 125) lie at 50, 51 of it.
struct MsByDistance {
  static constexpr int LN = 1;
  __device__ static inline unsigned bits(float v) { return __float_as_uint(v); }
};
struct MsByCoupling {
  static constexpr int LN = 51;
  __device__ static inline unsigned bits(float v) { return coupling_rank_bits(v); }
};

// f(key, i, j) for every candidate of the class, MS_SEL_BATCH loads in flight per thread.  Every thread of the workgroup.
template <class K, class F>
__device__ inline void ms_for_each(const MsClass& k, int L, const float* q, const float* dm, F f) {
  for (int base = threadIdx.x; base < k.total; base += MS_SEL_BATCH * MS_SEL_THREADS) {
    int ii[MS_SEL_BATCH], jj[MS_SEL_BATCH];
    bool ok[MS_SEL_BATCH];
    float v[MS_SEL_BATCH];
#pragma unroll
    for (int u = 0; u < MS_SEL_BATCH; ++u) {
      const int idx = base + u * MS_SEL_THREADS;
      ii[u] = jj[u] = 0;
      ok[u] = idx < k.total && ms_pair(k, L, idx, ii[u], jj[u]);
      ok[u] = ok[u] && q[3 * ii[u]] == q[3 * ii[u]] && q[3 * jj[u]] == q[3 * jj[u]];
      v[u] = ok[u] ? dm[(int64_t)ii[u] * L + jj[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < MS_SEL_BATCH; ++u)
      if (ok[u]) f(((unsigned long long)K::bits(v[u]) << 22) | (unsigned long long)(ii[u] * L + jj[u]), ii[u], jj[u]);
  }
}

template <class K>
__global__ __launch_bounds__(MS_SEL_THREADS) void mapscore_select_kernel(MapScoreArgs a) {
  extern __shared__ float q[];           // 3L native coordinates
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sh_prefix, sh_k;
  __shared__ unsigned sh_h;
  __shared__ int sh_done;
  const int L = a.L, tid = threadIdx.x, c = blockIdx.x / 3, dq = blockIdx.x % 3;
  float* o = a.out + 2 + 12 * c;
  // N_c and ln as mapscore_count left them
  const double Nc = (double)o[0], ln = (double)a.out[K::LN];
  const double kd = fmax(1.0, floor(ln / (dq == 0 ? 1.0 : (dq == 1 ? 2.0 : 5.0))));
  const unsigned t = (unsigned)fmin(kd, Nc);       // N_c < 2^24
  if (t == 0u) {                                   // uniform: an empty class
    if (tid == 0) { o[2 + dq] = 0.f; o[5 + dq] = 0.f; }
    return;
  }
  for (int i = tid; i < 3 * L; i += MS_SEL_THREADS) q[i] = a.nat[i];
  if (tid == 0) { sh_prefix = 0ull; sh_k = t; sh_h = 0u; sh_done = 0; }
  const MsClass k = ms_class(c, L);
  // 54 bits from the top: six digits of 8 bits, one of 6
  for (int p = 0; p < 7; ++p) {
    const int nb = p < 6 ? 8 : 6, sh = p < 6 ? 46 - 8 * p : 0;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = sh_prefix;
    ms_for_each<K>(k, L, q, a.dm, [&](unsigned long long key, int, int) {
      if ((key >> (sh + nb)) == prefix) atomicAdd(&hist[(unsigned)(key >> sh) & ((1u << nb) - 1u)], 1u);
    });
    __syncthreads();
    if (tid == 0) {
      unsigned long long want = sh_k;
      unsigned b = 0;
      for (; b + 1 < (1u << nb) && want > hist[b]; ++b) want -= hist[b];     // the bucket that holds the want-th of the prefix
      sh_prefix = (prefix << nb) | b;
      sh_k = want;
      // all 32 bits of dm are fixed and the list ends with the last pair of that value (always, where no two candidates
      // share a value): every key of the value belongs, the three passes over the pair index have nothing to decide
      if (p == 3 && want == hist[b]) {
        sh_prefix = (sh_prefix << 22) | 0x3fffffull;
        sh_done = 1;
      }
    }
    __syncthreads();
    if (sh_done) break;                            // uniform
  }
  const unsigned long long thr = sh_prefix;
  unsigned mine = 0u;
  ms_for_each<K>(k, L, q, a.dm, [&](unsigned long long key, int i, int j) {
    mine += (key <= thr && ms_native_contact(q + 3 * i, q + 3 * j)) ? 1u : 0u;
  });
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((tid & 63) == 0 && mine) atomicAdd(&sh_h, mine);
  __syncthreads();
  if (tid == 0) { o[2 + dq] = (float)sh_h; o[5 + dq] = (float)t; }
}

// The scratch (dmp_ctx::map_ws; common.h: Scratch), bytes from its start.  The head: the counters, then the three tickets; behind
// it the per-workgroup error sums and their totals.  1.7 KB.
constexpr int64_t MS_WS_CNT = 0, MS_WS_TICKET = 64, MS_WS_HEAD = 80, MS_WS_PARTIAL = MS_WS_HEAD,
                  MS_WS_SUMS = MS_WS_PARTIAL + 8 * 3 * MS_MAX_WG, MS_WS_BYTES = MS_WS_SUMS + 32;
static_assert(4 * MS_COUNTERS <= MS_WS_TICKET && MS_WS_TICKET + 4 * 3 <= MS_WS_HEAD, "the head holds the counters and the tickets");
ScratchNeed score_map_need() { return {MS_WS_BYTES, MS_WS_HEAD}; }

int score_map(dmp_ctx* c, int L, const float* d_score_block, float* d_block, hipStream_t s) {
  MapScoreArgs a{};
  a.dm = c->best_dm;
  a.nat = d_score_block;
  a.out = d_block;
  a.L = L;
  a.cnt = reinterpret_cast<unsigned*>(c->map_ws.p + MS_WS_CNT);
  a.ticket = reinterpret_cast<unsigned*>(c->map_ws.p + MS_WS_TICKET);
  a.partial = reinterpret_cast<double*>(c->map_ws.p + MS_WS_PARTIAL);
  a.sums = reinterpret_cast<double*>(c->map_ws.p + MS_WS_SUMS);
  hipLaunchKernelGGL(mapscore_count_kernel, dim3(mapscore_groups(L)), dim3(SC_THREADS), sizeof(float) * 3 * L, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mapscore_select_kernel<MsByDistance>, dim3(12), dim3(MS_SEL_THREADS), sizeof(float) * 3 * L, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// option "msa_report" (msareport.hip): the same select over the DCA contact map, strongest coupling first.  `d_classes`: the
// report block + 74, N_c of every class and n, ln already in it (msareport_pairs_kernel and msareport_classes_kernel, in front of this on the stream).
int mapscore_select_couplings(const float* d_contacts, const float* d_score_block, float* d_classes, int L, hipStream_t s) {
  MapScoreArgs a{};
  a.dm = d_contacts;
  a.nat = d_score_block;
  a.out = d_classes;
  a.L = L;
  hipLaunchKernelGGL(mapscore_select_kernel<MsByCoupling>, dim3(12), dim3(MS_SEL_THREADS), sizeof(float) * 3 * L, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
