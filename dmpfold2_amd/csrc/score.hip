// option "score_native": the prediction scored against a native C-alpha trace (include/dmpfold_hip.h has the layout of
// the score block and the definition of every number).  Three launches in dmp_predict_end behind ca_to_backbone:
//   score_prep    one workgroup: the rows that have a native residue, packed in sequence order (model trace from
//                 d_coords[:, 1], native from the block), n, lnorm, d0, d_cut; NaN into every out slot but n_pairs.
//   score_lddt    rows dealt to the workgroups: integer counts, so lDDT is exact and order-free.
//   score_search  one workgroup per seed of the superposition search; the last arriver (agent-scope ticket, common.h)
//                 reduces the seeds' records in seed order and writes the header and the deviations.
// Float64 from the float32 coordinates throughout; every sum has a fixed per-thread order, a fixed butterfly inside a
// wave (both partners of an exchange form a + b, so all 64 lanes hold the same bits) and a fixed order over the four
// waves' partial sums in LDS: the same bits on every run, and every thread of a workgroup takes the same branch.
// Nothing here is a reference computation, so contraction is switched off only to keep the bits independent of the
// compiler's choices.
#include "score_common.h"

namespace dmp {

constexpr int SC_LDDT_MAX_WG = 64;
// a seed's record (SCORE_REC doubles): tm, the five counts, R (9), t (3), rmsd (seed 0 only), spare
constexpr int REC_TM = 0, REC_CNT = 1, REC_R = 6, REC_T = 15, REC_RMSD = 18;
// header of the scratch: n, lnorm, d0, d_cut
constexpr int HDR_N = 0, HDR_LNORM = 1, HDR_D0 = 2, HDR_DCUT = 3;

// The distinct fragment lengths f_0 = n, f_k = max(n >> k, min(4, n)), k = 1..5, in level order (they never increase, so
// a repeat is a repeat of the one before); returns how many.
__host__ __device__ inline int score_levels(int n, int f[6]) {
  const int lo = n < 4 ? n : 4;
  int m = 0;
  for (int k = 0; k <= 5; ++k) {
    const int v = k == 0 ? n : ((n >> k) > lo ? (n >> k) : lo);
    if (m == 0 || f[m - 1] != v) f[m++] = v;
  }
  return m;
}

// Seeds of n rows: every start of every distinct fragment length.  Never decreases with n (n - f_k + 1 does not, and a
// longer chain has no fewer distinct levels), so a grid sized for L covers every n <= L; at most 1 + 5n.
__host__ __device__ inline int score_seeds(int n) {
  int f[6];
  const int m = score_levels(n, f);
  int total = 0;
  for (int q = 0; q < m; ++q) total += n - f[q] + 1;
  return total;
}


__device__ inline double score_dist(const float* a, const float* b) {
  const double ux = (double)a[0] - (double)b[0], uy = (double)a[1] - (double)b[1], uz = (double)a[2] - (double)b[2];
  return sqrt((ux * ux + uy * uy) + uz * uz);
}


struct ScoreArgs {
  const float* coords;   // [L][5][3] the backbone; the model trace is atom 1
  float* blk;            // the score block: [0, 3L) native (in), 3L lnorm (in), the rest out
  int L;
  float* pm;             // [n][3] packed model trace
  float* qn;             // [n][3] packed native trace
  int* idx;              // [n] alignment column of a packed row
  double* hdr;           // [8]
  double* rec;           // [seeds][SCORE_REC]
  unsigned long long* tot;   // [2] lDDT: preserved, pairs
  unsigned* ticket;      // zero between launches
};

// ---------------------------------------------------------------------------------------
// score_prep: pack the present rows, the constants, NaN into the out slots
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void score_prep_kernel(ScoreArgs a) {
  __shared__ int cnt[SC_THREADS];
  const int L = a.L, tid = threadIdx.x;
  const int chunk = (L + SC_THREADS - 1) / SC_THREADS;
  const int r0 = tid * chunk < L ? tid * chunk : L, r1 = r0 + chunk < L ? r0 + chunk : L;
  int mine = 0;
  for (int i = r0; i < r1; ++i) {
    const float x = a.blk[3 * i];
    mine += x == x ? 1 : 0;
  }
  cnt[tid] = mine;
  __syncthreads();
  int at = 0, n = 0;
  for (int k = 0; k < SC_THREADS; ++k) {
    if (k < tid) at += cnt[k];
    n += cnt[k];
  }
  for (int i = r0; i < r1; ++i) {
    const float x = a.blk[3 * i];
    if (x == x) {
      for (int c = 0; c < 3; ++c) {
        a.pm[3 * at + c] = a.coords[15 * (int64_t)i + 3 + c];
        a.qn[3 * at + c] = a.blk[3 * i + c];
      }
      a.idx[at] = i;
      ++at;
    }
  }
  const float nan = __builtin_nanf("");
  const ScoreLayout lay = score_layout(L);
  float* out = a.blk + lay.out;
  for (int i = tid; i < lay.total - lay.out; i += SC_THREADS) out[i] = i == 0 ? (float)n : nan;
  if (tid == 0) {
    const double given = (double)a.blk[lay.lnorm];
    const double lnorm = given == 0.0 ? (double)n : given;
    const double d0 = lnorm > 15.0 ? fmax(1.24 * cbrt(lnorm - 15.0) - 1.8, 0.5) : 0.5;
    a.hdr[HDR_N] = (double)n;
    a.hdr[HDR_LNORM] = lnorm;
    a.hdr[HDR_D0] = d0;
    a.hdr[HDR_DCUT] = fmin(fmax(d0, 4.5), 8.0);
    a.tot[0] = 0ull;
    a.tot[1] = 0ull;
  }
}

// ---------------------------------------------------------------------------------------
// score_lddt: superposition-free, integer counts
// ---------------------------------------------------------------------------------------
__host__ __device__ inline int score_lddt_groups(int L) {
  const int g = L / 16;
  return g < 1 ? 1 : (g > SC_LDDT_MAX_WG ? SC_LDDT_MAX_WG : g);
}

__global__ __launch_bounds__(SC_THREADS) void score_lddt_kernel(ScoreArgs a) {
  extern __shared__ float sm[];          // 2 x 3n coordinates
  __shared__ int ired[SC_WAVES][2];
  const int n = (int)a.hdr[HDR_N], L = a.L, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (n < 3) return;                     // every out slot but n_pairs stays NaN
  float* pm = sm;
  float* qn = sm + 3 * n;
  for (int i = tid; i < 3 * n; i += SC_THREADS) { pm[i] = a.pm[i]; qn[i] = a.qn[i]; }
  __syncthreads();
  float* out = a.blk + score_layout(L).lddt_res;
  unsigned long long tot_pres = 0ull, tot_part = 0ull;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    int pres = 0, part = 0;
    for (int j = tid; j < n; j += SC_THREADS) {
      if (j == i) continue;
      const double dn = score_dist(qn + 3 * i, qn + 3 * j);
      if (dn < 15.0) {
        const double e = fabs(score_dist(pm + 3 * i, pm + 3 * j) - dn);
        part += 1;
        pres += (e < 0.5 ? 1 : 0) + (e < 1.0 ? 1 : 0) + (e < 2.0 ? 1 : 0) + (e < 4.0 ? 1 : 0);
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
      out[a.idx[i]] = part > 0 ? (float)((double)pres / (4.0 * (double)part)) : 0.f;
      tot_pres += (unsigned long long)pres;
      tot_part += (unsigned long long)part;
    }
  }
  if (tid == 0) {
    __hip_atomic_fetch_add(&a.tot[0], tot_pres, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&a.tot[1], tot_part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------
// score_search: one workgroup per seed
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void score_search_kernel(ScoreArgs a) {
  extern __shared__ float sm[];          // 2 x 3n coordinates, then n flags: the set S
  __shared__ double wred[SC_WAVES][16];
  __shared__ double bc[12];              // R, t of this iteration (at the end: of the best seed)
  __shared__ int sh_last, sh_seed[SC_WAVES];
  const int n = (int)a.hdr[HDR_N], L = a.L, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (n < 3) return;
  int nseeds = score_seeds(n);
  if (nseeds > (int)gridDim.x) nseeds = (int)gridDim.x;     // never: score_seeds does not decrease with n, the grid is score_seeds(L)
  if ((int)blockIdx.x >= nseeds) return;
  const double lnorm = a.hdr[HDR_LNORM], d0 = a.hdr[HDR_D0], d_cut = a.hdr[HDR_DCUT];
  // (level, start) of this seed
  int frag, start = (int)blockIdx.x;
  {
    int f[6];
    const int m = score_levels(n, f);
    int q = 0;
    while (q < m - 1 && start >= n - f[q] + 1) { start -= n - f[q] + 1; ++q; }
    frag = f[q];
  }
  float* pm = sm;
  float* qn = sm + 3 * n;
  unsigned char* fl = reinterpret_cast<unsigned char*>(sm + 6 * n);
  for (int i = tid; i < 3 * n; i += SC_THREADS) { pm[i] = a.pm[i]; qn[i] = a.qn[i]; }
  for (int k = tid; k < n; k += SC_THREADS) fl[k] = (k >= start && k < start + frag) ? 1 : 0;
  __syncthreads();

  // thread 0 keeps the seed's best
  SeedBest best;
  score_seed_loop(pm, qn, fl, n, lnorm, d0, d_cut, wred, bc, best);
  const double best_tm = best.tm, rmsd = best.rmsd;
  const double *best_R = best.R, *best_t = best.t, *best_cnt = best.cnt;

  if (tid == 0) {
    double* rec = a.rec + (int64_t)blockIdx.x * SCORE_REC;
    agent_store_f64(rec + REC_TM, best_tm);
    for (int c = 0; c < 5; ++c) agent_store_f64(rec + REC_CNT + c, best_cnt[c]);
    for (int c = 0; c < 9; ++c) agent_store_f64(rec + REC_R + c, best_R[c]);
    for (int c = 0; c < 3; ++c) agent_store_f64(rec + REC_T + c, best_t[c]);
    agent_store_f64(rec + REC_RMSD, rmsd);
    sh_last = ticket_take_last(a.ticket, (unsigned)nseeds) ? 1 : 0;     // every record is behind its owner's release
    if (sh_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!sh_last) return;

  // the last arriver: the best seed (ties: the lowest number) and the maximum of each count, every thread over its share of
  // the records (agent-scope loads), then a butterfly and the four waves in order - a maximum does not depend on the order
  double top = -__builtin_inf();
  int top_seed = 0x7fffffff;
  double cmax[5] = {0, 0, 0, 0, 0};
  for (int s = tid; s < nseeds; s += SC_THREADS) {
    double* rec = a.rec + (int64_t)s * SCORE_REC;
    const double tm = agent_load_f64(rec + REC_TM);
    if (tm > top) { top = tm; top_seed = s; }          // s rises: the first of equals stays
    for (int c = 0; c < 5; ++c) cmax[c] = fmax(cmax[c], agent_load_f64(rec + REC_CNT + c));
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o_top = __shfl_xor(top, off, 64);
    const int o_seed = __shfl_xor(top_seed, off, 64);
    if (o_top > top || (o_top == top && o_seed < top_seed)) { top = o_top; top_seed = o_seed; }
    for (int c = 0; c < 5; ++c) cmax[c] = fmax(cmax[c], __shfl_xor(cmax[c], off, 64));
  }
  __syncthreads();
  if (lane == 0) {
    wred[wv][0] = top;
    sh_seed[wv] = top_seed;
    for (int c = 0; c < 5; ++c) wred[wv][1 + c] = cmax[c];
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < SC_WAVES; ++k) {
      if (wred[k][0] > top || (wred[k][0] == top && sh_seed[k] < top_seed)) { top = wred[k][0]; top_seed = sh_seed[k]; }
      for (int c = 0; c < 5; ++c) cmax[c] = fmax(cmax[c], wred[k][1 + c]);
    }
    float* out = a.blk + score_layout(L).lnorm;        // the header
    const float nan = __builtin_nanf("");
    const bool found = top_seed != 0x7fffffff;         // false only if every seed's tm is NaN
    double* rec = a.rec + (int64_t)(found ? top_seed : 0) * SCORE_REC;
    out[2] = (float)agent_load_f64(a.rec + REC_RMSD);
    out[3] = found ? (float)top : nan;
    out[4] = (float)((((cmax[1] + cmax[2]) + cmax[3]) + cmax[4]) / 4.0 / lnorm);
    out[5] = (float)((((cmax[0] + cmax[1]) + cmax[2]) + cmax[3]) / 4.0 / lnorm);
    const unsigned long long pres = a.tot[0], part = a.tot[1];     // score_lddt ran before this launch
    out[6] = part > 0 ? (float)((double)pres / (4.0 * (double)part)) : 0.f;
    for (int c = 0; c < 5; ++c) out[7 + c] = (float)cmax[c];
    for (int c = 0; c < 12; ++c) {
      const double v = agent_load_f64(rec + REC_R + c);
      bc[c] = v;
      out[12 + c] = found ? (float)v : nan;
    }
    sh_last = found ? 1 : 0;
    ticket_reset(a.ticket);
  }
  __syncthreads();
  if (!sh_last) return;                                // the deviations stay NaN
  double R[9], t[3];
  for (int c = 0; c < 9; ++c) R[c] = bc[c];
  for (int c = 0; c < 3; ++c) t[c] = bc[9 + c];
  float* dev = a.blk + score_layout(L).deviation;
  for (int k = tid; k < n; k += SC_THREADS) dev[a.idx[k]] = (float)score_dev(R, t, pm + 3 * k, qn + 3 * k);
}

int score_native(dmp_ctx* c, const float* d_coords, int L, float* d_block, hipStream_t s) {
  ScoreArgs a{};
  a.coords = d_coords;
  a.blk = d_block;
  a.L = L;
  a.pm = c->score_pm;
  a.qn = c->score_qn;
  a.idx = c->score_idx;
  a.hdr = c->score_hdr;
  a.rec = c->score_rec;
  a.tot = c->score_tot;
  a.ticket = c->score_ticket;
  hipLaunchKernelGGL(score_prep_kernel, dim3(1), dim3(SC_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_lddt_kernel, dim3(score_lddt_groups(L)), dim3(SC_THREADS), sizeof(float) * 6 * L, s, a);
  DMP_LAUNCH_CHECK();
  // the records hold 6 max_L seeds >= 1 + 5L; 6L floats + L flags of LDS: 50 KB at L = 2048
  hipLaunchKernelGGL(score_search_kernel, dim3(score_seeds(L)), dim3(SC_THREADS), sizeof(float) * 6 * L + round_up(L, 16), s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
