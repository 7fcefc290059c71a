// option "score_native": the prediction scored against a native C-alpha trace (include/dmpfold_hip.h has the layout of
// the score block and the definition of every number).  Three launches in dmp_predict_end behind ca_to_backbone:
//   score_prep    one workgroup: the rows that have a native residue, packed in sequence order (model trace from
//                 d_coords[:, 1], native from the block), n, lnorm, d0, d_cut; NaN into every out slot but n_pairs.
//   score_lddt    rows dealt to the workgroups: integer counts, so lDDT is exact and order-free.
//   score_search  one workgroup per seed of the superposition search; the last arriver (agent-scope ticket, common.h)
//                 reduces the seeds' records in seed order and writes the header and the deviations.
// Option "score_passes" (at the end of this file) runs score_lddt and score_search over the recorded passes' traces, the pass
// as blockIdx.y, with the native that score_prep packed.  Option "score_domains" (behind it) runs the same two bodies per domain
// of the domain block's two labellings, on traces it packs itself.
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


// One description for the three uses.  "score_native": one model trace (atom 1 of the backbone: `model` = d_coords + 3, 15 floats
// between rows), a grid with gridDim.y = 1, `rows` null, the results into the score block.  "score_passes": the model traces
// are ca_pass[pass0 + blockIdx.y] (3 floats between rows, 3L between traces); the packed native, the row index and the
// header are the ones score_prep made for the score block of the same call (their strides are 0); every pass has its own packed
// model, totals, records and ticket (`*_stride` apart), and its five scores go to its row of the pass block.  "score_domains"
// (at the end of this file): a slot is a leg, everything in it one leg apart - its own packed native, columns and headers too -
// and `info` says where each domain lies inside the leg.
struct ScoreArgs {
  const float* model;    // the model trace's first row
  int model_row;         // floats between its rows
  int64_t model_stride;  // floats between the traces of consecutive passes
  float* blk;            // the score block: [0, 3L) native (in), 3L lnorm (in), the rest out
  int L;
  float* pm;             // [n][3] packed model trace (slot y: + y * pm_stride)
  float* qn;             // [n][3] packed native trace (slot y: + y * qn_stride)
  int* idx;              // [n] alignment column of a packed row (slot y: + y * idx_stride)
  double* hdr;           // [8] (slot y: + y * hdr_stride)
  double* rec;           // [seeds][SCORE_REC] (slot y: + y * rec_stride)
  unsigned long long* tot;   // [2] lDDT: preserved, pairs (slot y: + y * tot_stride)
  unsigned* ticket;      // zero between launches (slot y: + y * ticket_stride)
  int64_t pm_stride, rec_stride, tot_stride;
  float* rows;           // null, or row 0 of this launch's passes in the pass block
  int64_t qn_stride, idx_stride, hdr_stride;   // 0: one native, one index, one header for every slot
  int ticket_stride;     // 1, or the tickets of a leg
  int* info;             // "score_domains" only: DS_INFO ints per leg (below), idx_stride apart
  float* dom;            // "score_domains" only: the domain-score block
};

// What one launch's workgroup works on, resolved from the arguments: the whole slot y ("score_native", "score_passes"), or
// domain d of leg y ("score_domains").  The packed rows [r0, r0 + n) of the slot's `nall` are the trace that is scored; the
// rest of the slot's rows are only partners of the two outer counters of the lDDT.
struct ScoreView {
  const float *pm, *qn;      // the slot's packed traces, row 0
  const int* idx;            // the slot's columns
  const double* hdr;         // n, lnorm, d0, d_cut of the trace that is scored
  double* rec;               // its seed records
  unsigned long long* tot;   // [2] preserved, pairs inside it (+ [2] the outer counters, with `outer`)
  unsigned* ticket;
  int r0, n, nall;
  bool outer;                // count the pairs that leave the trace as well, and count whatever n is
  float* head;               // where header float 0 (lnorm) would lie: floats 2 .. 23 are written; null for a pass
  float* row;                // a pass's row, or null
  float* lddt_res;           // [L] by column, or null
  float* dev;                // [L] by column, or null
};
__device__ inline ScoreView score_view(const ScoreArgs& a, int y) {
  ScoreView v;
  v.pm = a.pm + y * a.pm_stride;
  v.qn = a.qn + y * a.qn_stride;
  v.idx = a.idx + y * a.idx_stride;
  v.hdr = a.hdr + y * a.hdr_stride;
  v.rec = a.rec + y * a.rec_stride;
  v.tot = a.tot + y * a.tot_stride;
  v.ticket = a.ticket + y * a.ticket_stride;
  v.r0 = 0;
  v.n = v.nall = (int)v.hdr[HDR_N];
  v.outer = false;
  const ScoreLayout lay = score_layout(a.L);
  v.head = a.rows ? nullptr : a.blk + lay.lnorm;
  v.row = a.rows ? a.rows + PASS_ROW * (int64_t)y : nullptr;
  v.lddt_res = a.rows ? nullptr : a.blk + lay.lddt_res;       // the passes have no per-residue arrays
  v.dev = a.rows ? nullptr : a.blk + lay.deviation;
  return v;
}

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
        a.pm[3 * at + c] = a.model[a.model_row * (int64_t)i + c];
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

// score_pass_prep: pass blockIdx.y's trace packed by the row index score_prep left; its lDDT totals cleared
__global__ __launch_bounds__(SC_THREADS) void score_pass_prep_kernel(ScoreArgs a) {
  const int n = (int)a.hdr[HDR_N], y = blockIdx.y;
  const int k = blockIdx.x * SC_THREADS + threadIdx.x;
  if (k < n) {
    const float* src = a.model + y * a.model_stride + a.model_row * (int64_t)a.idx[k];
    float* dst = a.pm + y * a.pm_stride + 3 * k;
    for (int c = 0; c < 3; ++c) dst[c] = src[c];
  }
  if (k == 0) {
    a.tot[y * a.tot_stride] = 0ull;
    a.tot[y * a.tot_stride + 1] = 0ull;
  }
}

// ---------------------------------------------------------------------------------------
// score_lddt: superposition-free, integer counts
// ---------------------------------------------------------------------------------------
__host__ __device__ inline int score_lddt_groups(int L) {
  const int g = L / 16;
  return g < 1 ? 1 : (g > SC_LDDT_MAX_WG ? SC_LDDT_MAX_WG : g);
}

// The rows of the view's trace dealt to `groups` workgroups, this one being number `g`; the partners of a row are all the
// slot's rows: those of the trace count for the lDDT, the others - with `outer` - into the two outer counters.
__device__ inline void score_lddt_body(const ScoreView& v, int g, int groups, float* sm) {
  __shared__ int ired[SC_WAVES][4];
  const int n = v.n, nall = v.nall, r0 = v.r0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (n < 3 && !v.outer) return;         // every out slot but n_pairs stays NaN
  float* pm = sm;                        // 2 x 3 nall coordinates
  float* qn = sm + 3 * nall;
  for (int i = tid; i < 3 * nall; i += SC_THREADS) { pm[i] = v.pm[i]; qn[i] = v.qn[i]; }
  __syncthreads();
  float* out = n < 3 ? nullptr : v.lddt_res;
  unsigned long long tot_pres = 0ull, tot_part = 0ull, tot_opres = 0ull, tot_opart = 0ull;
  for (int i = r0 + g; i < r0 + n; i += groups) {
    int pres = 0, part = 0, opres = 0, opart = 0;
    for (int j = tid; j < nall; j += SC_THREADS) {
      if (j == i) continue;
      const double dn = score_dist(qn + 3 * i, qn + 3 * j);
      if (dn < 15.0) {
        const double e = fabs(score_dist(pm + 3 * i, pm + 3 * j) - dn);
        const int kept = (e < 0.5 ? 1 : 0) + (e < 1.0 ? 1 : 0) + (e < 2.0 ? 1 : 0) + (e < 4.0 ? 1 : 0);
        if (j >= r0 && j < r0 + n) { part += 1; pres += kept; }
        else { opart += 1; opres += kept; }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      pres += __shfl_xor(pres, off, 64);
      part += __shfl_xor(part, off, 64);
      opres += __shfl_xor(opres, off, 64);
      opart += __shfl_xor(opart, off, 64);
    }
    __syncthreads();
    if (lane == 0) { ired[wv][0] = pres; ired[wv][1] = part; ired[wv][2] = opres; ired[wv][3] = opart; }
    __syncthreads();
    if (tid == 0) {
      pres = part = opres = opart = 0;
      for (int k = 0; k < SC_WAVES; ++k) { pres += ired[k][0]; part += ired[k][1]; opres += ired[k][2]; opart += ired[k][3]; }
      if (out) out[v.idx[i]] = part > 0 ? (float)((double)pres / (4.0 * (double)part)) : 0.f;
      tot_pres += (unsigned long long)pres;
      tot_part += (unsigned long long)part;
      tot_opres += (unsigned long long)opres;
      tot_opart += (unsigned long long)opart;
    }
  }
  if (tid == 0) {
    __hip_atomic_fetch_add(&v.tot[0], tot_pres, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&v.tot[1], tot_part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v.outer) {
      __hip_atomic_fetch_add(&v.tot[2], tot_opres, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&v.tot[3], tot_opart, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(SC_THREADS) void score_lddt_kernel(ScoreArgs a) {
  extern __shared__ float sm[];
  score_lddt_body(score_view(a, blockIdx.y), blockIdx.x, gridDim.x, sm);
}

// ---------------------------------------------------------------------------------------
// score_search: one workgroup per seed
// ---------------------------------------------------------------------------------------
// Seed `seed` of the view's trace; at most `cap` seeds run (the launch's grid).  sm: 2 x 3n coordinates, then n flags: the set S.
__device__ inline void score_search_body(const ScoreView& v, int seed, int cap, float* sm) {
  __shared__ double wred[SC_WAVES][16];
  __shared__ double bc[12];              // R, t of this iteration (at the end: of the best seed)
  __shared__ int sh_last, sh_seed[SC_WAVES];
  const int n = v.n, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (n < 3) return;
  int nseeds = score_seeds(n);
  if (nseeds > cap) nseeds = cap;        // never: score_seeds does not decrease with n, the grid is score_seeds(L)
  if (seed >= nseeds) return;
  const double lnorm = v.hdr[HDR_LNORM], d0 = v.hdr[HDR_D0], d_cut = v.hdr[HDR_DCUT];
  // (level, start) of this seed
  int frag, start = seed;
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
  const float* gpm = v.pm + 3 * v.r0;
  const float* gqn = v.qn + 3 * v.r0;
  const int* gidx = v.idx + v.r0;
  double* grec = v.rec;
  unsigned* ticket = v.ticket;
  for (int i = tid; i < 3 * n; i += SC_THREADS) { pm[i] = gpm[i]; qn[i] = gqn[i]; }
  for (int k = tid; k < n; k += SC_THREADS) fl[k] = (k >= start && k < start + frag) ? 1 : 0;
  __syncthreads();

  // thread 0 keeps the seed's best
  SeedBest best;
  score_seed_loop(pm, qn, fl, n, lnorm, d0, d_cut, wred, bc, best);
  const double best_tm = best.tm, rmsd = best.rmsd;
  const double *best_R = best.R, *best_t = best.t, *best_cnt = best.cnt;

  if (tid == 0) {
    double* rec = grec + (int64_t)seed * SCORE_REC;
    agent_store_f64(rec + REC_TM, best_tm);
    for (int c = 0; c < 5; ++c) agent_store_f64(rec + REC_CNT + c, best_cnt[c]);
    for (int c = 0; c < 9; ++c) agent_store_f64(rec + REC_R + c, best_R[c]);
    for (int c = 0; c < 3; ++c) agent_store_f64(rec + REC_T + c, best_t[c]);
    agent_store_f64(rec + REC_RMSD, rmsd);
    sh_last = ticket_take_last(ticket, (unsigned)nseeds) ? 1 : 0;     // every record is behind its owner's release
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
    double* rec = grec + (int64_t)s * SCORE_REC;
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
    const float nan = __builtin_nanf("");
    const bool found = top_seed != 0x7fffffff;         // false only if every seed's tm is NaN
    double* rec = grec + (int64_t)(found ? top_seed : 0) * SCORE_REC;
    const float f_rmsd = (float)agent_load_f64(grec + REC_RMSD);
    const float f_tm = found ? (float)top : nan;
    const float f_ts = (float)((((cmax[1] + cmax[2]) + cmax[3]) + cmax[4]) / 4.0 / lnorm);
    const float f_ha = (float)((((cmax[0] + cmax[1]) + cmax[2]) + cmax[3]) / 4.0 / lnorm);
    const unsigned long long pres = v.tot[0], part = v.tot[1];         // score_lddt ran before this launch
    const float f_lddt = part > 0 ? (float)((double)pres / (4.0 * (double)part)) : 0.f;
    if (v.row) {                                       // a pass: its five scores into its row, nothing else
      float* row = v.row;
      row[2] = f_tm; row[3] = f_ts; row[4] = f_ha; row[5] = f_rmsd; row[6] = f_lddt;
      sh_last = 0;
    } else {
      float* out = v.head;                             // the header
      out[2] = f_rmsd; out[3] = f_tm; out[4] = f_ts; out[5] = f_ha; out[6] = f_lddt;
      for (int c = 0; c < 5; ++c) out[7 + c] = (float)cmax[c];
      for (int c = 0; c < 12; ++c) {
        const double w = agent_load_f64(rec + REC_R + c);
        bc[c] = w;
        out[12 + c] = found ? (float)w : nan;
      }
      sh_last = found ? 1 : 0;
    }
    ticket_reset(ticket);
  }
  __syncthreads();
  if (!sh_last) return;                                // the deviations stay NaN (a pass has none)
  double R[9], t[3];
  for (int c = 0; c < 9; ++c) R[c] = bc[c];
  for (int c = 0; c < 3; ++c) t[c] = bc[9 + c];
  for (int k = tid; k < n; k += SC_THREADS) v.dev[gidx[k]] = (float)score_dev(R, t, pm + 3 * k, qn + 3 * k);
}

__global__ __launch_bounds__(SC_THREADS) void score_search_kernel(ScoreArgs a) {
  extern __shared__ float sm[];
  score_search_body(score_view(a, blockIdx.y), blockIdx.x, gridDim.x, sm);
}

// ---------------------------------------------------------------------------------------
// the two scratches (common.h: Scratch): bytes from their start, every part 16-aligned
// ---------------------------------------------------------------------------------------
// A slot is one model trace's working set: the seed records, the packed trace, the lDDT totals.
struct PassSlot { int64_t rec, pm, tot, total; };
inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }
inline PassSlot pass_slot(int L) {
  PassSlot p;
  p.rec = 0;
  p.pm = up16(8 * (int64_t)SCORE_REC * score_seeds(L));
  p.tot = p.pm + up16(12 * (int64_t)L);
  p.total = p.tot + 16;
  return p;
}
// "score_native" (dmp_ctx::score_ws), sized for max_L.  The head: the search's ticket.  Then what score_prep packs once per call
// and "score_passes" reads back - the native rows, their alignment columns, the header - and one slot: the final model is a
// chunk of one.
constexpr int64_t SCORE_HEAD_BYTES = 16;
struct ScoreScratch { int64_t qn, idx, hdr, slot, total; };
inline ScoreScratch score_scratch(int max_L) {
  ScoreScratch w;
  w.qn = SCORE_HEAD_BYTES;
  w.idx = w.qn + up16(12 * (int64_t)max_L);
  w.hdr = w.idx + up16(4 * (int64_t)max_L);
  w.slot = w.hdr + 64;
  w.total = w.slot + pass_slot(max_L).total;
  return w;
}
// "score_passes" (dmp_ctx::pass_ws).  The head, at places that do not depend on L: PASS_MAX tickets of the search, PASS_MAX
// tickets of the delta; then the delta's partial sums [PASS_MAX][64]; then the slots of a chunk.
constexpr int64_t PASS_TICKET_BYTES = 2 * 4 * (int64_t)PASS_MAX;
constexpr int64_t PASS_HEAD_BYTES = PASS_TICKET_BYTES + 8 * 64 * (int64_t)PASS_MAX;
// passes per chunk: as many slots as the budget holds, 1 .. PASS_MAX; `cap` > 0 (option "score_passes_chunk") lowers it
inline int pass_chunk(int L, int cap) {
  int64_t C = PASS_BUDGET / pass_slot(L).total;
  C = C < 1 ? 1 : (C > PASS_MAX ? PASS_MAX : C);
  return cap > 0 && cap < C ? cap : (int)C;
}
ScratchNeed score_native_need(int max_L) { return {score_scratch(max_L).total, SCORE_HEAD_BYTES}; }
ScratchNeed score_passes_need(int max_L) {
  int64_t need = 0;
  for (int L = 8; L <= max_L; ++L) need = std::max<int64_t>(need, pass_chunk(L, 0) * pass_slot(L).total);
  return {PASS_HEAD_BYTES + need, PASS_TICKET_BYTES};
}

// The parts of a ScoreArgs that lie in the scratches: the native as score_prep packs it, and the slots from `slots` on, one
// per blockIdx.y.
static void score_scratch_args(const dmp_ctx* c, unsigned char* slots, const PassSlot& sl, unsigned* tickets, ScoreArgs& a) {
  const ScoreScratch w = score_scratch(c->max_L);
  a.qn = reinterpret_cast<float*>(c->score_ws.p + w.qn);
  a.idx = reinterpret_cast<int*>(c->score_ws.p + w.idx);
  a.hdr = reinterpret_cast<double*>(c->score_ws.p + w.hdr);
  a.rec = reinterpret_cast<double*>(slots + sl.rec);
  a.pm = reinterpret_cast<float*>(slots + sl.pm);
  a.tot = reinterpret_cast<unsigned long long*>(slots + sl.tot);
  a.ticket = tickets;
  a.rec_stride = sl.total / 8;
  a.pm_stride = sl.total / 4;
  a.tot_stride = sl.total / 8;
  a.ticket_stride = 1;
}

int score_native(dmp_ctx* c, const float* d_coords, int L, float* d_block, hipStream_t s) {
  ScoreArgs a{};
  a.model = d_coords + 3;
  a.model_row = 15;
  a.blk = d_block;
  a.L = L;
  score_scratch_args(c, c->score_ws.p + score_scratch(c->max_L).slot, pass_slot(c->max_L), reinterpret_cast<unsigned*>(c->score_ws.p), a);
  hipLaunchKernelGGL(score_prep_kernel, dim3(1), dim3(SC_THREADS), 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_lddt_kernel, dim3(score_lddt_groups(L)), dim3(SC_THREADS), sizeof(float) * 6 * L, s, a);
  DMP_LAUNCH_CHECK();
  // the slot's records hold score_seeds(max_L) >= score_seeds(L) seeds; 6L floats + L flags of LDS: 50 KB at L = 2048
  hipLaunchKernelGGL(score_search_kernel, dim3(score_seeds(L)), dim3(SC_THREADS), sizeof(float) * 6 * L + round_up(L, 16), s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// option "score_passes": the pass block (include/dmpfold_hip.h)
// ---------------------------------------------------------------------------------------
// pass_fill: what the block holds before the scores arrive.  Row p < rows: conf_mean, delta (+inf for pass 0; pass_deltas
// fills in the others), NaN in the five scores, zero; row p >= rows: NaN.  The header is pass_header's.
__global__ __launch_bounds__(SC_THREADS) void pass_fill_kernel(float* blk, int R, int rows, const float* conf_means) {
  const float nan = __builtin_nanf("");
  for (int i = threadIdx.x; i < pass_floats(R); i += SC_THREADS) {
    float v = 0.f;
    if (i >= PASS_HEADER) {
      const int p = (i - PASS_HEADER) / PASS_ROW, q = (i - PASS_HEADER) % PASS_ROW;
      v = p >= rows ? nan : q == 0 ? conf_means[p] : q == 1 ? (p == 0 ? __builtin_inff() : nan) : q == 7 ? 0.f : nan;
    }
    blk[i] = v;
  }
}

// pass_header: one thread reads the finished rows in pass order (at most 128 of them)
__global__ void pass_header_kernel(float* blk, int rows, const float* best_pass) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float nan = __builtin_nanf("");
  const float* row = blk + PASS_HEADER;
  const float bp = best_pass[0];
  const int b = bp < (float)PASS_MAX ? (int)bp : -1;   // best_pass < passes_run, so a pass below the cap has a row
  blk[0] = (float)rows;
  blk[1] = bp;
  for (int q = 0; q < 2; ++q) {                        // tm (offset 2 of a row), then lddt (offset 6)
    const int o = q == 0 ? 2 : 6;
    int top = -1;
    for (int p = 0; p < rows; ++p) {
      const float v = row[PASS_ROW * p + o];
      if (v == v && (top < 0 || v > row[PASS_ROW * top + o])) top = p;       // strict: the lowest of equals stays
    }
    blk[2 + q] = top < 0 ? nan : (float)top;
    const float vb = b >= 0 && b < rows ? row[PASS_ROW * b + o] : nan;
    blk[4 + q] = top >= 0 && vb == vb ? row[PASS_ROW * top + o] - vb : nan;
  }
}

int score_passes(dmp_ctx* c, int L, int R, int rows, float* d_block, hipStream_t s) {
  unsigned* tickets = reinterpret_cast<unsigned*>(c->pass_ws.p);
  double* partial = reinterpret_cast<double*>(c->pass_ws.p + PASS_TICKET_BYTES);
  float* d_rows = d_block + PASS_HEADER;
  hipLaunchKernelGGL(pass_fill_kernel, dim3(1), dim3(SC_THREADS), 0, s, d_block, R, rows, c->conf_means);
  DMP_LAUNCH_CHECK();
  int rc = pass_deltas(c, L, rows, d_rows, partial, tickets + PASS_MAX, s);
  if (rc) return rc;
  const int C = pass_chunk(L, c->run.passes_chunk);
  ScoreArgs a{};
  a.model_row = 3;
  a.model_stride = 3 * (int64_t)L;
  a.L = L;
  score_scratch_args(c, c->pass_ws.p + PASS_HEAD_BYTES, pass_slot(L), tickets, a);      // (the native: score_native of this call left it)
  for (int p0 = 0; p0 < rows; p0 += C) {               // the chunks reuse the slots: the stream orders them
    const int np = std::min(C, rows - p0);
    a.model = c->ca_pass + (int64_t)p0 * 3 * L;
    a.rows = d_rows + PASS_ROW * (int64_t)p0;
    hipLaunchKernelGGL(score_pass_prep_kernel, dim3(cdiv(L, SC_THREADS), np), dim3(SC_THREADS), 0, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_lddt_kernel, dim3(score_lddt_groups(L), np), dim3(SC_THREADS), sizeof(float) * 6 * L, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_search_kernel, dim3(score_seeds(L), np), dim3(SC_THREADS), sizeof(float) * 6 * L + round_up(L, 16), s, a);
    DMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pass_header_kernel, dim3(1), dim3(64), 0, s, d_block, rows, c->best_pass);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// option "score_domains": the domain-score block (include/dmpfold_hip.h)
// ---------------------------------------------------------------------------------------
// Four launches behind `domains`, a leg (0: the model's labels, 1: the native's) as the slot of a ScoreArgs:
//   domscore_prep    one workgroup per leg: the labels of both legs validated as domsearch_prep does (align.hip); the leg's part
//                    of the block filled; the present rows packed in (domain, column) order - model from d_coords, native from
//                    the score block -, and per domain its header (n, lnorm = n, d0, d_cut), its first packed row and its
//                    first seed: the prefix sums of the <= 16 row counts and seed counts.
//   domscore_lddt    score_lddt_body, (row group, domain, leg): the pairs inside the domain and the pairs that leave it.
//   domscore_search  score_search_body on a flat grid of Dmax + 5L workgroups per leg (score_seeds(n) <= 1 + 5n and the domains
//                    partition the chain): a workgroup finds its (domain, seed) in the prefix sums; each domain has its ticket
//                    and its stretch of the leg's records.
//   domscore_counts  the four integer counts of every row.
// Nothing here reads what score_native left in score_ws.
constexpr int DS_D = 0, DS_ROW0 = 1, DS_SEED0 = 1 + DOMAINS_MAX + 1, DS_INFO = 64;     // ints of a leg's info: D (0: no such leg),
                                                                                       // 17 first rows, 17 first seeds
constexpr int64_t DOMSCORE_HEAD_BYTES = 4 * 2 * DOMAINS_MAX;                           // the tickets [leg][domain]
struct DomScoreScratch { int64_t info, hdr, tot, qn, pm, idx, rec, leg, total; };      // bytes; a leg's parts from the leg's start
inline DomScoreScratch domscore_scratch(int max_L) {
  DomScoreScratch w;
  w.info = 0;
  w.hdr = w.info + up16(4 * DS_INFO);
  w.tot = w.hdr + 64 * DOMAINS_MAX;
  w.qn = w.tot + 32 * DOMAINS_MAX;
  w.pm = w.qn + up16(12 * (int64_t)max_L);
  w.idx = w.pm + up16(12 * (int64_t)max_L);
  w.rec = w.idx + up16(4 * (int64_t)max_L);
  w.leg = w.rec + up16(8 * (int64_t)SCORE_REC * (DOMAINS_MAX + 5 * (int64_t)max_L));
  w.total = DOMSCORE_HEAD_BYTES + 2 * w.leg;
  return w;
}
ScratchNeed score_domains_need(int max_L) { return {domscore_scratch(max_L).total, DOMSCORE_HEAD_BYTES}; }

// domain d of leg `leg`
__device__ inline ScoreView domscore_view(const ScoreArgs& a, int leg, int d) {
  const int* info = a.info + leg * a.idx_stride;
  const DomScoreLayout lay = domscore_layout(a.L);
  ScoreView v;
  v.pm = a.pm + leg * a.pm_stride;
  v.qn = a.qn + leg * a.qn_stride;
  v.idx = a.idx + leg * a.idx_stride;
  v.hdr = a.hdr + leg * a.hdr_stride + 8 * d;
  v.rec = a.rec + leg * a.rec_stride + (int64_t)SCORE_REC * info[DS_SEED0 + d];
  v.tot = a.tot + leg * a.tot_stride + 4 * d;
  v.ticket = a.ticket + leg * a.ticket_stride + d;
  v.r0 = info[DS_ROW0 + d];
  v.n = info[DS_ROW0 + d + 1] - v.r0;
  v.nall = info[DS_ROW0 + info[DS_D]];
  v.outer = true;
  v.head = a.dom + lay.rows + DOMSCORE_ROW * (DOMAINS_MAX * leg + d);
  v.row = nullptr;
  v.lddt_res = a.dom + lay.res + 2 * (int64_t)a.L * leg;
  v.dev = v.lddt_res + a.L;
  return v;
}

// D and the labels of one leg of the domain block (labels at `lab`): D if they are valid, 0 if not.  Every thread calls it;
// lab8 [L] gets the labels, 0xff for an invalid one.
__device__ inline int domscore_labels(float Df, const float* lab, int L, int dmax, unsigned char* lab8, int* bad) {
  const int tid = threadIdx.x;
  const int D = Df >= 1.f && Df <= (float)dmax && Df <= (float)DOMAINS_MAX && Df == floorf(Df) ? (int)Df : 0;      // a NaN fails the comparisons
  int mine = 0;
  for (int i = tid; i < L; i += SC_THREADS) {
    const float lf = lab[i];
    const bool ok = lf >= 0.f && lf < (float)D && lf == floorf(lf);
    mine |= ok ? 0 : 1;
    lab8[i] = ok ? (unsigned char)lf : (unsigned char)0xff;
  }
  __syncthreads();                        // (bad[] of the call before has been read)
  bad[tid] = mine;
  __syncthreads();
  int any = 0;
  for (int k = 0; k < SC_THREADS; ++k) any |= bad[k];
  return any ? 0 : D;
}

__global__ __launch_bounds__(SC_THREADS) void domscore_prep_kernel(ScoreArgs a, const float* dblk, int dmax) {
  __shared__ unsigned char lab[DMP_MAX_L], other[DMP_MAX_L];
  __shared__ int bad[SC_THREADS], cnt[DOMAINS_MAX], size[DOMAINS_MAX], row0[DOMAINS_MAX + 1];
  const int tid = threadIdx.x, leg = blockIdx.x, L = a.L < DMP_MAX_L ? a.L : DMP_MAX_L;
  const DomScoreLayout lay = domscore_layout(a.L);
  const float nan = __builtin_nanf("");
  int* info = a.info + leg * a.idx_stride;
  // both workgroups judge both legs: the model's must be valid; the native's valid, or absent (its D is 0)
  const int D0 = domscore_labels(dblk[0], dblk + DOMAINS_HEADER, L, dmax, leg == 0 ? lab : other, bad);
  const float D1f = dblk[DOMAINS_HEADER / 2];
  const int D1 = D1f == 0.f ? 0 : domscore_labels(D1f, dblk + DOMAINS_HEADER + a.L, L, dmax, leg == 1 ? lab : other, bad);
  const bool valid = D0 > 0 && (D1f == 0.f || D1 > 0);
  const int D = valid ? (leg == 0 ? D0 : D1) : 0;
  __syncthreads();
  if (tid < DOMAINS_MAX) {                // rows present and residues of domain tid
    int n = 0, sz = 0;
    for (int i = 0; i < L; ++i)
      if (tid < D && lab[i] == tid) {
        const float x = a.blk[3 * i];
        sz += 1;
        n += x == x ? 1 : 0;
      }
    cnt[tid] = n;
    size[tid] = sz;
  }
  __syncthreads();
  if (tid == 0) {
    int rows = 0, seeds = 0;
    info[DS_D] = D;
    for (int d = 0; d < DOMAINS_MAX; ++d) {
      const int n = cnt[d];
      row0[d] = rows;
      info[DS_ROW0 + d] = rows;
      info[DS_SEED0 + d] = seeds;
      rows += n;
      seeds += n < 3 ? 0 : score_seeds(n);           // at most D + 5 (rows of the leg) <= dmax + 5L: the grid, and the records
      const double lnorm = (double)n, d0 = score_d0(lnorm);
      double* hdr = a.hdr + leg * a.hdr_stride + 8 * d;
      hdr[HDR_N] = lnorm;
      hdr[HDR_LNORM] = lnorm;
      hdr[HDR_D0] = d0;
      hdr[HDR_DCUT] = fmin(fmax(d0, 4.5), 8.0);
      unsigned long long* tot = a.tot + leg * a.tot_stride + 4 * d;
      tot[0] = tot[1] = tot[2] = tot[3] = 0ull;
    }
    row0[DOMAINS_MAX] = rows;
    info[DS_ROW0 + DOMAINS_MAX] = rows;
    info[DS_SEED0 + DOMAINS_MAX] = seeds;
  }
  __syncthreads();
  // the leg's part of the block: its header words, its table, its two arrays
  if (leg == 0)
    for (int i = tid; i < DOMSCORE_HEADER; i += SC_THREADS)
      a.dom[i] = !valid ? nan : i == 0 ? (float)D0 : i == 1 ? (float)D1 : i == 2 ? (float)row0[DOMAINS_MAX] : 0.f;
  float* rows = a.dom + lay.rows + DOMSCORE_ROW * DOMAINS_MAX * leg;
  for (int i = tid; i < DOMSCORE_ROW * DOMAINS_MAX; i += SC_THREADS) {
    const int d = i / DOMSCORE_ROW, q = i % DOMSCORE_ROW;
    rows[i] = d >= D ? nan : q <= 1 ? (float)cnt[d] : q < 24 ? nan : q == 28 ? (float)size[d] : 0.f;      // 24 .. 27: domscore_counts
  }
  float* res = a.dom + lay.res + 2 * (int64_t)a.L * leg;
  for (int i = tid; i < 2 * a.L; i += SC_THREADS) res[i] = nan;
  if (tid < D) {                          // the present rows of domain tid, in rising column
    int at = row0[tid];
    float* pm = a.pm + leg * a.pm_stride;
    float* qn = a.qn + leg * a.qn_stride;
    int* idx = a.idx + leg * a.idx_stride;
    for (int i = 0; i < L; ++i) {
      if (lab[i] != tid) continue;
      const float x = a.blk[3 * i];
      if (x != x) continue;
      for (int c = 0; c < 3; ++c) {      // at < row0[tid + 1] <= L: the same rows were counted
        pm[3 * at + c] = a.model[a.model_row * (int64_t)i + c];
        qn[3 * at + c] = a.blk[3 * i + c];
      }
      idx[at] = i;
      ++at;
    }
  }
}

__global__ __launch_bounds__(SC_THREADS) void domscore_lddt_kernel(ScoreArgs a) {
  extern __shared__ float sm[];
  const int leg = blockIdx.z, d = blockIdx.y;
  if (d >= a.info[leg * a.idx_stride + DS_D]) return;                  // uniform
  score_lddt_body(domscore_view(a, leg, d), blockIdx.x, gridDim.x, sm);
}

__global__ __launch_bounds__(SC_THREADS) void domscore_search_kernel(ScoreArgs a) {
  extern __shared__ float sm[];
  const int leg = blockIdx.y, b = blockIdx.x;
  const int* info = a.info + leg * a.idx_stride;
  const int D = info[DS_D];
  if (D == 0 || b >= info[DS_SEED0 + D]) return;                       // uniform
  int d = 0;
  while (d < D - 1 && b >= info[DS_SEED0 + d + 1]) ++d;
  score_search_body(domscore_view(a, leg, d), b - info[DS_SEED0 + d], info[DS_SEED0 + d + 1] - info[DS_SEED0 + d], sm);
}

__global__ void domscore_counts_kernel(ScoreArgs a) {
  const int leg = threadIdx.x / DOMAINS_MAX, d = threadIdx.x % DOMAINS_MAX;
  if (leg >= 2 || d >= a.info[leg * a.idx_stride + DS_D]) return;
  const unsigned long long* tot = a.tot + leg * a.tot_stride + 4 * d;
  float* row = a.dom + domscore_layout(a.L).rows + DOMSCORE_ROW * (DOMAINS_MAX * leg + d);
  for (int c = 0; c < 4; ++c) row[24 + c] = (float)tot[c];
}

int score_domains(dmp_ctx* c, const float* d_coords, int L, float* d_score_block, const float* d_domain_block, float* d_block, hipStream_t s) {
  const DomScoreScratch w = domscore_scratch(c->max_L);
  unsigned char* leg0 = c->domscore_ws.p + DOMSCORE_HEAD_BYTES;
  const int dmax = std::max(1, std::min(DOMAINS_MAX, L / c->run.dom_min_size));
  ScoreArgs a{};
  a.model = d_coords + 3;
  a.model_row = 15;
  a.blk = d_score_block;                 // only its native trace is read
  a.L = L;
  a.dom = d_block;
  a.info = reinterpret_cast<int*>(leg0 + w.info);
  a.hdr = reinterpret_cast<double*>(leg0 + w.hdr);
  a.tot = reinterpret_cast<unsigned long long*>(leg0 + w.tot);
  a.qn = reinterpret_cast<float*>(leg0 + w.qn);
  a.pm = reinterpret_cast<float*>(leg0 + w.pm);
  a.idx = reinterpret_cast<int*>(leg0 + w.idx);
  a.rec = reinterpret_cast<double*>(leg0 + w.rec);
  a.ticket = reinterpret_cast<unsigned*>(c->domscore_ws.p);
  a.pm_stride = a.qn_stride = a.idx_stride = w.leg / 4;
  a.hdr_stride = a.rec_stride = a.tot_stride = w.leg / 8;
  a.ticket_stride = DOMAINS_MAX;
  hipLaunchKernelGGL(domscore_prep_kernel, dim3(2), dim3(SC_THREADS), 0, s, a, d_domain_block, dmax);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domscore_lddt_kernel, dim3(score_lddt_groups(L), dmax, 2), dim3(SC_THREADS), sizeof(float) * 6 * L, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domscore_search_kernel, dim3(dmax + 5 * L, 2), dim3(SC_THREADS), sizeof(float) * 6 * L + round_up(L, 16), s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domscore_counts_kernel, dim3(1), dim3(64), 0, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
