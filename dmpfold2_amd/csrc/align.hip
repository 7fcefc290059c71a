// option "align_structure": the final C-alpha trace aligned with a structure of any length and sequence (include/dmpfold_hip.h
// has the layout of the align block and the definition of every number).  Three launches in dmp_predict_end behind score_native:
//   align_prep    one workgroup: m validated, both traces packed (model from d_coords[:, 1], structure from the block), the
//                 constants; NaN into every out slot.
//   align_thread  stage 1, one workgroup per gapless threading (offset k): the shrinking-set loop of score_common.h on the
//                 overlap, one record (tm) per seed; the last arriver (agent-scope ticket, common.h) ranks the records and
//                 writes the AL_T survivors.
//   align_refine  stage 2, one workgroup per survivor: superposition, dynamic programme as an anti-diagonal wavefront
//                 (three rotating diagonals of H and of the diag flag in LDS, one barrier per diagonal, the directions one
//                 byte per cell in a per-workgroup scratch in global memory), serial traceback, until the alignment
//                 repeats; the last arriver picks the winner and writes the header, ali and the deviations.
// Option "search_structures" runs the same three stages over the K entries of a library, the entry as blockIdx.y, in chunks of
// as many entries as the scratch budget holds, between search_prep (lengths validated, trace offsets, NaN fill) and search_rank.
// Option "search_refine" = R makes that two passes: stage 1 and align_screen over every entry, search_select, the three stages
// over the R entries chosen.  Option "search_domains" runs the same passes once more with every domain of the model as the model: the
// bodies take the model's row count n from the slot header (AH_N); a.L is only the bound that sizes strides, LDS and grids.
// Both searches go through one frame, templates over a query (WholeQuery, DomainQuery): search_pair, search_align_{prep,thread,
// refine,screen}_kernel, search_select_kernel, search_rank_kernel, and search_passes on the host.
// Float64 from the float32 coordinates, contraction off, every sum in the fixed order of score_block_sum; every candidate
// of a DP cell is one float64 add of two defined values, so H does not depend on the order the cells are evaluated in.
// Every loop is bounded whatever the input holds, and every branch with a barrier inside is uniform over the workgroup.
#include "score_common.h"

namespace dmp {

constexpr int AL_T = ALIGN_SURVIVORS;   // seeds refined
constexpr int AL_ROUNDS = 10;           // superposition / DP rounds per survivor
constexpr int AL_SLICE = (DMP_MAX_L + 1 + SC_THREADS - 1) / SC_THREADS;   // rows i = tid + 256 k of a diagonal per thread
constexpr double AL_GAP = -0.6;         // added to a gap step that follows a diag step
// header of the scratch
constexpr int AH_VALID = 0, AH_N = 1, AH_M = 2, AH_LMIN = 3, AH_MINOV = 4, AH_SEEDS = 5, AH_D0S = 6, AH_DCUT = 7;

__device__ __forceinline__ void agent_store_i32(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int agent_load_i32(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct AlignArgs {
  const float* coords;   // [L][5][3] the backbone; the model trace is atom 1
  float mf;              // m as the caller wrote it (a float; validated in align_prep)
  float* out;            // [ALIGN_HEADER] the header: out[c - 1] is offset c of an align block
  float* ali;            // [L], then deviation [L]
  const float* trace;    // [m][3] the structure's trace (in)
  int L, max_m;          // max_m: the bound on m (the context's max_L; "search_max_m" in a search)
  size_t dir_stride, bali_stride;   // per survivor: bytes of `dir`, ints of `bali`
  float* pm;             // [L][3] model trace
  float* qs;             // [m][3] structure trace
  double* hdr;           // [8]
  double* rec;           // [L + max_m + 1] tm of every seed of stage 1
  int* surv;             // [1 + AL_T] how many survivors, their seed numbers in rank order
  double* btm;           // [AL_T] stage 2: a survivor's best tm ...
  int* bali;             // [AL_T][bali_stride >= 1 + 2 min(L, max_m)] ... and its alignment: K, then K pairs (i, j)
  unsigned char* dir;    // [AL_T][dir_stride >= (L + 1)(max_m + 1)] directions of the DP in flight, one byte per cell
  unsigned* ticket;      // [2] stage 1, stage 2: zero between launches
};

// What of an AlignArgs lies in a scratch: the parts of the slot at `sl` (common.h: search_slot(L, max_m)) and its two tickets.
// "align_structure" fills its one on the host, "search_structures" one per entry on the device.
__host__ __device__ inline void align_slot_args(AlignArgs& a, unsigned char* sl, const SearchSlot& slot, int L, int max_m, unsigned* tickets) {
  a.L = L;
  a.max_m = max_m;
  a.dir_stride = (size_t)(L + 1) * (size_t)(max_m + 1);
  a.bali_stride = (size_t)(1 + 2 * L);
  a.pm = reinterpret_cast<float*>(sl + slot.pm);
  a.qs = reinterpret_cast<float*>(sl + slot.qs);
  a.hdr = reinterpret_cast<double*>(sl + slot.hdr);
  a.rec = reinterpret_cast<double*>(sl + slot.rec);
  a.surv = reinterpret_cast<int*>(sl + slot.surv);
  a.btm = reinterpret_cast<double*>(sl + slot.btm);
  a.bali = reinterpret_cast<int*>(sl + slot.bali);
  a.dir = sl + slot.dir;
  a.ticket = tickets;
}

// ---------------------------------------------------------------------------------------
// align_prep
// ---------------------------------------------------------------------------------------
// The three kernels' bodies are device functions of one AlignArgs: the single-partner launches pass theirs as the kernel
// argument, the search launches of options "search_structures" and "search_domains" form one per pair (blockIdx.y) from the
// search block and the pair's slot - the same code either way, so an entry's floats are "align_structure"'s bit for bit.
// The structure half: NaN into the header, m validated, the structure's trace packed.  This thread's share of "a coordinate is
// NaN" comes back; m (0 if invalid) and m_ok go out.
__device__ __forceinline__ int align_prep_structure(const AlignArgs& a, int& m, bool& m_ok) {
  const int tid = threadIdx.x;
  const float nan = __builtin_nanf("");
  for (int i = tid; i < ALIGN_HEADER; i += SC_THREADS) a.out[i] = nan;
  const float mf = a.mf;
  m_ok = mf >= 3.f && mf <= (float)a.max_m && mf == floorf(mf);                 // a NaN fails the comparisons
  m = m_ok ? (int)mf : 0;                                                        // 0: nothing beyond [0] is read
  int mine = 0;
  for (int i = tid; i < 3 * m; i += SC_THREADS) {
    const float x = a.trace[i];
    mine |= x != x ? 1 : 0;
    a.qs[i] = x;
  }
  return mine;
}
// The model half: the n rows row(0) < row(1) < ... of the backbone are the model - all L of them, or the residues of one domain
// (option "search_domains") - packed into pm; NaN into their ali and deviation (a.ali[i], a.ali[a.L + i], i < n: a.L is the
// stride, n the rows).  Then the scratch header, n in it: every stage reads the model's row count from there.
template <class Row>
__device__ __forceinline__ void align_prep_body(const AlignArgs& a, int n, Row row) {
  __shared__ int bad[SC_THREADS];
  const int L = a.L, tid = threadIdx.x;
  const float nan = __builtin_nanf("");
  int m;
  bool m_ok;
  const int mine = align_prep_structure(a, m, m_ok);
  for (int i = tid; i < n; i += SC_THREADS) a.ali[i] = a.ali[L + i] = nan;
  for (int i = tid; i < 3 * n; i += SC_THREADS) a.pm[i] = a.coords[15 * (int64_t)row(i / 3) + 3 + i % 3];
  bad[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int any = 0;
    for (int k = 0; k < SC_THREADS; ++k) any |= bad[k];
    const int lmin = n < m ? n : m;
    const int minov = lmin / 2 > (lmin < 5 ? lmin : 5) ? lmin / 2 : (lmin < 5 ? lmin : 5);
    const double d0s = score_d0((double)lmin);
    a.hdr[AH_VALID] = m_ok && !any ? 1.0 : 0.0;
    a.hdr[AH_N] = (double)n;
    a.hdr[AH_M] = (double)m;
    a.hdr[AH_LMIN] = (double)lmin;
    a.hdr[AH_MINOV] = (double)minov;
    a.hdr[AH_SEEDS] = (double)(n + m - 2 * minov + 1);
    a.hdr[AH_D0S] = d0s;
    a.hdr[AH_DCUT] = fmin(fmax(d0s, 4.5), 8.0);
    a.surv[0] = 0;
  }
}
// the whole chain as the model
__device__ __forceinline__ void align_prep_body(const AlignArgs& a) {
  align_prep_body(a, a.L, [](int i) { return i; });
}

// the pairs of seed s: (i0 + t, i0 + k + t), t < ov
__device__ inline void align_seed(int s, int n, int m, int minov, int& k, int& i0, int& ov) {
  k = s - (n - minov);
  i0 = k < 0 ? -k : 0;
  ov = (n < m - k ? n : m - k) - i0;
}

// ---------------------------------------------------------------------------------------
// align_thread: stage 1, one workgroup per offset
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void align_thread_body(const AlignArgs& a) {
  extern __shared__ float sm[];          // 2 x 3 ov coordinates, then ov flags
  __shared__ double wred[SC_WAVES][16];
  __shared__ double bc[12];
  __shared__ int sh_last, sh_seed[SC_WAVES], sh_chosen[AL_T], sh_found;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.hdr[AH_VALID] == 0.0) return;
  const int n = (int)a.hdr[AH_N], m = (int)a.hdr[AH_M], minov = (int)a.hdr[AH_MINOV];
  int nseeds = (int)a.hdr[AH_SEEDS];
  if (nseeds > (int)gridDim.x) nseeds = (int)gridDim.x;      // never: the grid is L + max_m + 1 >= n + m - 2 minov + 1
  if ((int)blockIdx.x >= nseeds) return;
  const double lmin = a.hdr[AH_LMIN], d0s = a.hdr[AH_D0S], d_cut = a.hdr[AH_DCUT];
  int k, i0, ov;
  align_seed((int)blockIdx.x, n, m, minov, k, i0, ov);
  float* pm = sm;
  float* qn = sm + 3 * ov;
  unsigned char* fl = reinterpret_cast<unsigned char*>(sm + 6 * ov);
  for (int i = tid; i < 3 * ov; i += SC_THREADS) { pm[i] = a.pm[3 * i0 + i]; qn[i] = a.qs[3 * (i0 + k) + i]; }
  for (int t = tid; t < ov; t += SC_THREADS) fl[t] = 1;
  __syncthreads();
  SeedBest best;
  score_seed_loop(pm, qn, fl, ov, lmin, d0s, d_cut, wred, bc, best);
  if (tid == 0) {
    agent_store_f64(a.rec + blockIdx.x, best.tm);
    sh_last = ticket_take_last(a.ticket, (unsigned)nseeds) ? 1 : 0;
    if (sh_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!sh_last) return;

  // the last arriver: the AL_T best seeds in rank order (ties: the lower number), one maximum search per rank
  for (int r = 0; r < AL_T; ++r) {
    double top = -__builtin_inf();
    int top_seed = 0x7fffffff;
    for (int s = tid; s < nseeds; s += SC_THREADS) {
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= sh_chosen[q] == s;
      const double tm = agent_load_f64(a.rec + s);
      if (!taken && tm > top) { top = tm; top_seed = s; }      // s rises: the first of equals stays; a NaN is never taken
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double o_top = __shfl_xor(top, off, 64);
      const int o_seed = __shfl_xor(top_seed, off, 64);
      if (o_top > top || (o_top == top && o_seed < top_seed)) { top = o_top; top_seed = o_seed; }
    }
    __syncthreads();
    if (lane == 0) { wred[wv][0] = top; sh_seed[wv] = top_seed; }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < SC_WAVES; ++q)
        if (wred[q][0] > top || (wred[q][0] == top && sh_seed[q] < top_seed)) { top = wred[q][0]; top_seed = sh_seed[q]; }
      sh_found = top_seed != 0x7fffffff ? 1 : 0;
      if (sh_found) {
        sh_chosen[r] = top_seed;
        a.surv[1 + r] = top_seed;
        a.surv[0] = r + 1;
      }
    }
    __syncthreads();
    if (!sh_found) break;                // uniform: fewer than AL_T seeds (or nothing but NaN left)
  }
  if (tid == 0) ticket_reset(a.ticket);
}

// ---------------------------------------------------------------------------------------
// align_refine: stage 2, one workgroup per survivor
// ---------------------------------------------------------------------------------------
// LDS of align_refine in bytes: three diagonals of H, then what the superposition (2 x 3L floats, L flags) and the dynamic
// programme (the structure's 3 max_m floats, three diagonals of the flag) use in turn, then three pair lists of L (i, j).
struct AlignLds { int un, lists, total; };
__host__ __device__ inline AlignLds align_lds(int L, int max_m) {
  const int h = 3 * (L + 1) * 8;
  const int sup = 24 * L + L, dp = 12 * max_m + 3 * (L + 1);
  const int un = ((sup > dp ? sup : dp) + 7) / 8 * 8;
  return {h, h + un, h + un + 3 * 2 * L * 2};
}

// K packed pairs (pi(t), pj(t)) into pm2 / qn2, the flags set: the start of a superposition
template <class PairI, class PairJ>
__device__ inline void align_pack(const AlignArgs& a, PairI pi, PairJ pj, int K, float* pm2, float* qn2, unsigned char* fl) {
  for (int t = threadIdx.x; t < K; t += SC_THREADS) {
    const int i = pi(t), j = pj(t);
    for (int c = 0; c < 3; ++c) { pm2[3 * t + c] = a.pm[3 * i + c]; qn2[3 * t + c] = a.qs[3 * j + c]; }
    fl[t] = 1;
  }
  __syncthreads();
}

// The outputs of one alignment - wK pairs (pi(t), pj(t)) that grew from seed number `seed` - by the final formulae of the header
// file: the two superpositions, the header, ali and the deviations.  The one definition of align_refine's winner and of a
// screened entry's gapless alignment (`screened`: offset 21 of the header, 1 = "screened, not refined").  The whole workgroup
// calls it; pm2 / qn2 / fl hold 3 wK, 3 wK floats and wK flags.
template <class PairI, class PairJ>
__device__ __forceinline__ void align_finish(const AlignArgs& a, PairI pi, PairJ pj, int wK, int seed, float screened, int n, int m,
                                             int minov, double d_cut, float* pm2, float* qn2, unsigned char* fl,
                                             double (*wred)[16], double* bc) {
  const int tid = threadIdx.x, L = a.L;                      // L: the stride between ali and deviation; the model has n rows
  const double d0n = score_d0((double)n), d0m = score_d0((double)m);
  align_pack(a, pi, pj, wK, pm2, qn2, fl);
  SeedBest bn;
  score_seed_loop(pm2, qn2, fl, wK, (double)n, d0n, d_cut, wred, bc, bn);
  __syncthreads();
  for (int t = tid; t < wK; t += SC_THREADS) fl[t] = 1;
  __syncthreads();
  SeedBest bm;
  score_seed_loop(pm2, qn2, fl, wK, (double)m, d0m, d_cut, wred, bc, bm);
  if (tid == 0) {
    float* out = a.out - 1;                                  // out[c]: offset c of an align block
    int k, i0, ov;
    align_seed(seed, n, m, minov, k, i0, ov);
    out[1] = (float)wK;
    out[2] = (float)bn.rmsd;
    out[3] = (float)bn.tm;
    out[4] = (float)bm.tm;
    for (int c = 0; c < 9; ++c) { out[5 + c] = (float)bm.R[c]; bc[c] = bm.R[c]; }
    for (int c = 0; c < 3; ++c) { out[14 + c] = (float)bm.t[c]; bc[9 + c] = bm.t[c]; }
    out[17] = (float)d0n;
    out[18] = (float)d0m;
    out[19] = (float)k;
    out[20] = (float)a.hdr[AH_SEEDS];
    out[21] = screened;
    for (int c = 22; c < ALIGN_HEADER + 1; ++c) out[c] = 0.f;
  }
  for (int i = tid; i < n; i += SC_THREADS) a.ali[i] = -1.f;      // (the deviations of these rows stay NaN)
  __syncthreads();
  double R[9], tr[3];
  for (int c = 0; c < 9; ++c) R[c] = bc[c];
  for (int c = 0; c < 3; ++c) tr[c] = bc[9 + c];
  for (int t = tid; t < wK; t += SC_THREADS) {
    const int i = pi(t);
    a.ali[i] = (float)pj(t);
    a.ali[L + i] = (float)score_dev(R, tr, pm2 + 3 * t, qn2 + 3 * t);
  }
}

__device__ __forceinline__ void align_refine_body(const AlignArgs& a) {
  extern __shared__ double smd[];
  __shared__ double wred[SC_WAVES][16];
  __shared__ double bc[12];
  __shared__ int sh_flag, sh_K, sh_off, sh_diff, sh_last, sh_win;
  const int tid = threadIdx.x, L = a.L;
  if (a.hdr[AH_VALID] == 0.0) return;
  const int nsurv = a.surv[0];
  if ((int)blockIdx.x >= nsurv) return;                      // (no survivor at all: the out slots stay NaN)
  const int n = (int)a.hdr[AH_N], m = (int)a.hdr[AH_M], minov = (int)a.hdr[AH_MINOV];
  const double lmin = a.hdr[AH_LMIN], d0s = a.hdr[AH_D0S], d_cut = a.hdr[AH_DCUT];
  const AlignLds lds = align_lds(L, a.max_m);
  unsigned char* base = reinterpret_cast<unsigned char*>(smd);
  double* Hb = smd;                                          // [3][L + 1]
  float* pm2 = reinterpret_cast<float*>(base + lds.un);      // superposition: [K][3], [K][3], [K]
  float* qn2 = pm2 + 3 * L;
  unsigned char* fl = reinterpret_cast<unsigned char*>(qn2 + 3 * L);
  float* qs = reinterpret_cast<float*>(base + lds.un);       // dynamic programme: [m][3], [3][L + 1]
  unsigned char* Db = reinterpret_cast<unsigned char*>(qs + 3 * a.max_m);
  unsigned short* lst = reinterpret_cast<unsigned short*>(base + lds.lists);
  unsigned short *ci = lst, *cj = lst + L, *ni = lst + 2 * L, *nj = lst + 3 * L, *bi = lst + 4 * L, *bj = lst + 5 * L;
  unsigned char* dirp = a.dir + (size_t)blockIdx.x * a.dir_stride;
  const int seed = a.surv[1 + blockIdx.x];

  int K, coff = 0, bK = 0;                                   // the alignment in hand: K pairs from ci / cj [coff]
  {
    int k, i0;
    align_seed(seed, n, m, minov, k, i0, K);
    for (int t = tid; t < K; t += SC_THREADS) { ci[t] = (unsigned short)(i0 + t); cj[t] = (unsigned short)(i0 + k + t); }
  }
  __syncthreads();
  double best_tm = -1.0;                                     // thread 0

  for (int round = 0; round < AL_ROUNDS; ++round) {
    {
      const unsigned short *li = ci + coff, *lj = cj + coff;
      align_pack(a, [li](int t) { return (int)li[t]; }, [lj](int t) { return (int)lj[t]; }, K, pm2, qn2, fl);
    }
    SeedBest sb;
    score_seed_loop(pm2, qn2, fl, K, lmin, d0s, d_cut, wred, bc, sb);
    if (tid == 0) {
      sh_flag = sb.tm > best_tm ? 1 : 0;
      if (sh_flag) best_tm = sb.tm;
      for (int c = 0; c < 9; ++c) bc[c] = sb.R[c];
      for (int c = 0; c < 3; ++c) bc[9 + c] = sb.t[c];
    }
    __syncthreads();
    if (sh_flag) {
      for (int t = tid; t < K; t += SC_THREADS) { bi[t] = ci[coff + t]; bj[t] = cj[coff + t]; }
      bK = K;
    }
    if (round == AL_ROUNDS - 1) break;                       // the alignment a further DP gave would never be scored
    double R[9], tr[3];
    for (int c = 0; c < 9; ++c) R[c] = bc[c];
    for (int c = 0; c < 3; ++c) tr[c] = bc[9 + c];

    // the dynamic programme: cell (i, j), 1 <= i <= n, 1 <= j <= m, lies on diagonal d = i + j at index i
    for (int i = tid; i < 3 * m; i += SC_THREADS) qs[i] = a.qs[i];
    double rp[AL_SLICE][3];
#pragma unroll
    for (int kk = 0; kk < AL_SLICE; ++kk) {
      const int i = tid + SC_THREADS * kk;
      rp[kk][0] = rp[kk][1] = rp[kk][2] = 0.0;
      if (i >= 1 && i <= n) {
        const double px = a.pm[3 * (i - 1)], py = a.pm[3 * (i - 1) + 1], pz = a.pm[3 * (i - 1) + 2];
        rp[kk][0] = ((R[0] * px + R[1] * py) + R[2] * pz) + tr[0];
        rp[kk][1] = ((R[3] * px + R[4] * py) + R[5] * pz) + tr[1];
        rp[kk][2] = ((R[6] * px + R[7] * py) + R[8] * pz) + tr[2];
      }
    }
    __syncthreads();
    const double d0sq = d0s * d0s;
    const int W = L + 1;
    for (int d = 0; d <= n + m; ++d) {
      double* Hc = Hb + (d % 3) * W;
      const double* H1 = Hb + ((d + 2) % 3) * W;             // diagonal d - 1
      const double* H2 = Hb + ((d + 1) % 3) * W;             // diagonal d - 2
      unsigned char* Dc = Db + (d % 3) * W;
      const unsigned char* D1 = Db + ((d + 2) % 3) * W;
      unsigned char* drow = dirp + (size_t)(d % (m + 1)) * (size_t)(n + 1);
#pragma unroll
      for (int kk = 0; kk < AL_SLICE; ++kk) {
        const int i = tid + SC_THREADS * kk, j = d - i;
        if (i <= n && j >= 0 && j <= m) {
          if (i == 0 || j == 0) {
            Hc[i] = 0.0;
            Dc[i] = 0;
          } else {
            const double ex = rp[kk][0] - (double)qs[3 * (j - 1)], ey = rp[kk][1] - (double)qs[3 * (j - 1) + 1],
                         ez = rp[kk][2] - (double)qs[3 * (j - 1) + 2];
            const double dd = (ex * ex + ey * ey) + ez * ez;
            const double s = 1.0 / (1.0 + dd / d0sq);
            const double ca = H2[i - 1] + s;
            const double cb = H1[i - 1] + (D1[i - 1] ? AL_GAP : 0.0);      // up: (i - 1, j)
            const double cc = H1[i] + (D1[i] ? AL_GAP : 0.0);              // left: (i, j - 1)
            const double bcm = cb > cc ? cb : cc;
            const unsigned char dr = ca >= bcm ? 0 : (cb >= cc ? 1 : 2);
            Hc[i] = dr == 0 ? ca : (dr == 1 ? cb : cc);
            Dc[i] = dr == 0 ? 1 : 0;
            drow[i] = dr;
          }
        }
      }
      __syncthreads();
    }
    // the traceback: serial, at most n + m steps; the pairs arrive last first and fill the new list from its end
    if (tid == 0) {
      int i = n, j = m, pos = L;
      for (int step = 0; step < n + m && i > 0 && j > 0; ++step) {
        const unsigned char dr = dirp[(size_t)((i + j) % (m + 1)) * (size_t)(n + 1) + i];
        if (dr == 0) {
          if (pos > 0) { --pos; ni[pos] = (unsigned short)(i - 1); nj[pos] = (unsigned short)(j - 1); }
          --i; --j;
        } else if (dr == 1) --i;
        else --j;
      }
      sh_off = pos;
      sh_K = L - pos;
      sh_diff = 0;
    }
    __syncthreads();
    const int nK = sh_K, noff = sh_off;
    if (nK == K)
      for (int t = tid; t < K; t += SC_THREADS)
        if (ni[noff + t] != ci[coff + t] || nj[noff + t] != cj[coff + t]) sh_diff = 1;
    __syncthreads();
    if ((nK == K && !sh_diff) || nK < 3) break;              // uniform: A' = A, or too few pairs to superpose
    unsigned short* sw = ci; ci = ni; ni = sw;
    sw = cj; cj = nj; nj = sw;
    K = nK;
    coff = noff;
    __syncthreads();                                         // (sh_diff is read above, written by thread 0 next round)
  }
  __syncthreads();

  // this survivor's record: best tm, its alignment
  int* rec = a.bali + (size_t)blockIdx.x * a.bali_stride;
  for (int t = tid; t < bK; t += SC_THREADS) { agent_store_i32(rec + 1 + 2 * t, (int)bi[t]); agent_store_i32(rec + 2 + 2 * t, (int)bj[t]); }
  __syncthreads();
  if (tid == 0) {
    agent_store_i32(rec, bK);
    agent_store_f64(a.btm + blockIdx.x, best_tm);
    sh_last = ticket_take_last(a.ticket + 1, (unsigned)nsurv) ? 1 : 0;
    if (sh_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!sh_last) return;

  // the last arriver: the winner (largest tm; ties: the lower seed number), the final superpositions, the outputs
  if (tid == 0) {
    double top = -__builtin_inf();
    int win = -1, win_seed = 0x7fffffff;
    for (int w = 0; w < nsurv; ++w) {
      const double tm = agent_load_f64(a.btm + w);
      const int sd = a.surv[1 + w];
      if (tm > top || (tm == top && sd < win_seed)) { top = tm; win = w; win_seed = sd; }
    }
    if (win >= 0 && agent_load_i32(a.bali + (size_t)win * a.bali_stride) < 3) win = -1;
    sh_win = win;
    ticket_reset(a.ticket + 1);
  }
  __syncthreads();
  const int win = sh_win;
  if (win < 0) return;                                       // nothing but NaN: the out slots stay NaN
  int* wrec = a.bali + (size_t)win * a.bali_stride;
  int wK = agent_load_i32(wrec);
  if (wK > L) wK = L;                                        // never
  for (int t = tid; t < wK; t += SC_THREADS) {
    ci[t] = (unsigned short)agent_load_i32(wrec + 1 + 2 * t);
    cj[t] = (unsigned short)agent_load_i32(wrec + 2 + 2 * t);
  }
  __syncthreads();
  align_finish(a, [ci](int t) { return (int)ci[t]; }, [cj](int t) { return (int)cj[t]; }, wK, a.surv[1 + win], 0.f, n, m, minov,
               d_cut, pm2, qn2, fl, wred, bc);
}

// ---------------------------------------------------------------------------------------
// align_screen: option "search_refine", one workgroup per entry - stage 1's best seed as the entry's answer
// ---------------------------------------------------------------------------------------
// The rank-0 survivor of align_thread (the best seed; ties went to the lower seed number) is a gapless alignment A*: the
// entry's header, ali and deviations by align_finish on A*, offset 21 = 1.  Nothing is written for an invalid entry or one
// without a survivor: its out slots stay NaN.  Dynamic LDS as align_thread's: 6 L floats, L flags.
__device__ __forceinline__ void align_screen_body(const AlignArgs& a) {
  extern __shared__ float sm[];
  __shared__ double wred[SC_WAVES][16];
  __shared__ double bc[12];
  const int L = a.L;
  if (a.hdr[AH_VALID] == 0.0) return;
  if (a.surv[0] < 1) return;
  const int n = (int)a.hdr[AH_N], m = (int)a.hdr[AH_M], minov = (int)a.hdr[AH_MINOV];
  const int seed = a.surv[1];
  int k, i0, ov;
  align_seed(seed, n, m, minov, k, i0, ov);
  if (ov < 3 || ov > L || i0 < 0 || i0 + ov > n || i0 + k < 0 || i0 + k + ov > m) return;      // never: a seed of align_thread
  align_finish(a, [i0](int t) { return i0 + t; }, [i0, k](int t) { return i0 + k + t; }, ov, seed, 1.f, n, m, minov, a.hdr[AH_DCUT],
               sm, sm + 3 * L, reinterpret_cast<unsigned char*>(sm + 6 * L), wred, bc);
}

// the single-partner launches of option "align_structure"
__global__ __launch_bounds__(SC_THREADS) void align_prep_kernel(AlignArgs a, const float* m_in) {
  a.mf = m_in[0];
  align_prep_body(a);
}
__global__ __launch_bounds__(SC_THREADS) void align_thread_kernel(AlignArgs a) { align_thread_body(a); }
__global__ __launch_bounds__(SC_THREADS) void align_refine_kernel(AlignArgs a) { align_refine_body(a); }

// ---------------------------------------------------------------------------------------
// options "search_structures" and "search_domains": the same three stages over a chunk of pairs (blockIdx.y)
// ---------------------------------------------------------------------------------------
// A search is a QUERY - what the library is searched with - run through one frame: the resolver search_pair, the four stage
// kernels, search_select and search_rank, each a template over the query, and the host's walk search_passes.  A query holds the
// SearchArgs as `sa` and answers, on the device: which pair - unit d (the chain, or one domain of it) against entry k - is
// virtual entry first + blockIdx.y (pair); which rows of the backbone form the pair's model (rows); where the pair's header
// (out) and its ali and deviation (ali) go; where a unit's screened tm_model, its select table and its ranking lie (screen,
// sel, rank); and the special cases of its select and rank launches (unit, unscreened, faulted).
struct SearchArgs {
  const float* coords;   // [L][5][3]
  float* conf;           // the d_conf buffer; the search block begins at B0 (search_base), which search_prep leaves in the table
  ConfLayout lay;
  int align;             // option "align_structure" of this prediction: its block lies in front of B0
  int L, max_L, max_m, K;
  unsigned char* ws;     // the scratch: table, tickets, slots (common.h)
  SearchSlot slot;
  const int* fault;      // the fault word of the prediction in flight
  int per, use_sel;      // this pass: the entries of a unit - all K, or the R chosen (option "search_refine"), which are taken
                         // through the unit's row of the select table
};
__device__ __forceinline__ int64_t* search_tab(const SearchArgs& sa) { return reinterpret_cast<int64_t*>(sa.ws); }

// unit d against entry k; the model is rows [off, off + n) of the query's row map
struct SearchPair { int d, k, off, n; };
// The r-th entry of a unit in this pass: through the unit's row `sel` of the select table, or r itself.
__device__ __forceinline__ bool search_pick(const SearchArgs& sa, const int* sel, int r, int& k) {
  k = sa.use_sel ? sel[r] : r;
  return k >= 0 && k < sa.K;                                 // always: search_select writes entries
}

// Option "search_structures": the whole chain against every entry.  One unit; the identity over the L rows; header, ali and
// deviation in the search block at b = conf + B0; the tables of option "search_refine" in the search scratch (common.h).
struct WholeQuery {
  SearchArgs sa;
  __device__ bool pair(int first, SearchPair& p) const {
    const int at = first + (int)blockIdx.y;
    if (at < 0 || at >= sa.per) return false;
    p.d = 0, p.off = 0, p.n = sa.L;
    return search_pick(sa, sel(0), at, p.k);
  }
  __device__ auto rows(const SearchPair&) const { return [](int i) { return i; }; }
  __device__ float* out(float* b, int, int k) const { return b + search_layout(sa.L, sa.K).hdr + (int64_t)ALIGN_HEADER * k; }
  __device__ float* ali(float* b, const SearchPair& p) const { return b + search_layout(sa.L, sa.K).res + 2 * (int64_t)sa.L * p.k; }
  __device__ float* screen(int) const { return reinterpret_cast<float*>(sa.ws + SEARCH_SCREEN_OFF); }
  __device__ int* sel(int) const { return reinterpret_cast<int*>(sa.ws + SEARCH_SEL_OFF); }
  __device__ float* rank(float* b, int) const { return b + search_layout(sa.L, sa.K).rank; }
  __device__ bool unit(int) const { return true; }           // (the grids of search_select and search_rank are 1)
  // with an invalid m_k somewhere nothing was screened (those entries return early)
  __device__ bool unscreened() const { return search_tab(sa)[0] != 1; }
  // a prediction that latched a fault gets NaN in every out slot instead of a ranking (the fault latch of api.hip does not know B0)
  __device__ bool faulted(float* b) const {
    if (*sa.fault == 0) return false;
    const SearchLayout lay = search_layout(sa.L, sa.K);
    const float nan = __builtin_nanf("");
    for (int64_t i = lay.rank + threadIdx.x; i < lay.in; i += SC_THREADS) b[i] = nan;
    return true;
  }
};

// Option "search_domains": every domain of the model against every entry (include/dmpfold_hip.h has the definition).
// Behind search_structures, on its stream, in its slots and with its table of the entries (validity, B0, trace offsets): the
// whole-model search has finished with the slots and the table stays as search_prep left it.  The virtual entry p = d per + r
// - domain d, the r-th of the `per` entries of a domain - takes slot p - first of its chunk, domain-major, so a chunk may
// straddle domains.  The model of pair (d, k) is the domain's rows gathered through the residue list; n_d goes into the slot
// header, and the shared bodies above read every row count from there.  ali and deviation of pair (d, k) go COMPACTLY into
// entry k's place of the block, at the domain's offset in the sorted list - the domains partition the chain, so the pairs of
// one entry never overlap, and a chunk's slot may be reused while they wait there - and domsearch_finish permutes each
// entry's 2L floats through LDS into residue order.
// The scratch of its own (dmp_ctx::domsearch_ws): per domain the screened tm_model of every entry and the entries selected
// (option "search_refine"), then 32 ints - [0] D, or 0 if nothing can be searched (the block stays NaN), [1] the one-domain
// shortcut is taken, [2 + d] the offset of domain d in the list, d <= 16 - then the residue list sorted by (label, index).
constexpr int64_t DS_SCREEN_OFF = 0, DS_SEL_OFF = 4 * (int64_t)DOMAINS_MAX * SEARCH_MAX, DS_INFO_OFF = 2 * DS_SEL_OFF,
                  DS_LIST_OFF = DS_INFO_OFF + 128;
ScratchNeed search_domains_need(int max_L) { return {DS_LIST_OFF + 4 * (int64_t)max_L, 0}; }

struct DomainQuery {
  SearchArgs sa;
  float* blk;            // the domain-search block
  const float* dom;      // the domain block of the same call
  unsigned char* dws;    // the scratch above
  int dmax;              // the domains the grids are sized for: max(1, min(16, L / min_size))
  int mode;              // the option's value: 2 never takes the shortcut
  __device__ int* info() const { return reinterpret_cast<int*>(dws + DS_INFO_OFF); }
  __device__ int* list() const { return reinterpret_cast<int*>(dws + DS_LIST_OFF); }
  // false before a slot is touched for an index that is no pair: d >= D, the shortcut, nothing to search
  __device__ bool pair(int first, SearchPair& p) const {
    const int64_t at = (int64_t)first + (int)blockIdx.y;
    if (first < 0 || sa.per < 1 || sa.per > sa.K || sa.K > SEARCH_MAX || at >= (int64_t)dmax * sa.per) return false;
    p.d = (int)(at / sa.per);
    if (!unit(p.d) || !search_pick(sa, sel(p.d), (int)(at % sa.per), p.k)) return false;
    p.off = info()[2 + p.d];
    p.n = info()[3 + p.d] - p.off;
    return p.off >= 0 && p.n >= 3 && p.off + p.n <= sa.L;    // always: domsearch_prep checked
  }
  __device__ auto rows(const SearchPair& p) const {
    const int* r = list() + p.off;
    return [r](int i) { return r[i]; };
  }
  __device__ float* out(float*, int d, int k) const {
    return blk + domsearch_layout(sa.L, sa.K).hdr + (int64_t)ALIGN_HEADER * ((int64_t)d * sa.K + k);
  }
  // compact: rows [off, off + n) of entry k's ali and, L further, deviation
  __device__ float* ali(float*, const SearchPair& p) const { return blk + domsearch_layout(sa.L, sa.K).res + 2 * (int64_t)sa.L * p.k + p.off; }
  __device__ float* screen(int d) const { return reinterpret_cast<float*>(dws + DS_SCREEN_OFF) + d * SEARCH_MAX; }
  __device__ int* sel(int d) const { return reinterpret_cast<int*>(dws + DS_SEL_OFF) + d * SEARCH_MAX; }
  __device__ float* rank(float*, int d) const { return blk + (int64_t)d * sa.K; }
  __device__ bool unit(int d) const { return d < DOMAINS_MAX && d < info()[0] && !info()[1]; }
  __device__ bool unscreened() const { return false; }       // (D = 0 then: no unit)
  __device__ bool faulted(float*) const { return false; }
};

// Virtual entry first + blockIdx.y of query q -> its pair p, in slot blockIdx.y.  False (uniform over the workgroup) for an
// index that is no pair.  With an invalid m_k somewhere the table says so: the entry then reads as m = 0 and nothing of its
// trace is touched.
template <class Q>
__device__ __forceinline__ bool search_pair(const Q& q, int first, AlignArgs& a, SearchPair& p) {
  const SearchArgs& sa = q.sa;
  const int y = (int)blockIdx.y;
  if (y >= SEARCH_CHUNK_MAX || !q.pair(first, p)) return false;
  const int64_t* tab = search_tab(sa);
  const bool ok = tab[0] == 1;
  float* b = sa.conf + tab[1];
  unsigned char* sl = sa.ws + SEARCH_HEAD_BYTES + (size_t)y * (size_t)sa.slot.total;
  a.coords = sa.coords;
  a.mf = ok ? b[p.k] : 0.f;
  a.out = q.out(b, p.d, p.k);
  a.ali = q.ali(b, p);
  a.trace = b + search_layout(sa.L, sa.K).in + (ok ? 3 * tab[2 + p.k] : 0);
  align_slot_args(a, sl, sa.slot, sa.L, sa.max_m, reinterpret_cast<unsigned*>(sa.ws + SEARCH_TAB_BYTES) + 2 * y);
  return true;
}

template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_align_prep_kernel(Q q, int first) {
  AlignArgs a;
  SearchPair p;
  if (search_pair(q, first, a, p)) align_prep_body(a, p.n, q.rows(p));
}
template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_align_thread_kernel(Q q, int first) {
  AlignArgs a;
  SearchPair p;
  if (search_pair(q, first, a, p)) align_thread_body(a);
}
template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_align_refine_kernel(Q q, int first) {
  AlignArgs a;
  SearchPair p;
  if (search_pair(q, first, a, p)) align_refine_body(a);
}
// the screen pass of option "search_refine": the pair's answer from its best seed, its tm_model (NaN: no result) in the unit's table
template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_align_screen_kernel(Q q, int first) {
  AlignArgs a;
  SearchPair p;
  if (!search_pair(q, first, a, p)) return;
  align_screen_body(a);
  if (threadIdx.x == 0) q.screen(p.d)[p.k] = a.out[2];       // what this thread wrote, or align_prep's NaN
}

// search_prep, one workgroup: B0 by the rule of common.h; every m_k an integer in [3, max_m]?; the rows in front of each
// entry (thread t sums entries 16 t .. 16 t + 15, thread 0 scans the 256 sums: integers, order-free); NaN into every out slot.
__global__ __launch_bounds__(SC_THREADS) void search_prep_kernel(SearchArgs sa) {
  constexpr int PER = SEARCH_MAX / SC_THREADS;
  __shared__ int bad[SC_THREADS];
  __shared__ int64_t part[SC_THREADS];
  __shared__ int sh_ok;
  const int tid = threadIdx.x, K = sa.K, L = sa.L;
  const int64_t B0 = search_base(sa.lay, L, sa.align, sa.align ? sa.conf[sa.lay.align.off] : 0.f, sa.max_L);
  float* b = sa.conf + B0;
  int64_t* tab = search_tab(sa);
  int mine = 0, mk[PER];
  int64_t sum = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int k = PER * tid + q;
    mk[q] = 0;
    if (k < K) {
      const float mf = b[k];
      const bool ok = mf >= 3.f && mf <= (float)sa.max_m && mf == floorf(mf);
      mine |= ok ? 0 : 1;
      mk[q] = ok ? (int)mf : 0;
      sum += mk[q];
    }
  }
  bad[tid] = mine;
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int any = 0;
    int64_t run = 0;
    for (int t = 0; t < SC_THREADS; ++t) {
      any |= bad[t];
      const int64_t v = part[t];
      part[t] = run;
      run += v;
    }
    sh_ok = any ? 0 : 1;
    tab[0] = sh_ok;
    tab[1] = B0;
  }
  __syncthreads();
  const bool ok = sh_ok != 0;
  int64_t run = part[tid];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int k = PER * tid + q;
    if (k < K) tab[2 + k] = ok ? run : 0;
    run += mk[q];
  }
  const SearchLayout lay = search_layout(L, K);
  const float nan = __builtin_nanf("");
  for (int64_t i = lay.rank + tid; i < lay.in; i += SC_THREADS) b[i] = nan;
}

// The ranking rule: entry j (value u) stands in front of entry k (value v) - a larger value, or an equal one of a lower index;
// the NaN entries last, in index order.
__device__ __forceinline__ bool search_before(float u, int j, float v, int k) {
  const bool unan = u != u, vnan = v != v;
  return vnan ? (!unan || j < k) : (!unan && (u > v || (u == v && j < k)));
}
// entry k's place among the K values of tm
__device__ __forceinline__ int search_place(const float* tm, int K, int k) {
  const float v = tm[k];
  int pos = 0;
  for (int j = 0; j < K; ++j) pos += search_before(tm[j], j, v, k) ? 1 : 0;
  return pos;
}

// The two rules as every thread of a workgroup applies them (tm: K floats of LDS, filled and behind a barrier): the R entries
// that rank first into sel, in rank order; every entry's index into rank, as a float.  Each a permutation: every place is
// written once.
__device__ __forceinline__ void search_select_into(const float* tm, int K, int R, int* sel) {
  for (int k = threadIdx.x; k < K; k += SC_THREADS) {
    const int pos = search_place(tm, K, k);
    if (pos < R) sel[pos] = k;
  }
}
__device__ __forceinline__ void search_rank_into(const float* tm, int K, float* rank) {
  for (int k = threadIdx.x; k < K; k += SC_THREADS) {
    const int pos = search_place(tm, K, k);
    if (pos < K) rank[pos] = (float)k;
  }
}

// search_select, one workgroup per unit (option "search_refine"): sel[r] = the entry with the r-th largest screened tm_model of
// unit blockIdx.x, r < R, by the rule of search_rank.  Where nothing was screened: the identity.
template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_select_kernel(Q q, int R) {
  __shared__ float tm[SEARCH_MAX];
  const int tid = threadIdx.x, K = q.sa.K < SEARCH_MAX ? q.sa.K : SEARCH_MAX, d = (int)blockIdx.x;
  if (!q.unit(d)) return;                                    // uniform
  R = R < K ? R : K;
  int* sel = q.sel(d);
  if (q.unscreened()) {                                      // uniform
    for (int r = tid; r < R; r += SC_THREADS) sel[r] = r;
    return;
  }
  const float* screen = q.screen(d);
  for (int k = tid; k < K; k += SC_THREADS) tm[k] = screen[k];
  __syncthreads();
  search_select_into(tm, K, R, sel);
}

// search_rank, one workgroup per unit: rank[r] = the entry with the r-th largest tm_model of unit blockIdx.x, by counting -
// entry k comes behind every entry with a larger value and every equal one of a lower index; the NaN entries last, in index
// order.
template <class Q>
__global__ __launch_bounds__(SC_THREADS) void search_rank_kernel(Q q) {
  __shared__ float tm[SEARCH_MAX];
  const int tid = threadIdx.x, K = q.sa.K < SEARCH_MAX ? q.sa.K : SEARCH_MAX, d = (int)blockIdx.x;
  if (!q.unit(d)) return;                                    // uniform
  float* b = q.sa.conf + search_tab(q.sa)[1];
  if (q.faulted(b)) return;                                  // uniform
  for (int k = tid; k < K; k += SC_THREADS) tm[k] = q.out(b, d, k)[2];
  __syncthreads();
  search_rank_into(tm, K, q.rank(b, d));
}

int align_kernel_attrs(dmp_ctx* c) {
  static_assert(AL_SLICE * SC_THREADS >= DMP_MAX_L + 1, "a thread's slice of a diagonal");
  static_assert(SEARCH_MAX % SC_THREADS == 0, "search_prep: a whole number of entries per thread");
  static bool done[64] = {};
  if (c->device >= 0 && c->device < 64 && done[c->device]) return DMP_OK;
  for (const void* refine : {(const void*)align_refine_kernel, (const void*)search_align_refine_kernel<WholeQuery>,
                             (const void*)search_align_refine_kernel<DomainQuery>})
    DMP_HIP(hipFuncSetAttribute(refine, hipFuncAttributeMaxDynamicSharedMemorySize, align_lds(DMP_MAX_L, DMP_MAX_L).total));
  if (c->device >= 0 && c->device < 64) done[c->device] = true;
  return DMP_OK;
}

// The scratch of "align_structure" (dmp_ctx::align_ws): the head - the two tickets - then the one slot, the largest a length takes.
constexpr int64_t ALIGN_HEAD_BYTES = 16;
ScratchNeed align_structure_need(int max_L) { return {ALIGN_HEAD_BYTES + search_slot(max_L, max_L).total, ALIGN_HEAD_BYTES}; }

// LDS of align_thread and align_screen in bytes: a seed's overlap has at most L rows, 6L floats + L flags, 50 KB at L = 2048
static size_t align_thread_lds(int L) { return sizeof(float) * 6 * L + round_up(L, 16); }

int align_structure(dmp_ctx* c, const float* d_coords, int L, float* d_block, hipStream_t s) {
  const AlignLayout lay = align_layout(L);
  AlignArgs a{};
  a.coords = d_coords;
  a.out = d_block + 1;
  a.ali = d_block + lay.ali;
  a.trace = d_block + lay.in;
  align_slot_args(a, c->align_ws.p + ALIGN_HEAD_BYTES, search_slot(L, c->max_L), L, c->max_L, reinterpret_cast<unsigned*>(c->align_ws.p));
  hipLaunchKernelGGL(align_prep_kernel, dim3(1), dim3(SC_THREADS), 0, s, a, (const float*)d_block);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(align_thread_kernel, dim3(L + c->max_L + 1), dim3(SC_THREADS), align_thread_lds(L), s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(align_refine_kernel, dim3(AL_T), dim3(SC_THREADS), align_lds(L, c->max_L).total, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

int search_wg_per_cu(int L, int max_m, int* out) {
  DMP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(out, (const void*)search_align_refine_kernel<WholeQuery>, SC_THREADS,
                                                       (size_t)align_lds(L, max_m).total));
  if (*out > 8) *out = 8;      // 256-thread workgroups: the hardware admits at most 8 per CU whatever the query answers
  return DMP_OK;
}

// One pass of query q over `total` virtual entries, in chunks of C consecutive ones (one slot each): align_prep, align_thread
// and the pass's last stage, `wgs` workgroups per pair with `lds` bytes.
template <class Q>
static int search_pass(const Q& q, int total, int C, void (*last)(Q, int), int wgs, size_t lds, hipStream_t s) {
  const int L = q.sa.L;
  for (int first = 0; first < total; first += C) {
    const int cn = std::min(C, total - first);
    hipLaunchKernelGGL(search_align_prep_kernel<Q>, dim3(1, cn), dim3(SC_THREADS), 0, s, q, first);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(search_align_thread_kernel<Q>, dim3(L + q.sa.max_m + 1, cn), dim3(SC_THREADS), align_thread_lds(L), s, q, first);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(last, dim3(wgs, cn), dim3(SC_THREADS), lds, s, q, first);
    DMP_LAUNCH_CHECK();
  }
  return DMP_OK;
}
// The passes of query q with `units` units (1, or the domains the grids are sized for): the three stages over every entry of
// every unit.  With option "search_refine" = R, 0 < R < K: stage 1 and align_screen over all units x K, search_select per
// unit, then the three stages over the units x R selected.  Everything is sized from (L, max_m, K, R) here; nothing comes
// back from the device.
template <class Q>
static int search_passes(Q& q, int units, int C, int refine, hipStream_t s) {
  SearchArgs& sa = q.sa;
  const int R = refine > 0 && refine < sa.K ? refine : 0;
  if (R) {
    sa.per = sa.K;
    if (int rc = search_pass(q, units * sa.K, C, search_align_screen_kernel<Q>, 1, align_thread_lds(sa.L), s)) return rc;
    hipLaunchKernelGGL(search_select_kernel<Q>, dim3(units), dim3(SC_THREADS), 0, s, q, R);
    DMP_LAUNCH_CHECK();
  }
  sa.per = R ? R : sa.K;                                     // slot y of a chunk holds virtual entry first + y of units x per
  sa.use_sel = R ? 1 : 0;
  return search_pass(q, units * sa.per, C, search_align_refine_kernel<Q>, AL_T, align_lds(sa.L, sa.max_m).total, s);
}

static SearchArgs search_args(dmp_ctx* c, const float* d_coords, int L, float* d_conf, const ConfLayout& lay) {
  SearchArgs sa{};
  sa.coords = d_coords;
  sa.conf = d_conf;
  sa.lay = lay;
  sa.align = c->run.align;
  sa.L = L;
  sa.max_L = c->max_L;
  sa.max_m = c->run.search_mm > 0 ? c->run.search_mm : c->max_L;
  sa.K = c->run.search;
  sa.ws = c->search_ws.p;
  sa.slot = search_slot(L, sa.max_m);
  sa.fault = c->seq_abort;
  return sa;
}

// search_prep, the passes of the whole query, search_rank
int search_structures(dmp_ctx* c, const float* d_coords, int L, float* d_conf, const ConfLayout& lay, hipStream_t s) {
  WholeQuery q{search_args(c, d_coords, L, d_conf, lay)};
  SearchArgs& sa = q.sa;
  const int C = search_chunk_entries(L, sa.max_m, c->run.search_chunk);
  DMP_ARG(sa.ws && SEARCH_HEAD_BYTES + (int64_t)C * sa.slot.total <= c->search_ws.bytes,
          "search_structures: the scratch does not hold a chunk of %d entries at L = %d, search_max_m = %d", C, L, sa.max_m);
  c->search_last_L = L;
  c->search_last_mm = sa.max_m;
  c->search_last_C = C;
  hipLaunchKernelGGL(search_prep_kernel, dim3(1), dim3(SC_THREADS), 0, s, sa);
  DMP_LAUNCH_CHECK();
  if (int rc = search_passes(q, 1, C, c->run.search_refine, s)) return rc;
  hipLaunchKernelGGL(search_rank_kernel<WholeQuery>, dim3(1), dim3(SC_THREADS), 0, s, q);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// option "search_domains": the domain query's own two kernels, in front of and behind the frame's
// ---------------------------------------------------------------------------------------
// domsearch_prep, one workgroup: NaN into the whole block; D and the labels from the domain block, validated (D an integer
// in [1, dmax], every label an integer in [0, D), every domain of at least 3 rows - always, after domains.hip; and every
// m_k valid, by search_prep's table - else D = 0 and nothing more runs); the counting sort: thread d counts label d, thread 0
// scans the 16 counts, thread d writes its residues in rising order.  Integers only.
__global__ __launch_bounds__(SC_THREADS) void domsearch_prep_kernel(DomainQuery da) {
  __shared__ unsigned char lab[DMP_MAX_L];
  __shared__ int cnt[DOMAINS_MAX], bad[SC_THREADS], sh_D;
  const int tid = threadIdx.x, L = da.sa.L < DMP_MAX_L ? da.sa.L : DMP_MAX_L;
  const DomSearchLayout lay = domsearch_layout(da.sa.L, da.sa.K);
  const float nan = __builtin_nanf("");
  for (int64_t i = tid; i < lay.total; i += SC_THREADS) da.blk[i] = nan;
  const float Df = da.dom[0];
  int D = Df >= 1.f && Df <= (float)da.dmax && Df <= (float)DOMAINS_MAX && Df == floorf(Df) ? (int)Df : 0;      // a NaN fails the comparisons
  if (search_tab(da.sa)[0] != 1) D = 0;
  int mine = 0;
  for (int i = tid; i < L; i += SC_THREADS) {
    const float lf = da.dom[DOMAINS_HEADER + i];
    const bool ok = lf >= 0.f && lf < (float)D && lf == floorf(lf);
    mine |= ok ? 0 : 1;
    lab[i] = ok ? (unsigned char)lf : (unsigned char)0xff;
  }
  bad[tid] = mine;
  __syncthreads();
  if (tid < DOMAINS_MAX) {
    int n = 0;
    for (int i = 0; i < L; ++i) n += lab[i] == tid ? 1 : 0;
    cnt[tid] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int* info = da.info();
    int any = 0, run = 0;
    for (int k = 0; k < SC_THREADS; ++k) any |= bad[k];
    for (int d = 0; d < DOMAINS_MAX; ++d) {
      const int n = cnt[d];
      any |= d < D && n < 3 ? 1 : 0;
      info[2 + d] = run;
      cnt[d] = run;
      run += n;
    }
    info[2 + DOMAINS_MAX] = run;
    if (any || run != L) D = 0;
    info[0] = D;
    info[1] = D == 1 && da.mode != 2 ? 1 : 0;
    sh_D = D;
  }
  __syncthreads();
  if (sh_D == 0) return;                                     // uniform
  if (tid < DOMAINS_MAX) {
    int* list = da.list();
    int at = cnt[tid];
    for (int i = 0; i < L; ++i)
      if (lab[i] == tid) list[at++] = i;                     // at most cnt's n of them: the same labels were counted
  }
}

// domsearch_finish, one workgroup per entry.  The shortcut (D = 1, the domain is the chain): the whole search's rank, header,
// ali and deviation of this entry into row 0.  Else: the entry's 2L compact floats into residue order, through LDS - position
// j of the sorted list is residue list[j], and the list is a permutation of 0 .. L - 1.
__global__ __launch_bounds__(SC_THREADS) void domsearch_finish_kernel(DomainQuery da) {
  __shared__ float buf[2 * DMP_MAX_L];
  const int tid = threadIdx.x, K = da.sa.K, k = (int)blockIdx.x, L = da.sa.L < DMP_MAX_L ? da.sa.L : DMP_MAX_L;
  const int* info = da.info();
  if (k >= K || info[0] == 0) return;                        // uniform
  const DomSearchLayout dl = domsearch_layout(da.sa.L, K);
  float* res = da.blk + dl.res + 2 * (int64_t)L * k;
  if (info[1]) {                                             // uniform
    const float* b = da.sa.conf + search_tab(da.sa)[1];
    const SearchLayout lay = search_layout(da.sa.L, K);
    for (int i = tid; i < 2 * L; i += SC_THREADS) res[i] = b[lay.res + 2 * (int64_t)L * k + i];
    for (int i = tid; i < ALIGN_HEADER; i += SC_THREADS)
      da.blk[dl.hdr + (int64_t)ALIGN_HEADER * k + i] = b[lay.hdr + (int64_t)ALIGN_HEADER * k + i];
    if (tid == 0) da.blk[k] = b[lay.rank + k];
    return;
  }
  for (int i = tid; i < 2 * L; i += SC_THREADS) buf[i] = res[i];
  __syncthreads();
  const int* list = da.list();
  for (int j = tid; j < L; j += SC_THREADS) {
    int i = list[j];
    i = i < 0 ? 0 : (i >= L ? L - 1 : i);                    // never
    res[i] = buf[j];
    res[L + i] = buf[L + j];
  }
}

// domsearch_prep, the passes of the domain query over its Dmax units (select and rank one workgroup per domain),
// domsearch_finish.  Dmax = max(1, min(16, L / min_size)) bounds D: a cut is admissible only if both parts hold min_size
// residues (domains.hip, domains_cuts_kernel: `if (size < a.min_size || n - size < a.min_size ...) continue;`), so
// D min_size <= L.  Nothing comes back from the device.
int search_domains(dmp_ctx* c, const float* d_coords, int L, float* d_conf, const ConfLayout& lay, hipStream_t s) {
  DomainQuery q{search_args(c, d_coords, L, d_conf, lay)};
  SearchArgs& sa = q.sa;
  q.blk = d_conf + lay.domsearch.off;
  q.dom = d_conf + lay.domains.off;
  q.dws = c->domsearch_ws.p;
  q.dmax = std::max(1, std::min(DOMAINS_MAX, L / c->run.dom_min_size));
  q.mode = c->run.search_domains;
  const int C = search_chunk_entries(L, sa.max_m, c->run.search_chunk);
  DMP_ARG(sa.ws && SEARCH_HEAD_BYTES + (int64_t)C * sa.slot.total <= c->search_ws.bytes && q.dws &&
              c->domsearch_ws.bytes >= search_domains_need(L).bytes,
          "search_domains: the scratch does not hold a chunk of %d entries at L = %d, search_max_m = %d", C, L, sa.max_m);
  hipLaunchKernelGGL(domsearch_prep_kernel, dim3(1), dim3(SC_THREADS), 0, s, q);
  DMP_LAUNCH_CHECK();
  if (int rc = search_passes(q, q.dmax, C, c->run.search_refine, s)) return rc;
  hipLaunchKernelGGL(search_rank_kernel<DomainQuery>, dim3(q.dmax), dim3(SC_THREADS), 0, s, q);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(domsearch_finish_kernel, dim3(sa.K), dim3(SC_THREADS), 0, s, q);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
