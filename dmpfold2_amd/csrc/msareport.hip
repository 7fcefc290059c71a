// option "msa_report": how deep the alignment of a prediction was, how conserved each column is, and what the raw DCA contact
// map says (include/dmpfold_hip.h has the layout of the report block and the definition of every number).  It runs in
// dmp_predict_end, behind "flex", from what the front end left on the device: the packed clamped alignment (c->msa_words), the
// weights (c->w) and the contact map the stem was given (c->contacts).  A "gap" is a clamped code of 20.
//   msa_count_kernel<true>   (msa.hip) the N^2 L byte compares of the weights once more, with the report's epilogue: per row the
//                            neighbour counts at 0.62, 0.8 and 0.9 and the largest count over the other rows (integer atomics)
//   msareport_row_kernel     one wave per row: identity to the query, coverage, nearest neighbour into three histograms, the gap
//                            cells and the copied rows - LDS first, then one integer atomic per bin and workgroup
//   msareport_col_kernel     one workgroup per column: raw counts (integers) and weighted counts (float64, every thread its own
//                            LDS column, then a fixed tree) of the 21 codes, then the column's six figures
//   msareport_dca_kernel     one workgroup per row of the contact map: the strongest coupling at |j - l| >= 6 and its partner
//   msareport_pairs_kernel,  with a native: the candidates and native contacts of "score_map"'s classes (integer counts), n, ln,
//   msareport_classes_kernel then mapscore.hip's radix select with the coupling key for h and t
//   msareport_finish_kernel  one workgroup: the three Neff sums (block_tree_sum_f64) and the header
// No float atomics, every float64 sum in a fixed order: the same bits on every run.  The counters are cleared on the stream in
// front of every report.
#include "common.h"

#pragma clang fp contract(off)

namespace dmp {

constexpr int MR_THREADS = 256;
constexpr int MR_WAVES = MR_THREADS / 64;
constexpr int MR_CODES = 21;
// the counters (ints): the three histograms, then
constexpr int MR_IDQ = 0, MR_COV = 20, MR_NN = 40, MR_GAPS = 60, MR_COPIES = 61, MR_CLASS = 64, MR_COUNTERS = 80;
constexpr int MR_MAX_WG = 64;

struct ReportArgs {
  const uint32_t* words;   // [N][Lw] c->msa_words
  const float* w;          // [N] c->w
  const float* contacts;   // [L][L] c->contacts
  const float* nat;        // the score block (its trace, lnorm) or null
  float* out;              // the report block
  int* cnt;                // [MR_COUNTERS]
  int* nbr;                // [4][N]
  int N, L, Lw;
};

__global__ __launch_bounds__(MR_THREADS) void msareport_row_kernel(ReportArgs a) {
  __shared__ unsigned h[64];
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.x * MR_WAVES + (tid >> 6);
  if (tid < 64) h[tid] = 0u;
  __syncthreads();
  if (n < a.N) {                                   // uniform in the wave
    int num = 0, den = 0, cov = 0;
    for (int wd = lane; wd < a.Lw; wd += 64) {
      const uint32_t x = a.words[(int64_t)n * a.Lw + wd], q = a.words[wd];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (wd * 4 + b >= a.L) break;              // (the tail bytes of the last word)
        const unsigned cx = (x >> (8 * b)) & 255u, cq = (q >> (8 * b)) & 255u;
        cov += cx < 20u ? 1 : 0;
        den += cq < 20u ? 1 : 0;
        num += (cx == cq && cq < 20u) ? 1 : 0;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      num += __shfl_xor(num, off, 64);
      den += __shfl_xor(den, off, 64);
      cov += __shfl_xor(cov, off, 64);
    }
    if (lane == 0) {
      const int bq = den > 0 ? min(19, 20 * num / den) : 0, bc = min(19, 20 * cov / a.L);
      atomicAdd(&h[MR_IDQ + bq], 1u);
      atomicAdd(&h[MR_COV + bc], 1u);
      if (a.L - cov) atomicAdd(&h[MR_GAPS], (unsigned)(a.L - cov));
      if (a.N > 1) {
        const int top = a.nbr[3 * (int64_t)a.N + n];
        atomicAdd(&h[MR_NN + min(19, 20 * top / a.L)], 1u);
        if (top == a.L) atomicAdd(&h[MR_COPIES], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < 64 && h[tid]) atomicAdd(&a.cnt[tid], (int)h[tid]);
}

__global__ __launch_bounds__(MR_THREADS) void msareport_col_kernel(ReportArgs a) {
  __shared__ double acc[MR_CODES][MR_THREADS];
  __shared__ int raw[MR_CODES];
  const int tid = threadIdx.x, l = blockIdx.x, L = a.L;
#pragma unroll
  for (int k = 0; k < MR_CODES; ++k) acc[k][tid] = 0.0;
  if (tid < MR_CODES) raw[tid] = 0;
  __syncthreads();
  const int wd = l >> 2, sh = 8 * (l & 3);
  for (int n = tid; n < a.N; n += MR_THREADS) {
    const unsigned code = (a.words[(int64_t)n * a.Lw + wd] >> sh) & 255u;     // <= 20: msa_pack_kernel clamped it
    acc[code][tid] += (double)a.w[n];
    atomicAdd(&raw[code], 1);
  }
  __syncthreads();
  for (int s = MR_THREADS / 2; s > 0; s >>= 1) {
    for (int idx = tid; idx < MR_CODES * s; idx += MR_THREADS) {
      const int k = idx / s, t = idx - k * s;
      acc[k][t] += acc[k][t + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const float nan = __builtin_nanf("");
  float* col = a.out + MSAREPORT_HEADER + l;
  double tot = 0.0;
  for (int k = 0; k < 20; ++k) tot += acc[k][0];
  double ent = 0.0;
  int best = -1, most = 0;
  for (int k = 0; k < 20; ++k) {
    if (raw[k] > most) { most = raw[k]; best = k; }
    const double p = tot > 0.0 ? acc[k][0] / tot : 0.0;
    if (p > 0.0) ent -= p * log(p);
  }
  const unsigned cq = (a.words[wd] >> sh) & 255u;
  col[0] = (float)raw[20];
  col[L] = (float)tot;
  col[2 * (int64_t)L] = tot > 0.0 ? (float)ent : 0.f;
  col[3 * (int64_t)L] = best < 0 ? nan : (float)best;
  col[4 * (int64_t)L] = best < 0 ? nan : (float)(acc[best][0] / tot);
  col[5 * (int64_t)L] = cq < 20u ? (float)(acc[cq][0] / tot) : nan;
}

__global__ __launch_bounds__(MR_THREADS) void msareport_dca_kernel(ReportArgs a) {
  __shared__ unsigned long long red[MR_WAVES];
  const int tid = threadIdx.x, l = blockIdx.x, L = a.L;
  float* col = a.out + MSAREPORT_HEADER + 6 * (int64_t)L + l;
  const float nan = __builtin_nanf("");
  if (a.N <= 1) {                                  // uniform: no covariance features, c->contacts holds another target's
    if (tid == 0) { col[0] = nan; col[L] = nan; }
    return;
  }
  const float* row = a.contacts + (int64_t)l * L;
  unsigned long long best = ~0ull;
  for (int j = tid; j < L; j += MR_THREADS) {
    if (j - l < 6 && l - j < 6) continue;
    const unsigned long long key = ((unsigned long long)coupling_rank_bits(row[j]) << 32) | (unsigned)j;
    best = key < best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < MR_WAVES; ++k) best = red[k] < best ? red[k] : best;
  const int j = (int)(unsigned)best;
  col[0] = best == ~0ull ? nan : row[j];
  col[L] = best == ~0ull ? nan : (float)j;
}

// the native contact test of "score_map": float32, every operation rounded
__device__ inline bool mr_native_contact(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return (dx * dx + dy * dy) + dz * dz < 64.0f;
}

__global__ __launch_bounds__(MR_THREADS) void msareport_pairs_kernel(ReportArgs a) {
  extern __shared__ float q[];                     // 3L native coordinates
  __shared__ int icnt[6];
  const int tid = threadIdx.x, L = a.L;
  for (int i = tid; i < 3 * L; i += MR_THREADS) q[i] = a.nat[i];
  if (tid < 6) icnt[tid] = 0;
  __syncthreads();
  int cls[6] = {0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x; i < L; i += gridDim.x) {
    if (!(q[3 * i] == q[3 * i])) continue;         // uniform: the row is absent
    for (int j = i + 6 + tid; j < L; j += MR_THREADS) {
      if (!(q[3 * j] == q[3 * j])) continue;
      const int s = j - i, c = s <= 11 ? 0 : (s <= 23 ? 1 : 2);
      const int nc = mr_native_contact(q + 3 * i, q + 3 * j) ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k == c) { cls[2 * k] += 1; cls[2 * k + 1] += nc; }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int v = cls[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0 && v) atomicAdd(&icnt[k], v);
  }
  __syncthreads();
  if (tid < 6 && icnt[tid]) atomicAdd(&a.cnt[MR_CLASS + tid], icnt[tid]);
}

// one workgroup: N_c, the native contacts and the zeros of every class, n and ln - what the select reads and leaves alone
__global__ __launch_bounds__(MR_THREADS) void msareport_classes_kernel(ReportArgs a) {
  __shared__ int red[MR_WAVES];
  const int tid = threadIdx.x, L = a.L;
  int n = 0;
  for (int i = tid; i < L; i += MR_THREADS) n += a.nat[3 * i] == a.nat[3 * i] ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = n;
  __syncthreads();
  if (tid != 0) return;
  n = 0;
  for (int k = 0; k < MR_WAVES; ++k) n += red[k];
  const float lnorm = a.nat[3 * L];
  for (int c = 0; c < 4; ++c) {
    float* o = a.out + MSAREPORT_CLASSES + 12 * c;
    const int* u = a.cnt + MR_CLASS + 2 * (c < 3 ? c : 1);
    const int* v = a.cnt + MR_CLASS + 2 * 2;
    o[0] = (float)(u[0] + (c == 3 ? v[0] : 0));
    o[1] = (float)(u[1] + (c == 3 ? v[1] : 0));
    for (int k = 2; k < 12; ++k) o[k] = 0.f;
  }
  a.out[MSAREPORT_N] = (float)n;
  a.out[MSAREPORT_N + 1] = lnorm > 0.f ? lnorm : (float)n;
}

__global__ __launch_bounds__(MR_THREADS) void msareport_finish_kernel(ReportArgs a) {
  __shared__ double red[MR_THREADS];
  const int tid = threadIdx.x, N = a.N;
  double neff[3];
  for (int t = 0; t < 3; ++t) {
    double v = 0.0;
    for (int n = tid; n < N; n += MR_THREADS) v += 1.0 / (double)a.nbr[(int64_t)t * N + n];
    neff[t] = block_tree_sum_f64<MR_THREADS>(v, red);
    __syncthreads();
  }
  const bool ranked = a.nat != nullptr && N > 1;
  float* out = a.out;
  for (int k = tid; k < MSAREPORT_HEADER; k += MR_THREADS) {
    float v = 0.f;
    if (k == 0) v = (float)N;
    else if (k == 1) v = (float)a.L;
    else if (k < 5) v = (float)neff[k - 2];
    else if (k == 5) v = (float)a.cnt[MR_GAPS];
    else if (k == 6) v = (float)a.cnt[MR_COPIES];
    else if (k == 7) {                             // the query's gap columns
      int g = 0;
      for (int l = 0; l < a.L; ++l) g += ((a.words[l >> 2] >> (8 * (l & 3))) & 255u) == 20u ? 1 : 0;
      v = (float)g;
    } else if (k >= 16 && k < 16 + 3 * MSAREPORT_HIST) v = (float)a.cnt[k - 16];
    else if (k >= MSAREPORT_CLASSES && k < MSAREPORT_N + 2) {
      if (ranked) continue;                        // msareport_classes_kernel's and the select's
    } else if (k == 126) v = N > 1 ? 1.f : 0.f;
    else if (k == 127) v = a.nat != nullptr ? 1.f : 0.f;
    out[k] = v;
  }
}

// The scratch (dmp_ctx::report_ws), ints from its start: the counters, then the rows' four neighbour counts.  All of it is
// cleared on the stream in front of every report: nothing survives a prediction.
ScratchNeed msa_report_need(int max_N) { return {4 * (MR_COUNTERS + 4 * (int64_t)max_N), 0}; }

int msa_report(dmp_ctx* c, int N, int L, const float* d_native, float* d_block, hipStream_t s) {
  ReportArgs a{};
  a.words = c->msa_words;
  a.w = c->w;
  a.contacts = c->contacts;
  a.nat = d_native;
  a.out = d_block;
  a.cnt = reinterpret_cast<int*>(c->report_ws.p);
  a.nbr = a.cnt + MR_COUNTERS;
  a.N = N;
  a.L = L;
  a.Lw = cdiv(L, 4);
  const dim3 T(MR_THREADS);
  DMP_HIP(hipMemsetAsync(a.cnt, 0, sizeof(int) * (MR_COUNTERS + 4 * (size_t)N), s));
  if (int rc = msa_report_pairs(c, N, L, a.nbr, s)) return rc;
  hipLaunchKernelGGL(msareport_row_kernel, dim3(cdiv(N, MR_WAVES)), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(msareport_col_kernel, dim3(L), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(msareport_dca_kernel, dim3(L), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  if (d_native && N > 1) {
    const int g = std::min(std::max(L / 16, 1), MR_MAX_WG);
    hipLaunchKernelGGL(msareport_pairs_kernel, dim3(g), T, sizeof(float) * 3 * L, s, a);
    DMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(msareport_classes_kernel, dim3(1), T, 0, s, a);
    DMP_LAUNCH_CHECK();
    if (int rc = mapscore_select_couplings(c->contacts, d_native, d_block + MSAREPORT_CLASSES - 2, L, s)) return rc;
  }
  hipLaunchKernelGGL(msareport_finish_kernel, dim3(1), T, 0, s, a);
  DMP_LAUNCH_CHECK();
  if (c->run.msa_report == 2) {
    float* map = d_block + MSAREPORT_HEADER + MSAREPORT_COLS * (int64_t)L;
    const size_t bytes = sizeof(float) * (size_t)L * L;
    if (N > 1) DMP_HIP(hipMemcpyAsync(map, c->contacts, bytes, hipMemcpyDeviceToDevice, s));
    else DMP_HIP(hipMemsetAsync(map, 0, bytes, s));
  }
  return DMP_OK;
}

}  // namespace dmp
