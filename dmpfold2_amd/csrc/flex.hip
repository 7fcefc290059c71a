// option "flex": the Gaussian network model of the final C-alpha trace, and of the native's where option "score_native" holds a
// whole native trace (include/dmpfold_hip.h has the layout of the flex block and the only definition of every figure in it).
// Per leg, stream-ordered, nothing read back by the host:
//   (memset)              the degrees zero
//   flex_kirchhoff_kernel the contacts of a tile of 16 rows x 256 columns - the rows' coordinates through LDS, the float64
//                         test of the header on float32 coordinates - as the off-diagonal of the float32 matrix
//                         M = sigma I - Gamma (1 in contact, else 0), and the rows' degrees by one integer atomic per row and tile
//   flex_sigma_kernel     one workgroup: the largest degree and the contact total from the degrees, sigma = 2 max degree, then
//                         the diagonal sigma - degree_i.  Every entry of M is an integer below 4096, exact in float32
//   eigh_top8_modes       the solver of the MDS step (mds.hip) on M with the other epilogue of its back-transformation: the unit
//                         vectors under the sign rule, as float32 straight into the block and as float64 into the solver's scratch
//   flex_finish_kernel    lambda_k = sigma - mu_(7-k) in double, the zero rule, components, used, and
//                         msf_i = sum over the non-zero modes, ascending, of z_ki z_ki / lambda_k
//                         from the float64 z of the back-transformation KEPT IN SCRATCH - not from the float32 modes of the
//                         block - accumulated in float64 in that order and rounded once; the leg's header and degrees
// A native leg that is absent (no score block, or a NaN coordinate: whole_xyz of the native entity) gets zeros / NaN from
// flex_finish_kernel alone; with a score block whose trace is not whole the solver still runs on what the finite rows give,
// since no launch depends on what the device finds, and its modes are overwritten.
// Integer atomics only: the same bits on every run.  Contraction is off (score_common.h), so d2 is the header's expression.
#include "score_common.h"

namespace dmp {

constexpr int FLEX_THREADS = 256, FLEX_ROWS = 16;
constexpr double FLEX_ZERO = 1e-7;        // a mode is a zero mode iff lambda <= this (the header derives the number)
static_assert(FLEX_HEADER == 16 && FLEX_LEG == 16 && FLEX_MODES == 8, "the block of include/dmpfold_hip.h");

// The scratch of a context of capacity `cap` (bytes from its start, every part 16-aligned): a head of 16 bytes = contacts,
// sigma | the degrees [cap] | M [cap][cap] float32.  Nothing in it has to be zero between launches.
struct FlexScratch { int64_t deg, m, total; };
constexpr int64_t FLEX_HEAD_BYTES = 16;
inline FlexScratch flex_scratch(int cap) {
  auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  FlexScratch s;
  s.deg = FLEX_HEAD_BYTES;
  s.m = s.deg + up(4 * (int64_t)cap);
  s.total = s.m + up(4 * (int64_t)cap * cap);
  return s;
}
ScratchNeed flex_need(int max_L) { return {flex_scratch(max_L).total, FLEX_HEAD_BYTES}; }

struct FlexArgs {
  const float* xyz;           // the leg's first C-alpha ...
  int pitch;                  // ... and the floats from one residue's to the next's
  int L, e, cut_mA;
  double cut2;                // c c, c = cut_mA / 1000.0
  const int* whole;           // leg 1: the native entity's whole_xyz, or null where there is no score block
  int* head;                  // [0] contacts, [1] sigma
  int* deg;                   // [L]
  float* M;                   // [L][L]
  const double* mu;           // [8] the solver's eigenvalues of M, ascending
  const double* zq;           // [L][8] its unit vectors in float64, column c of eigenvalue mu[c]
  float* out;                 // the flex block
};

__global__ __launch_bounds__(FLEX_THREADS) void flex_kirchhoff_kernel(FlexArgs a) {
  __shared__ float row[FLEX_ROWS][3];
  __shared__ int cnt[FLEX_ROWS];
  const int tid = threadIdx.x, L = a.L, j = blockIdx.x * FLEX_THREADS + tid, i0 = blockIdx.y * FLEX_ROWS;
  if (tid < FLEX_ROWS * 3) {
    const int r = tid / 3, i = i0 + r;
    row[r][tid % 3] = i < L ? a.xyz[(int64_t)a.pitch * i + tid % 3] : 0.f;
  }
  if (tid < FLEX_ROWS) cnt[tid] = 0;
  double qx = 0.0, qy = 0.0, qz = 0.0;
  if (j < L) {
    const float* q = a.xyz + (int64_t)a.pitch * j;
    qx = (double)q[0]; qy = (double)q[1]; qz = (double)q[2];
  }
  __syncthreads();
  for (int r = 0; r < FLEX_ROWS; ++r) {
    const int i = i0 + r;
    if (i >= L) break;                                    // uniform
    const double dx = (double)row[r][0] - qx, dy = (double)row[r][1] - qy, dz = (double)row[r][2] - qz;
    const bool c = j < L && j != i && (dx * dx + dy * dy) + dz * dz < a.cut2;
    if (j < L) a.M[(int64_t)i * L + j] = c ? 1.f : 0.f;   // the diagonal: flex_sigma_kernel, behind this launch
    const unsigned long long m = __ballot(c);
    if ((tid & 63) == 0 && m) atomicAdd(&cnt[r], __popcll(m));
  }
  __syncthreads();
  if (tid < FLEX_ROWS && i0 + tid < L && cnt[tid]) atomicAdd(&a.deg[i0 + tid], cnt[tid]);
}

__global__ __launch_bounds__(FLEX_THREADS) void flex_sigma_kernel(FlexArgs a) {
  __shared__ int wmax[FLEX_THREADS / 64], wsum[FLEX_THREADS / 64];
  const int tid = threadIdx.x, L = a.L;
  int mx = 0, sum = 0;
  for (int i = tid; i < L; i += FLEX_THREADS) {
    const int d = a.deg[i];
    mx = d > mx ? d : mx;
    sum += d;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(mx, off, 64);
    mx = o > mx ? o : mx;
    sum += __shfl_xor(sum, off, 64);
  }
  if ((tid & 63) == 0) { wmax[tid >> 6] = mx; wsum[tid >> 6] = sum; }
  __syncthreads();
  mx = 0; sum = 0;
#pragma unroll
  for (int w = 0; w < FLEX_THREADS / 64; ++w) {
    mx = wmax[w] > mx ? wmax[w] : mx;
    sum += wsum[w];
  }
  const int sigma = 2 * mx;
  if (tid == 0) { a.head[0] = sum / 2; a.head[1] = sigma; }
  for (int i = tid; i < L; i += FLEX_THREADS) a.M[(int64_t)i * L + i] = (float)(sigma - a.deg[i]);
}

__global__ __launch_bounds__(FLEX_THREADS) void flex_finish_kernel(FlexArgs a) {
  const int tid = threadIdx.x, L = a.L, e = a.e, i = blockIdx.x * FLEX_THREADS + tid;
  const FlexLayout lay = flex_layout(L);
  const bool active = e == 0 || (a.whole && *a.whole != 0);
  float* hdr = a.out + lay.leg + FLEX_LEG * e;
  float* deg = a.out + lay.res + (int64_t)lay.per_leg * e;
  float* msf = deg + L;
  float* modes = msf + L;
  if (e == 0 && i < FLEX_HEADER) a.out[i] = i == 0 ? (float)L : (i == 1 ? (float)a.cut_mA : 0.f);
  if (e == 1 && i == 0) a.out[2] = active ? 1.f : 0.f;     // behind leg 0's launch
  if (!active) {                                           // uniform: no native leg
    const float nan = __builtin_nanf("");
    if (i < FLEX_LEG) hdr[i] = 0.f;
    if (i < L) {
      deg[i] = nan;
      msf[i] = nan;
      for (int k = 0; k < FLEX_MODES; ++k) modes[(int64_t)k * L + i] = nan;
    }
    return;
  }
  const int sigma = a.head[1];
  double lam[FLEX_MODES];
  int zero = 0;
#pragma unroll
  for (int k = 0; k < FLEX_MODES; ++k) {
    lam[k] = (double)sigma - a.mu[FLEX_MODES - 1 - k];
    zero += lam[k] <= FLEX_ZERO ? 1 : 0;
  }
  if (i < L) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < FLEX_MODES; ++k) {
      const double z = a.zq[(int64_t)i * FLEX_MODES + (FLEX_MODES - 1 - k)];
      if (lam[k] > FLEX_ZERO) acc += (z * z) / lam[k];
    }
    msf[i] = (float)acc;
    deg[i] = (float)a.deg[i];
  }
  if (i < FLEX_LEG) {
    float v = 0.f;
    if (i == 0) v = (float)a.head[0];
    else if (i == 1) v = (float)sigma;
    else if (i == 2) v = (float)zero;
    else if (i == 3) v = (float)(FLEX_MODES - zero);
    else if (i >= 8) v = (float)lam[i - 8];
    hdr[i] = v;
  }
}

int flex(dmp_ctx* c, const float* d_coords, int L, const float* d_native, float* d_block, hipStream_t s) {
  const FlexScratch sc = flex_scratch(c->max_L);
  const FlexLayout lay = flex_layout(L);
  unsigned char* ws = c->flex_ws.p;
  const double cut = c->run.flex_cut / 1000.0;
  FlexArgs a{};
  a.L = L;
  a.cut_mA = c->run.flex_cut;
  a.cut2 = cut * cut;
  a.head = (int*)ws;
  a.deg = (int*)(ws + sc.deg);
  a.M = (float*)(ws + sc.m);
  a.out = d_block;
  const dim3 T(FLEX_THREADS);
  const unsigned fin = (unsigned)cdiv(std::max(L, FLEX_LEG), FLEX_THREADS);
  for (int e = 0; e < 2; ++e) {
    a.e = e;
    a.xyz = e ? d_native : d_coords + 3;  // the score block's native trace [L][3]; the C-alpha of [L][5][3] N, CA, C, O, CB
    a.pitch = e ? 3 : 15;
    a.whole = e && d_native ? native_entity(c).whole_xyz : nullptr;
    if (e == 0 || d_native) {
      DMP_HIP(hipMemsetAsync(a.deg, 0, sizeof(int) * (size_t)L, s));
      hipLaunchKernelGGL(flex_kirchhoff_kernel, dim3(cdiv(L, FLEX_THREADS), cdiv(L, FLEX_ROWS)), T, 0, s, a);
      DMP_LAUNCH_CHECK();
      hipLaunchKernelGGL(flex_sigma_kernel, dim3(1), T, 0, s, a);
      DMP_LAUNCH_CHECK();
      float* modes = d_block + lay.res + (int64_t)lay.per_leg * e + 2 * (int64_t)L;
      if (int rc = eigh_top8_modes(c, a.M, L, modes, &a.mu, &a.zq, s)) return rc;
    }
    hipLaunchKernelGGL(flex_finish_kernel, dim3(fin), T, 0, s, a);
    DMP_LAUNCH_CHECK();
  }
  return DMP_OK;
}

}  // namespace dmp
