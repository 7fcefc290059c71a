// What score.hip (option "score_native") and align.hip (option "align_structure") share: the rotation of a superposition,
// the deviation of a pair under it, the workgroup's fixed-order float64 sum, and the shrinking-set loop of one seed of the
// superposition search over packed pair arrays.  Float64 from the float32 coordinates; contraction is off so that the bits
// do not depend on the compiler's choices (and are the same in both translation units).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace dmp {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_ITERS = 20;

// d0 of a normalising length (the TM-score's distance scale)
__host__ __device__ inline double score_d0(double lnorm) { return lnorm > 15.0 ? fmax(1.24 * cbrt(lnorm - 15.0) - 1.8, 0.5) : 0.5; }

// Rotation R (row-major) maximising sum_k q_k . R p_k from the covariance M[a][b] = sum_k p_a q_b of the centred sets:
// the eigenvector of the largest eigenvalue of Horn's symmetric 4 x 4 matrix (J. Opt. Soc. Am. A 4, 629, 1987), by cyclic
// Jacobi rotations in float64.  Unlike the Newton iteration on the characteristic polynomial (QCP) it loses nothing when
// M is singular - three points, a planar set - where two eigenvalues of the polynomial approach each other.  A bounded
// number of sweeps whatever the input holds (NaN included).
__host__ __device__ inline void horn_rotation(const double M[9], double R[9]) {
  const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      diag += A[p][p] * A[p][p];
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    }
    if (off <= 1e-36 * diag || off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
        for (int k = 0; k < 4; ++k) {          // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = cs * akp - sn * akq;
          A[k][q] = sn * akp + cs * akq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {          // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = cs * apk - sn * aqk;
          A[q][k] = sn * apk + cs * aqk;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {          // V <- V J: the columns of V stay the eigenvectors
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
    }
  }
  double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0], top = A[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (A[j][j] > top) { top = A[j][j]; w = V[0][j]; x = V[1][j]; y = V[2][j]; z = V[3][j]; }
  const double nrm = sqrt((w * w + x * x) + (y * y + z * z));
  w /= nrm; x /= nrm; y /= nrm; z /= nrm;
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (y * z + w * x);         R[8] = w * w - x * x - y * y + z * z;
}

// |R p + t - q|
__device__ inline double score_dev(const double* R, const double* t, const float* p, const float* q) {
  const double px = p[0], py = p[1], pz = p[2];
  const double ex = (((R[0] * px + R[1] * py) + R[2] * pz) + t[0]) - (double)q[0];
  const double ey = (((R[3] * px + R[4] * py) + R[5] * pz) + t[1]) - (double)q[1];
  const double ez = (((R[6] * px + R[7] * py) + R[8] * pz) + t[2]) - (double)q[2];
  return sqrt((ex * ex + ey * ey) + ez * ez);
}

// Sum of K values per thread over the workgroup, left in v[] of EVERY thread.  `wred` is reused by the next call: the
// leading barrier keeps its writers behind the previous call's readers.
template <int K>
__device__ inline void score_block_sum(double (&v)[K], double (*wred)[16]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) wred[wv][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((wred[0][k] + wred[1][k]) + wred[2][k]) + wred[3][k];
}

// What thread 0 keeps of one seed: the best tm with its R, t, the largest of each of the five counts over the iterations,
// and the RMSD of the first iteration (the plain Kabsch RMSD over the starting set).
struct SeedBest {
  double tm = -1.0, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0}, cnt[5] = {0, 0, 0, 0, 0}, rmsd = 0.0;
};

// The loop of one seed over n packed pairs (pm[k], qn[k]): superpose on the set S (fl[k], the caller's start), score all
// pairs, keep the best tm (strict comparison: the earliest of equals stays), S' = {d < d_cut}; at most SC_ITERS times, until
// |S'| < 3 or S' = S.  EVERY thread of the workgroup calls it (barriers inside, every branch uniform); `best` is meaningful
// in thread 0; `wred` and `bc` (12 doubles) are LDS.  Bounded whatever the input holds (a NaN runs it to SC_ITERS).
__device__ inline void score_seed_loop(const float* pm, const float* qn, unsigned char* fl, int n, double lnorm, double d0,
                                       double d_cut, double (*wred)[16], double* bc, SeedBest& best) {
  const int tid = threadIdx.x;
  double& best_tm = best.tm;
  double* best_R = best.R;
  double* best_t = best.t;
  double* best_cnt = best.cnt;
  double& rmsd = best.rmsd;
  for (int it = 0; it < SC_ITERS; ++it) {
    // a thread owns the rows k = tid, tid + 256, ...: it alone reads and writes their flags
    double s7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += SC_THREADS)
      if (fl[k]) {
        s7[0] += 1.0;
        for (int c = 0; c < 3; ++c) { s7[1 + c] += (double)pm[3 * k + c]; s7[4 + c] += (double)qn[3 * k + c]; }
      }
    score_block_sum<7>(s7, wred);
    const double pc[3] = {s7[1] / s7[0], s7[2] / s7[0], s7[3] / s7[0]};
    const double qc[3] = {s7[4] / s7[0], s7[5] / s7[0], s7[6] / s7[0]};
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += SC_THREADS)
      if (fl[k]) {
        const double px = (double)pm[3 * k] - pc[0], py = (double)pm[3 * k + 1] - pc[1], pz = (double)pm[3 * k + 2] - pc[2];
        const double qx = (double)qn[3 * k] - qc[0], qy = (double)qn[3 * k + 1] - qc[1], qz = (double)qn[3 * k + 2] - qc[2];
        M[0] += px * qx; M[1] += px * qy; M[2] += px * qz;
        M[3] += py * qx; M[4] += py * qy; M[5] += py * qz;
        M[6] += pz * qx; M[7] += pz * qy; M[8] += pz * qz;
      }
    score_block_sum<9>(M, wred);
    if (tid == 0) {
      double R[9];
      horn_rotation(M, R);
      for (int c = 0; c < 9; ++c) bc[c] = R[c];
      for (int c = 0; c < 3; ++c) bc[9 + c] = qc[c] - ((R[3 * c] * pc[0] + R[3 * c + 1] * pc[1]) + R[3 * c + 2] * pc[2]);
    }
    __syncthreads();
    double R[9], t[3];
    for (int c = 0; c < 9; ++c) R[c] = bc[c];
    for (int c = 0; c < 3; ++c) t[c] = bc[9 + c];
    // tm sum, the five counts, |S'|, rows whose flag changed, sum of squares
    double s9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += SC_THREADS) {
      const double d = score_dev(R, t, pm + 3 * k, qn + 3 * k);
      const double r = d / d0;
      s9[0] += 1.0 / (1.0 + r * r);
      s9[1] += d < 0.5 ? 1.0 : 0.0;
      s9[2] += d < 1.0 ? 1.0 : 0.0;
      s9[3] += d < 2.0 ? 1.0 : 0.0;
      s9[4] += d < 4.0 ? 1.0 : 0.0;
      s9[5] += d < 8.0 ? 1.0 : 0.0;
      const unsigned char in = d < d_cut ? 1 : 0;
      s9[6] += (double)in;
      s9[7] += in != fl[k] ? 1.0 : 0.0;
      s9[8] += d * d;
      fl[k] = in;
    }
    score_block_sum<9>(s9, wred);
    if (tid == 0) {
      const double tm = s9[0] / lnorm;
      if (tm > best_tm) {
        best_tm = tm;
        for (int c = 0; c < 9; ++c) best_R[c] = R[c];
        for (int c = 0; c < 3; ++c) best_t[c] = t[c];
      }
      for (int c = 0; c < 5; ++c) best_cnt[c] = fmax(best_cnt[c], s9[1 + c]);
      if (it == 0) rmsd = sqrt(s9[8] / (double)n);       // the plain Kabsch RMSD where S starts as all n pairs (score.hip: seed 0)
    }
    // the same bits in every thread: a uniform branch.  (A NaN keeps the loop going to its bound.)
    if (s9[6] < 3.0 || s9[7] == 0.0) break;
  }
}

}  // namespace dmp
