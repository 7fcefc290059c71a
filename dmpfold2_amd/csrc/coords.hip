// Coordinate-side kernels: coord_fc, pair distances, best-of selection, the steric/bond
// minimiser (reference network.py:106-137) and the backbone builder (network.py:141-177).
// The reference evaluates these as chains of separately rounded float32 tensor ops, so
// floating-point contraction is switched off for this file.
#include "cluster.h"

#pragma clang fp contract(off)

namespace dmp {

// ca[i][c] = sum_k g[i][k] * W[c][k]                                     (network.py:255)
__global__ __launch_bounds__(192) void coord_fc_kernel(const float* __restrict__ g,
                                                       const float* __restrict__ w, int L,
                                                       float* __restrict__ ca) {
  const int i = blockIdx.x;
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc = 0.f;
  for (int k = lane; k < WIDTH; k += 64) acc = fmaf(g[(int64_t)i * WIDTH + k], w[c * WIDTH + k], acc);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) ca[i * 3 + c] = acc;
}

int coord_fc(dmp_ctx* c, const float* d_g, int L, float* d_ca, hipStream_t s) {
  hipLaunchKernelGGL(coord_fc_kernel, dim3(L), dim3(192), 0, s, d_g, c->W.fc, L, d_ca);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// emb[i] = [mat1d[:, i] | mds[i, :]]                                      (network.py:251)
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ mat1d,
                                                    const float* __restrict__ mds, int L,
                                                    float* __restrict__ emb) {
  const int i = blockIdx.x;
  for (int k = threadIdx.x; k < WIDTH + 8; k += 256)
    emb[(int64_t)i * (WIDTH + 8) + k] =
        k < WIDTH ? mat1d[(int64_t)k * L + i] : mds[(int64_t)i * 8 + (k - WIDTH)];
}

int build_embed(const float* d_mat1d, const float* d_mds, int L, float* d_emb, hipStream_t s) {
  hipLaunchKernelGGL(embed_kernel, dim3(L), dim3(256), 0, s, d_mat1d, d_mds, L, d_emb);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int R, int C,
                                                        float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    if (r0 + r < R && c0 + tx < C) tile[r][tx] = in[(int64_t)(r0 + r) * C + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (c0 + r < C && r0 + tx < R) out[(int64_t)(c0 + r) * R + r0 + tx] = tile[tx][r];
}

int transpose_f32(const float* d_in, int R, int C, float* d_out, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), 0, s, d_in, R, C,
                     d_out);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// clamp=1: sqrt(max(|ci-cj|^2, 1e-8)) (network.py:272); clamp=0: sqrt(|ci-cj|^2) (predict.py:143)
__global__ __launch_bounds__(256) void pairdist_kernel(const float* __restrict__ ca, int L, int clamp,
                                                       float* __restrict__ dmap) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= L) return;
  const float dx = ca[j * 3] - ca[i * 3], dy = ca[j * 3 + 1] - ca[i * 3 + 1],
              dz = ca[j * 3 + 2] - ca[i * 3 + 2];
  float s = (dx * dx + dy * dy) + dz * dz;
  if (clamp) s = fmaxf(s, 1e-8f);
  dmap[(int64_t)i * L + j] = sqrtf(s);
}

int pair_distances(const float* d_ca, int L, int clamp, float* d_dmap, hipStream_t s) {
  hipLaunchKernelGGL(pairdist_kernel, dim3(cdiv(L, 256), L), dim3(256), 0, s, d_ca, L, clamp, d_dmap);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

__global__ void fill_kernel(float* __restrict__ d, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = v;
}

int fill_f32(float* d, int64_t n, float v, hipStream_t s) {
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, d, n, v);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// best-of selection on the device (network.py:302-306: strict '>' on the mean logit)
__global__ __launch_bounds__(256) void select_best_kernel(const float* __restrict__ conf,
                                                          const float* __restrict__ ca, int L,
                                                          int pass, int rec_cap,
                                                          float* __restrict__ best_mean,
                                                          float* __restrict__ best_conf,
                                                          float* __restrict__ best_ca,
                                                          float* __restrict__ conf_means,
                                                          float* __restrict__ ca_pass,
                                                          float* __restrict__ best_pass) {
  __shared__ double red[256];
  __shared__ int take;
  double acc = 0.0;
  for (int i = threadIdx.x; i < L; i += 256) acc += (double)conf[i];
  const double sum = block_tree_sum_f64<256>(acc, red);
  if (threadIdx.x == 0) {
    const float mean = (float)(sum / (double)L);
    if (pass < rec_cap) conf_means[pass] = mean;
    take = (pass == 0) || (mean > best_mean[0]);
    if (take) {
      best_mean[0] = mean;
      best_pass[0] = (float)pass;        // the word keep_best_dm and emit_distmap read (exact below 2^24)
    }
  }
  __syncthreads();
  if (pass < rec_cap)
    for (int i = threadIdx.x; i < 3 * L; i += 256) ca_pass[(int64_t)pass * 3 * L + i] = ca[i];
  if (take) {
    for (int i = threadIdx.x; i < L; i += 256) best_conf[i] = conf[i];
    for (int i = threadIdx.x; i < 3 * L; i += 256) best_ca[i] = ca[i];
  }
}

int select_best(dmp_ctx* c, const float* d_conf, const float* d_ca, int L, int pass, int rec_cap,
                hipStream_t s) {
  hipLaunchKernelGGL(select_best_kernel, dim3(1), dim3(256), 0, s, d_conf, d_ca, L, pass, rec_cap,
                     c->best_mean, c->best_conf, c->best_ca, c->conf_means, c->ca_pass, c->best_pass);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// recycle_delta (option "recycle_tol_mA"): how far did this pass move the trace?
// ---------------------------------------------------------------------------------------
// d_p = sqrt(mean over i < j of (D(ca_p)_ij - D(seed_p)_ij)^2), D(x)_ij = sqrt(max(|x_i - x_j|^2, 1e-8)): the RMS change
// of the distance map the NEXT pass would be seeded with against the one THIS pass was seeded with (network.py:272 forms
// that map from the trace; here both maps are formed on the fly from the two traces in LDS, 2 x 3L floats, no L^2
// traffic).  Float64 throughout: at d = 1e-3 A the float32 rounding of two 30 A distances is a tenth of the value.
// Rows i are dealt round robin to the workgroups, a row's partners j to the threads; every thread sums its pairs in a
// fixed order, the workgroup's tree and the last arriver's loop over the partial sums (grid_sum_f64) are fixed too, so the value - and
// with it the stop decision - has the same bits however the workgroups are scheduled.  Workgroup 0 keeps the trace for
// the next pass's comparison (the two keep buffers alternate: nobody reads the one being written).  The last arriver
// records d_p and tells the host: {pass + 1, stop} in one word of pinned host memory, an ordinary store - the route of
// the pipeline's per-ticket fault words.
constexpr int RD_THREADS = 256;
constexpr int RD_MAX_WG = 64;

__host__ __device__ inline int recycle_delta_groups(int L) {
  const int g = L / 32;
  return g < 1 ? 1 : (g > RD_MAX_WG ? RD_MAX_WG : g);
}

// The one statement of d_p, which recycle_delta_kernel and pass_delta_kernel (option "score_passes") both evaluate: this
// thread's share of the pair sum over the two traces in LDS - workgroup blockIdx.x of gridDim.x, the same grid width in both
// kernels - and the value from the grid's total.
__device__ __forceinline__ double recycle_delta_pairs(const float* xa, const float* xb, int L) {
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  double acc = 0.0;
  for (int i = g; i < L - 1; i += G) {
    const double ax = xa[3 * i], ay = xa[3 * i + 1], az = xa[3 * i + 2];
    const double bx = xb[3 * i], by = xb[3 * i + 1], bz = xb[3 * i + 2];
    for (int j = i + 1 + tid; j < L; j += RD_THREADS) {
      const double ux = (double)xa[3 * j] - ax, uy = (double)xa[3 * j + 1] - ay, uz = (double)xa[3 * j + 2] - az;
      const double vx = (double)xb[3 * j] - bx, vy = (double)xb[3 * j + 1] - by, vz = (double)xb[3 * j + 2] - bz;
      const double da = sqrt(fmax((ux * ux + uy * uy) + uz * uz, 1e-8));
      const double db = sqrt(fmax((vx * vx + vy * vy) + vz * vz, 1e-8));
      const double e = da - db;
      acc += e * e;
    }
  }
  return acc;
}
__device__ __forceinline__ float recycle_delta_value(double sum, int L) {
  return (float)sqrt(sum / (0.5 * (double)L * (double)(L - 1)));
}

struct RecycleDeltaArgs {
  const float* ca;       // [L][3] this pass's trace
  const float* seed;     // [L][3] the trace whose distance map seeded this pass (null: pass 0, no delta)
  float* keep;           // [L][3] <- ca
  int L, pass, rec_cap;
  float tol;             // A
  float* pass_delta;     // [rec_cap]
  double* partial;       // [RD_MAX_WG]
  unsigned* counter;     // zero between launches
  int* host_word;        // pinned: ((pass + 1) << 1) | stop
};

__global__ __launch_bounds__(RD_THREADS) void recycle_delta_kernel(RecycleDeltaArgs a) {
  extern __shared__ float sm[];          // 2 x 3L coordinates
  __shared__ double red[RD_THREADS];
  const int L = a.L, tid = threadIdx.x, g = blockIdx.x;
  if (g == 0)
    for (int i = tid; i < 3 * L; i += RD_THREADS) a.keep[i] = a.ca[i];
  if (!a.seed) {                         // pass 0 (one workgroup): nothing to compare with
    if (tid == 0) {
      if (a.pass < a.rec_cap) a.pass_delta[a.pass] = __builtin_inff();
      *a.host_word = (a.pass + 1) << 1;
    }
    return;
  }
  float* xa = sm;
  float* xb = sm + 3 * L;
  for (int i = tid; i < 3 * L; i += RD_THREADS) { xa[i] = a.ca[i]; xb[i] = a.seed[i]; }
  __syncthreads();
  const double acc = recycle_delta_pairs(xa, xb, L);
  double sum;
  if (grid_sum_f64<RD_THREADS>(acc, red, a.partial, a.counter, &sum)) {
    const float d = recycle_delta_value(sum, L);
    if (a.pass < a.rec_cap) a.pass_delta[a.pass] = d;
    const int stop = d <= a.tol ? 1 : 0;           // false for NaN
    *a.host_word = ((a.pass + 1) << 1) | stop;
  }
}

int recycle_delta(dmp_ctx* c, const float* d_ca, int L, int pass, int rec_cap, hipStream_t s) {
  RecycleDeltaArgs a{};
  a.ca = d_ca;
  a.seed = pass > 0 ? c->delta_keep + (int64_t)((pass - 1) & 1) * 3 * c->max_L : nullptr;
  a.keep = c->delta_keep + (int64_t)(pass & 1) * 3 * c->max_L;
  a.L = L; a.pass = pass; a.rec_cap = rec_cap;
  a.tol = (float)c->run.tol_mA * 1e-3f;
  a.pass_delta = c->pass_delta;
  a.partial = c->delta_partial;
  a.counter = c->delta_counter;
  a.host_word = c->delta_host;
  const int G = pass > 0 ? recycle_delta_groups(L) : 1;
  hipLaunchKernelGGL(recycle_delta_kernel, dim3(G), dim3(RD_THREADS), pass > 0 ? sizeof(float) * 6 * L : 0, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// Option "score_passes": d_p of every recorded pass p >= 1 in one launch at the prediction's end, the pass as blockIdx.y.
// select_best recorded in ca_pass[p - 1] the very trace recycle_delta keeps as pass p's seed (pass 0's after its
// minimiser steps), so the operands, the grid width, the sums' order and with them the bits are those of pass_delta[p] -
// whether or not "recycle_tol_mA" ran.  Each pass has its own partial sums and its own ticket.
struct PassDeltaArgs {
  const float* ca_pass;  // [rows][L][3]
  int L;
  float* rows;           // the pass block's rows: d_p goes to rows[PASS_ROW * p + 1]
  double* partial;       // [rows][RD_MAX_WG]
  unsigned* counter;     // [rows] zero between launches
};

__global__ __launch_bounds__(RD_THREADS) void pass_delta_kernel(PassDeltaArgs a) {
  extern __shared__ float sm[];          // 2 x 3L coordinates
  __shared__ double red[RD_THREADS];
  const int L = a.L, tid = threadIdx.x, p = (int)blockIdx.y + 1;
  float* xa = sm;
  float* xb = sm + 3 * L;
  const float* ca = a.ca_pass + (int64_t)p * 3 * L;
  for (int i = tid; i < 3 * L; i += RD_THREADS) { xa[i] = ca[i]; xb[i] = ca[i - 3 * L]; }
  __syncthreads();
  const double acc = recycle_delta_pairs(xa, xb, L);
  double sum;
  if (grid_sum_f64<RD_THREADS>(acc, red, a.partial + (int64_t)p * RD_MAX_WG, a.counter + p, &sum))
    a.rows[PASS_ROW * p + 1] = recycle_delta_value(sum, L);
}

int pass_deltas(dmp_ctx* c, int L, int rows, float* d_rows, double* d_partial, unsigned* d_counter, hipStream_t s) {
  if (rows < 2) return DMP_OK;
  PassDeltaArgs a{c->ca_pass, L, d_rows, d_partial, d_counter};
  hipLaunchKernelGGL(pass_delta_kernel, dim3(recycle_delta_groups(L), rows - 1), dim3(RD_THREADS), sizeof(float) * 6 * L, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// option "emit_distmap": the chosen pass's predicted distance map (include/dmpfold_hip.h)
// ---------------------------------------------------------------------------------------
// keep_best_dm runs in the pass tail behind select_best.  Every workgroup reads the pass select_best took last and
// leaves at once unless it is this one; otherwise head0 - the plane the last block's norm kernel left, which nothing
// has overwritten in the tail unit - becomes best_dm, dm_ij = distmap_entry(h0_ij, h0_ji).  A workgroup owns the tile
// pair (bi <= bj): tiles (bi, bj) and (bj, bi) of h0 go to LDS with row-contiguous (coalesced) reads, and both mirrored
// tiles of dm are written row-contiguously, the transposed operand coming from LDS.  64 x 64 floats per tile: a wave
// reads or writes one 256-byte row segment per instruction.  The LDS rows are padded to 65 words: ds_read_b32 and
// ds_write_b32 resolve banks as (word address) % 32 within each 32-lane half, the row access r * 65 + lane is
// conflict-free at any pitch, and the column access lane * 65 + r lands on bank (lane + r) % 32 - 32 different banks
// per half - where pitch 64 would put a whole half on one bank.  2 x 64 x 65 x 4 B = 33 KB per workgroup.
constexpr int KD_TILE = 64;
constexpr int KD_PITCH = KD_TILE + 1;
constexpr int KD_THREADS = 256;

__global__ __launch_bounds__(KD_THREADS) void keep_best_dm_kernel(const float* __restrict__ h0,
                                                                  const float* __restrict__ best_pass, int L,
                                                                  int pass, float* __restrict__ best_dm) {
  __shared__ float ta[KD_TILE * KD_PITCH];     // h0 tile (bi, bj)
  __shared__ float tb[KD_TILE * KD_PITCH];     // h0 tile (bj, bi)
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  if (best_pass[0] != (float)pass) return;
  const int i0 = bi * KD_TILE, j0 = bj * KD_TILE;
  const int tx = threadIdx.x & (KD_TILE - 1), ty = threadIdx.x / KD_TILE;
  constexpr int ROWS = KD_THREADS / KD_TILE;
  for (int r = ty; r < KD_TILE; r += ROWS) {
    float a = 0.f, b = 0.f;
    if (i0 + r < L && j0 + tx < L) a = h0[(int64_t)(i0 + r) * L + j0 + tx];
    if (j0 + r < L && i0 + tx < L) b = h0[(int64_t)(j0 + r) * L + i0 + tx];
    ta[r * KD_PITCH + tx] = a;
    tb[r * KD_PITCH + tx] = b;
  }
  __syncthreads();
  for (int r = ty; r < KD_TILE; r += ROWS) {
    // dm[i0 + r][j0 + tx] from h0[i0 + r][j0 + tx] and h0[j0 + tx][i0 + r]
    if (i0 + r < L && j0 + tx < L)
      best_dm[(int64_t)(i0 + r) * L + j0 + tx] = distmap_entry(ta[r * KD_PITCH + tx], tb[tx * KD_PITCH + r]);
    // the mirrored tile: dm[j0 + r][i0 + tx] from h0[j0 + r][i0 + tx] and h0[i0 + tx][j0 + r]
    if (bi != bj && j0 + r < L && i0 + tx < L)
      best_dm[(int64_t)(j0 + r) * L + i0 + tx] = distmap_entry(tb[r * KD_PITCH + tx], ta[tx * KD_PITCH + r]);
  }
}

int keep_best_dm(dmp_ctx* c, int L, int pass, hipStream_t s) {
  const int T = cdiv(L, KD_TILE);
  hipLaunchKernelGGL(keep_best_dm_kernel, dim3(T, T), dim3(KD_THREADS), 0, s, c->head0, c->best_pass, L, pass,
                     c->best_dm);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// emit_distmap runs in dmp_predict_end behind ca_to_backbone: best_dm goes to the caller's buffer behind the
// confidences, followed by {best_pass, passes_run, map_rms},
//   map_rms = sqrt(mean over i < j of (dm_ij - |ca_i - ca_j|)^2)     [Angstrom],
// ca the final, refined trace the backbone was built from: distances in float64 from the float32 coordinates, no clamp.
// The sum is formed the way recycle_delta forms its own: the trace in LDS, rows dealt round robin to the workgroups, a
// row's partners to the threads, per-thread sums in a fixed order, a fixed tree, and the last arriver adds the partial
// sums in index order and resets the counter - the same bits on every run.  The workgroup that owns a row copies it.
struct EmitDistmapArgs {
  const float* best_dm;    // [L][L]
  const float* ca;         // [L][3]
  const float* best_pass;  // [1]
  int L, passes_run;
  float* out;              // [L][L]
  float* info;             // [3] best_pass, passes_run, map_rms
  double* partial;         // [RD_MAX_WG]
  unsigned* counter;       // zero between launches
};

__global__ __launch_bounds__(RD_THREADS) void emit_distmap_kernel(EmitDistmapArgs a) {
  extern __shared__ float sm[];          // 3L coordinates
  __shared__ double red[RD_THREADS];
  const int L = a.L, tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  for (int i = tid; i < 3 * L; i += RD_THREADS) sm[i] = a.ca[i];
  __syncthreads();
  double acc = 0.0;
  for (int i = g; i < L; i += G) {
    const double ax = sm[3 * i], ay = sm[3 * i + 1], az = sm[3 * i + 2];
    const float* src = a.best_dm + (int64_t)i * L;
    float* dst = a.out + (int64_t)i * L;
    for (int j = tid; j < L; j += RD_THREADS) {
      const float dm = src[j];
      dst[j] = dm;
      if (j > i) {
        const double ux = (double)sm[3 * j] - ax, uy = (double)sm[3 * j + 1] - ay, uz = (double)sm[3 * j + 2] - az;
        const double e = (double)dm - sqrt((ux * ux + uy * uy) + uz * uz);
        acc += e * e;
      }
    }
  }
  double sum;
  if (grid_sum_f64<RD_THREADS>(acc, red, a.partial, a.counter, &sum)) {
    a.info[0] = a.best_pass[0];
    a.info[1] = (float)a.passes_run;
    a.info[2] = (float)sqrt(sum / (0.5 * (double)L * (double)(L - 1)));
  }
}

int emit_distmap(dmp_ctx* c, const float* d_ca, int L, int passes_run, float* d_map, float* d_info, hipStream_t s) {
  EmitDistmapArgs a{};
  a.best_dm = c->best_dm;
  a.ca = d_ca;
  a.best_pass = c->best_pass;
  a.L = L; a.passes_run = passes_run;
  a.out = d_map; a.info = d_info;
  a.partial = c->rms_partial;
  a.counter = c->rms_counter;
  hipLaunchKernelGGL(emit_distmap_kernel, dim3(recycle_delta_groups(L)), dim3(RD_THREADS), sizeof(float) * 3 * L, s, a);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

// ---------------------------------------------------------------------------------------
// refine_coords: all steps in one launch, coordinates double-buffered in LDS
// ---------------------------------------------------------------------------------------
// T threads share a residue j, each summing the steric term over a contiguous slice of the
// partners i; the slices are then added in order, followed by the two bond terms.
//
// Option "restrain_milli" (include/dmpfold_hip.h): the final refinement's steps also pull every pair with |i - j| >= 2
// whose predicted distance t = best_dm[i][j] lies below the cutoff towards t, a_j -= k clamp(d - t, +-3) (x_j - x_i) / d.
// The reference has no such term.  The thread that owns residue j reads best_dm[i * L + j] - the map is exactly symmetric
// (keep_best_dm), and the threads of a wave own neighbouring j, so a wave reads one contiguous piece of row i per partner -
// from L2 in every step: a workgroup's share of the map is Lg x L floats, read once per step - more than a CU's LDS from
// about L = 800 on, so it is not staged there at any length (one placement, one set of bits); the map fits the XCD's L2 up to
// L = 1000 and the Infinity Cache always.  One sqrt and one set of quotients per pair serve both terms.  A map entry that
// is NaN fails `t < cut` and its pair is skipped.
struct Restraint {
  const float* dm;     // [L][L] best_dm
  float k, cut;        // force constant, cutoff (A)
};

// The pair loop of both forms of the minimiser: the acceleration of residue j from the partners [i0, i1).  RESTRAIN =
// false is the reference's steric term alone.
template <bool RESTRAIN>
__device__ __forceinline__ void refine_pairs(const float* cur, int L, int j, int i0, int i1, const Restraint& r,
                                             float& ax, float& ay, float& az) {
  const float xj = cur[3 * j], yj = cur[3 * j + 1], zj = cur[3 * j + 2];
  for (int i = i0; i < i1; ++i) {
    float t = 0.f;
    if constexpr (RESTRAIN) t = r.dm[(int64_t)i * L + j];       // always in bounds: issued ahead of the sqrt and the divides
    const float dx = xj - cur[3 * i], dy = yj - cur[3 * i + 1], dz = zj - cur[3 * i + 2];
    const float d_raw = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float d = fminf(fmaxf(d_raw, 0.01f), 10.0f);
    const float viol = (d < 3.0f) ? (3.0f - d) : 0.0f;
    const float f = 100.0f * viol;
    if constexpr (!RESTRAIN) {
      ax += f * (dx / d);
      ay += f * (dy / d);
      az += f * (dz / d);
    } else {
      // One set of quotients serves both terms: dr = d wherever d < 10, and beyond that f is 0 and f * (dx / d) the same
      // signed zero as f * (dx / dr) - the steric term keeps the bits of the plain loop.
      const float dr = fmaxf(d_raw, 0.01f);
      const float qx = dx / dr, qy = dy / dr, qz = dz / dr;
      ax += f * qx;
      ay += f * qy;
      az += f * qz;
      if ((i - j >= 2 || j - i >= 2) && t < r.cut) {            // `t < cut` is false for NaN
        const float e = fminf(fmaxf(dr - t, -3.0f), 3.0f);
        const float ke = r.k * e;
        ax -= ke * qx;
        ay -= ke * qy;
        az -= ke * qz;
      }
    }
  }
}

template <bool RESTRAIN>
__global__ __launch_bounds__(1024) void refine_kernel(float* __restrict__ ca, int L, int steps, Restraint r) {
  extern __shared__ float sm[];          // 2 x 3L coordinates + T x 3L partial sums
  float* cur = sm;
  float* nxt = sm + 3 * L;
  float* part = sm + 6 * L;
  const int T = L >= 1024 ? 1 : (1024 / L > 8 ? 8 : 1024 / L);
  const int chunk = (L + T - 1) / T;
  for (int i = threadIdx.x; i < 3 * L; i += 1024) cur[i] = ca[i];
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    for (int idx = threadIdx.x; idx < T * L; idx += 1024) {
      const int j = idx % L, sub = idx / L;
      const int i0 = sub * chunk, i1 = (i0 + chunk < L) ? i0 + chunk : L;
      float ax = 0.f, ay = 0.f, az = 0.f;
      refine_pairs<RESTRAIN>(cur, L, j, i0, i1, r, ax, ay, az);
      part[(sub * L + j) * 3] = ax;
      part[(sub * L + j) * 3 + 1] = ay;
      part[(sub * L + j) * 3 + 2] = az;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += 1024) {
      const float xj = cur[3 * j], yj = cur[3 * j + 1], zj = cur[3 * j + 2];
      float ax = part[3 * j], ay = part[3 * j + 1], az = part[3 * j + 2];
      for (int sub = 1; sub < T; ++sub) {
        ax += part[(sub * L + j) * 3];
        ay += part[(sub * L + j) * 3 + 1];
        az += part[(sub * L + j) * 3 + 2];
      }
      if (j < L - 1) {   // bond to j+1: accels[:-1] += accels_cov
        const float dx = cur[3 * j + 3] - xj, dy = cur[3 * j + 4] - yj, dz = cur[3 * j + 5] - zj;
        const float d = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 0.1f);
        const float f = 100.0f * fminf(d - 3.78f, 3.0f);
        ax += f * (dx / d);
        ay += f * (dy / d);
        az += f * (dz / d);
      }
      if (j > 0) {       // bond from j-1: accels[1:] -= accels_cov
        const float dx = xj - cur[3 * j - 3], dy = yj - cur[3 * j - 2], dz = zj - cur[3 * j - 1];
        const float d = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 0.1f);
        const float f = 100.0f * fminf(d - 3.78f, 3.0f);
        ax -= f * (dx / d);
        ay -= f * (dy / d);
        az -= f * (dz / d);
      }
      nxt[3 * j] = xj + fminf(fmaxf(ax, -100.0f), 100.0f) * 0.001f;
      nxt[3 * j + 1] = yj + fminf(fmaxf(ay, -100.0f), 100.0f) * 0.001f;
      nxt[3 * j + 2] = zj + fminf(fmaxf(az, -100.0f), 100.0f) * 0.001f;
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  for (int i = threadIdx.x; i < 3 * L; i += 1024) ca[i] = cur[i];
}

// The same iteration on a cluster of RF_G workgroups (one XCD): workgroup g owns the residues
// [g Lg, (g+1) Lg), keeps a copy of all coordinates in LDS, and per step computes the accelerations of
// its residues (T threads per residue, each over a contiguous slice of the partners, slices added in
// order), publishes the new coordinates as granules and gathers the others' (the hand-off of cluster.h,
// DESIGN section 4).
constexpr int RF_G = 16;          // workgroups of the cluster
constexpr int RF_THREADS = 512;    // 8 waves of 54 VGPRs: fits beside two convolution workgroups on a CU
constexpr ClusterLayout refine_layout(int L) { return {(int64_t)2 * 3 * L, 1}; }   // [2 parity][3L] granules, the placement header
static_assert(refine_layout(513).words() == 6 * 513 + 2 && refine_layout(513).header() == 6 * 513, "granule buffer of the minimiser");
int64_t refine_cluster_need(int max_L) { return refine_layout(max_L).words(); }
struct RefineArgs : ClusterArgs {
  float* ca;
  int L, steps, xcd;
  Restraint r;         // option "restrain_milli" (the RESTRAIN = true instantiation reads it)
};

__host__ __device__ inline int refine_slices(int L) {
  const int Lg = (L + RF_G - 1) / RF_G;
  const int t = RF_THREADS / Lg;
  return t < 1 ? 1 : (t > 32 ? 32 : t);
}

// grid: 8 * RF_G blocks (only ids with id % 8 == xcd work)   block: RF_THREADS   dynamic LDS: see refine_coords
template <bool RESTRAIN>
__global__ __launch_bounds__(RF_THREADS) void refine_cluster_kernel(RefineArgs a) {
  extern __shared__ float sm[];          // 3L coordinates + T x 3 Lg partial sums
  __shared__ int sh_abort, sh_local;
  if ((int)(blockIdx.x & 7) != a.xcd) return;
  const int g = blockIdx.x >> 3, L = a.L, tid = threadIdx.x;
  const int Lg = (L + RF_G - 1) / RF_G;
  const int j_lo = g * Lg;
  const int nj = (j_lo + Lg <= L ? Lg : L - j_lo);
  if (nj <= 0) return;                   // short chains: the last workgroups own nothing
  const int T = refine_slices(L);
  const int chunk = (L + T - 1) / T;
  float* cur = sm;
  float* part = sm + 3 * L;
  for (int i = tid; i < 3 * L; i += RF_THREADS) cur[i] = a.ca[i];
  const bool local = cluster_begin(&sh_local, &sh_abort, a.gx + refine_layout(L).header(), (L + Lg - 1) / Lg /* the owners of residues */, a.allow_local);
  for (int step = 0; step < a.steps; ++step) {
    const unsigned epoch = (unsigned)step + 1u;
    granule* gx = a.gx + (int64_t)(step & 1) * 3 * L;
    for (int idx = tid; idx < T * nj; idx += RF_THREADS) {
      const int jl = idx % nj, sub = idx / nj, j = j_lo + jl;
      const int i0 = sub * chunk, i1 = (i0 + chunk < L) ? i0 + chunk : L;
      float ax = 0.f, ay = 0.f, az = 0.f;
      refine_pairs<RESTRAIN>(cur, L, j, i0, i1, a.r, ax, ay, az);
      part[(sub * nj + jl) * 3] = ax;
      part[(sub * nj + jl) * 3 + 1] = ay;
      part[(sub * nj + jl) * 3 + 2] = az;
    }
    __syncthreads();
    if (tid < nj) {
      const int jl = tid, j = j_lo + jl;
      const float xj = cur[3 * j], yj = cur[3 * j + 1], zj = cur[3 * j + 2];
      float ax = part[3 * jl], ay = part[3 * jl + 1], az = part[3 * jl + 2];
      for (int sub = 1; sub < T; ++sub) {
        ax += part[(sub * nj + jl) * 3];
        ay += part[(sub * nj + jl) * 3 + 1];
        az += part[(sub * nj + jl) * 3 + 2];
      }
      if (j < L - 1) {   // bond to j+1: accels[:-1] += accels_cov
        const float dx = cur[3 * j + 3] - xj, dy = cur[3 * j + 4] - yj, dz = cur[3 * j + 5] - zj;
        const float d = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 0.1f);
        const float f = 100.0f * fminf(d - 3.78f, 3.0f);
        ax += f * (dx / d);
        ay += f * (dy / d);
        az += f * (dz / d);
      }
      if (j > 0) {       // bond from j-1: accels[1:] -= accels_cov
        const float dx = xj - cur[3 * j - 3], dy = yj - cur[3 * j - 2], dz = zj - cur[3 * j - 1];
        const float d = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 0.1f);
        const float f = 100.0f * fminf(d - 3.78f, 3.0f);
        ax -= f * (dx / d);
        ay -= f * (dy / d);
        az -= f * (dz / d);
      }
      const float nx = xj + fminf(fmaxf(ax, -100.0f), 100.0f) * 0.001f;
      const float ny = yj + fminf(fmaxf(ay, -100.0f), 100.0f) * 0.001f;
      const float nz = zj + fminf(fmaxf(az, -100.0f), 100.0f) * 0.001f;
      cluster_publish_f32(&gx[3 * j], nx, epoch, local);
      cluster_publish_f32(&gx[3 * j + 1], ny, epoch, local);
      cluster_publish_f32(&gx[3 * j + 2], nz, epoch, local);
    }
    __syncthreads();                     // every thread has read the old coordinates
    for (int i = tid; i < 3 * L; i += RF_THREADS) {          // one granule at a time; a time-out shows in sh_abort
      granule x[1][1];
      cluster_gather(x, 1, epoch, REFINE_GATHER_BOUND, &sh_abort, [&](int, int) { return &gx[i]; });
      cur[i] = granule_f32(x[0][0]);
    }
    __syncthreads();                     // cur holds the new coordinates
    if (sh_abort) break;                 // the same word in every thread: nothing writes it between this barrier and the next gather
  }
  if (sh_abort && tid == 0) atomicOr(a.abort_flag, DMP_FAULT_REFINE_HANDOFF);
  for (int i = tid; i < 3 * nj; i += RF_THREADS) a.ca[3 * j_lo + i] = cur[3 * j_lo + i];
}

// `restrain`: the steps of the prediction's final refinement with option "restrain_milli" on - the map is c->best_dm, which
// keep_best_dm filled in the pass tails, the constants are the prediction's own (c->run)
int refine_coords(dmp_ctx* c, float* d_ca, int L, int steps, hipStream_t s, bool restrain) {
  if (steps <= 0) return DMP_OK;
  Restraint r{};
  if (restrain) {
    r.dm = c->best_dm;
    r.k = (float)c->run.restrain / 1000.0f;
    r.cut = (float)c->run.restrain_cut / 1000.0f;
  }
  if ((c->refine_single && L <= 1280) || L < 2 * RF_G) {      // one workgroup: (6 + 3 T) L floats of LDS
    const int T = L >= 1024 ? 1 : (1024 / L > 8 ? 8 : 1024 / L);
    const auto kernel = restrain ? refine_kernel<true> : refine_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(1024), sizeof(float) * (6 + 3 * T) * L, s, d_ca, L, steps, r);
    DMP_LAUNCH_CHECK();
    return DMP_OK;
  }
  RefineArgs a{};
  a.ca = d_ca; a.L = L; a.steps = steps; a.xcd = c->refine_xcd;
  a.r = r;
  const int Lg = (L + RF_G - 1) / RF_G;
  return cluster_launch(c, s, restrain ? refine_cluster_kernel<true> : refine_cluster_kernel<false>, RF_G, RF_THREADS,
                        sizeof(float) * (3 * L + 3 * refine_slices(L) * Lg), c->refine_gx, refine_layout(L), a);
}

// ---------------------------------------------------------------------------------------
// backbone from the C-alpha trace + sigmoid of the confidence logits
// ---------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* p, int i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// The packed-f32 hazard: v_pk_{mul,add,fma}_f32 with op_sel[0] = 0, op_sel[1] = 1
// return 0 in lanes 48..63 about once per 100 executions while f16 / bf16 MFMA waves share the SIMD.
// The vectoriser produces that form for the cross products below, so this file is compiled with
// -fno-slp-vectorize (dmpfold2_amd/build.py) and tools/isa_lint.py checks that no kernel of the library
// contains it.
__device__ __forceinline__ V3 dvd(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float nrm(V3 a) { return sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z); }
__device__ __forceinline__ V3 unit(V3 a) { return dvd(a, fmaxf(nrm(a), 1e-12f)); }

__device__ __forceinline__ V3 ext_at(const float* ca, int L, int t) {
  // t = 0: virtual N-terminal CA; 1..L: ca[t-1]; L+1: virtual C-terminal CA
  if (t >= 1 && t <= L) return ld3(ca, t - 1);
  if (t == 0) {
    const V3 a0 = ld3(ca, 0), a1 = ld3(ca, 1), a2 = ld3(ca, 2);
    return add(a0, mul(unit(cross(sub(a0, a1), sub(a2, a1))), 3.82f));
  }
  const V3 z0 = ld3(ca, L - 1), z1 = ld3(ca, L - 2), z2 = ld3(ca, L - 3);
  return add(z0, mul(unit(cross(sub(z0, z1), sub(z2, z1))), 3.82f));
}

// N, CA, C, O, CB of residue r from the trace: the one statement both kernels below evaluate, so that a native trace
// (option "assign_ss") gets the backbone the model's trace would get, bit for bit
__device__ __forceinline__ void backbone_residue(const float* __restrict__ ca, int L, int r, float sxc, float syc,
                                                 float* __restrict__ coords) {
  const V3 e0 = ext_at(ca, L, r), e1 = ext_at(ca, L, r + 1), e2 = ext_at(ca, L, r + 2);
  const V3 prev = sub(e0, e1), nxt = sub(e2, e1);
  const V3 mid0 = dvd(add(e1, e0), 2.0f);          // between ext[r] and ext[r+1]
  const V3 mid1 = dvd(add(e2, e1), 2.0f);          // between ext[r+1] and ext[r+2]
  const V3 nr = unit(cross(prev, nxt));
  const V3 n_at = add(sub(mid0, dvd(prev, 8.0f)), dvd(nr, 4.0f));
  V3 c_at, o_at;
  if (r < L - 1) {
    const V3 e3 = ext_at(ca, L, r + 3);
    const V3 prev1 = sub(e1, e2), nxt1 = sub(e3, e2);
    const V3 nr1 = unit(cross(prev1, nxt1));
    c_at = sub(add(mid1, dvd(prev1, 8.0f)), dvd(nr1, 2.0f));
    o_at = sub(mid1, mul(nr1, 1.8f));
  } else {
    c_at = add(sub(mid1, dvd(nxt, 8.0f)), dvd(nr, 2.0f));
    o_at = add(mid1, mul(nr, 2.0f));
  }
  const V3 vn = sub(e1, n_at), vc = sub(e1, c_at);
  const V3 cr = cross(vn, vc);
  const V3 vb = add(vn, vc);
  // Python `const / tensor` is evaluated as tensor.reciprocal() * const
  const float sx = (1.0f / nrm(vb)) * sxc, sy = (1.0f / nrm(cr)) * syc;
  const V3 cb = add(add(e1, mul(vb, sx)), mul(cr, sy));
  float* o = coords + (int64_t)r * 15;
  o[0] = n_at.x; o[1] = n_at.y; o[2] = n_at.z;
  o[3] = e1.x;   o[4] = e1.y;   o[5] = e1.z;
  o[6] = c_at.x; o[7] = c_at.y; o[8] = c_at.z;
  o[9] = o_at.x; o[10] = o_at.y; o[11] = o_at.z;
  o[12] = cb.x;  o[13] = cb.y;  o[14] = cb.z;
}

__global__ __launch_bounds__(256) void backbone_kernel(const float* __restrict__ ca,
                                                       const float* __restrict__ logit, int L,
                                                       float sxc, float syc,
                                                       float* __restrict__ coords,
                                                       float* __restrict__ conf) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= L) return;
  backbone_residue(ca, L, r, sxc, syc, coords);
  conf[r] = 1.0f / (1.0f + expf(-logit[r]));
}

__global__ __launch_bounds__(256) void backbone_trace_kernel(const float* __restrict__ ca, int L, float sxc, float syc,
                                                             float* __restrict__ coords) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= L) return;
  backbone_residue(ca, L, r, sxc, syc, coords);
}

static void backbone_constants(float* sxc, float* syc) {
  const double ang = 3.14159265358979323846 / 2.0 - asin(1.0 / sqrt(3.0));
  *sxc = (float)(1.5 * cos(ang));
  *syc = (float)(1.5 * sin(ang));
}

int ca_to_backbone(const float* d_ca, const float* d_logit, int L, float* d_coords,
                   float* d_conf_out, hipStream_t s) {
  float sxc, syc;
  backbone_constants(&sxc, &syc);
  hipLaunchKernelGGL(backbone_kernel, dim3(cdiv(L, 256)), dim3(256), 0, s, d_ca, d_logit, L, sxc,
                     syc, d_coords, d_conf_out);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

int trace_to_backbone(const float* d_ca, int L, float* d_coords, hipStream_t s) {
  float sxc, syc;
  backbone_constants(&sxc, &syc);
  hipLaunchKernelGGL(backbone_trace_kernel, dim3(cdiv(L, 256)), dim3(256), 0, s, d_ca, L, sxc, syc, d_coords);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

}  // namespace dmp
