// The hand-off between the workgroups of a cluster kernel - seq_gru_kernel (gru.hip), refine_cluster_kernel (coords.hip),
// tridiag_cluster_kernel (mds.hip) - and its only text.  DESIGN section 4, "The cluster hand-off", describes the protocol.
#pragma once
#include "common.h"

namespace dmp {

// ---- granules: 8 bytes {epoch : 32 | value : 32}, the data is the flag; a float64 travels as two, its halves under one epoch ----
typedef unsigned long long granule;
__device__ __forceinline__ granule granule_pack(unsigned epoch, unsigned bits) { return ((granule)epoch << 32) | (granule)bits; }
__device__ __forceinline__ bool granule_has(granule x, unsigned epoch) { return (unsigned)(x >> 32) == epoch; }
__device__ __forceinline__ float granule_f32(granule x) { return __uint_as_float((unsigned)x); }
__device__ __forceinline__ double granule_f64(granule lo, granule hi) { return __longlong_as_double((long long)((lo & 0xffffffffull) | (hi << 32))); }

// A kernel's granule buffer: the two parity arrays (`granules` together), then `headers` placement headers of two words.  Each
// kernel states its layout beside itself; the allocation (api.hip: *_cluster_need), the zeroing and the kernel's header pointer use it.
struct ClusterLayout {
  int64_t granules; int headers;
  constexpr int64_t header(int i = 0) const { return granules + 2 * i; }
  constexpr int64_t words() const { return granules + 2 * headers; }
};
int64_t seq_gru_cluster_need(), refine_cluster_need(int max_L), tridiag_cluster_need(int max_L);   // words of a context's buffers

// ---- placement and publication ----------------------------------------------------------------------------------------
// Granules are gathered with sc1 loads (agent scope: past the L1, served by the L2).  An agent-scope STORE is written through to
// the memory side so that every XCD can see it: measured (tools/ubench_handoff.hip) 450 ns one way, 2.78 us per step of the
// sequence GRU.  A PLAIN store stops in the L2 of the XCD its workgroup runs on, where the sc1 loads of workgroups on THAT XCD
// find it: 284 ns one way, 1.29 us per step, the same bits - and never seen from another XCD.  So the cluster checks where it
// runs: every workgroup ORs the bit of its XCC id (hardware register) into the header's mask word and counts itself in; when all
// `members` have arrived, a mask with one bit set means plain stores are safe.  True for "one XCD" (call from one thread per
// workgroup; bounded wait: false on a timeout or with `allow` = false, option "cluster_local" = 0 - agent-scope stores work wherever the members run).
__device__ __forceinline__ bool cluster_on_one_xcd(granule* hdr, int members, bool allow = true) {
  if (!allow) return false;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  __hip_atomic_fetch_or(&hdr[0], 1ull << (xcc & 15u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(&hdr[1], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  for (unsigned spins = 0; spins < 2000000u; ++spins) {
    if (__hip_atomic_load(&hdr[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned long long)members) {
      const unsigned long long mask = __hip_atomic_load(&hdr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return (mask & (mask - 1)) == 0;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}
// The prologue behind a kernel's XCD filter, called by every thread of the workgroup (one barrier inside): thread 0 clears
// the workgroup's abort word (`sh_abort`, null in the sequence GRU, which has none) and asks where the `members` run.
__device__ __forceinline__ bool cluster_begin(int* sh_local, int* sh_abort, granule* hdr, int members, int allow_local) {
  if (threadIdx.x == 0) {
    if (sh_abort) *sh_abort = 0;
    *sh_local = cluster_on_one_xcd(hdr, members, allow_local != 0) ? 1 : 0;
  }
  __syncthreads();
  return *sh_local != 0;
}
__device__ __forceinline__ void cluster_publish(granule* p, granule v, bool local) {   // publication of a granule: `local` = cluster_begin
  if (local) asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(p), "v"(v) : "memory");
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cluster_publish_f32(granule* p, float v, unsigned epoch, bool local) { cluster_publish(p, granule_pack(epoch, __float_as_uint(v)), local); }
__device__ __forceinline__ void cluster_publish_f64(granule* lo, granule* hi, double v, unsigned epoch, bool local) {
  const granule bits = (granule)__double_as_longlong(v);
  cluster_publish(lo, granule_pack(epoch, (unsigned)bits), local);
  cluster_publish(hi, granule_pack(epoch, (unsigned)(bits >> 32)), local);
}

// ---- the bounded gather -----------------------------------------------------------------------------------------------
// Waits until the first `count` of this thread's N elements, K granules each at at(i, c), carry `epoch`; q receives them.  A
// sweep loads all of them, then tests (it costs an L2 round trip whatever it loads); false after more than `bound` sweeps.
// A thread leaves when its own granules are there; one at the bound sets the workgroup's abort word, which ends the others'
// waits (an atomic read per sweep); the workgroup tests the word behind its next barrier and leaves its step loop together.
constexpr unsigned SEQ_GATHER_BOUND = 2000000u, REFINE_GATHER_BOUND = 4000000u, TRIDIAG_GATHER_BOUND = 2000000u;   // (the sequence GRU keeps its own sweep: gru.hip)
template <int N, int K, class At>
__device__ __forceinline__ bool cluster_gather(granule (&q)[N][K], int count, unsigned epoch, unsigned bound, int* abort, At at) {
  for (unsigned sweeps = 0;; ++sweeps) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < count) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
          q[i][c] = __hip_atomic_load(at(i, c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = ok && granule_has(q[i][c], epoch);
        }
      }
    if (ok) return true;
    if (sweeps > bound || __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
      __hip_atomic_store(abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

struct ClusterArgs {   // what every cluster kernel's argument struct begins with; cluster_launch fills it
  granule* gx;        // the granule buffer (ClusterLayout), zeroed before every launch
  int* abort_flag;     // the context's fault word: after a time-out ONE thread per workgroup (per wave in the sequence GRU) ORs the kernel's DMP_FAULT_*_HANDOFF bit
  int allow_local;     // 0: never the XCD-local publication
};
// G workgroups of one XCD in a grid of 8 G (block id % 8 picks the XCD, the others leave at once); not beside a persistent vertical-GRU launch (CoResident)
template <class Args>
int cluster_launch(dmp_ctx* c, hipStream_t s, void (*kernel)(Args), int G, int threads, size_t lds, unsigned long long* gx, ClusterLayout lay, Args a) {
  a.gx = gx; a.abort_flag = c->seq_abort; a.allow_local = c->cluster_local;
  CoResident guard(c, s, false);
  if (guard.status()) return guard.status();
  DMP_HIP(hipMemsetAsync(gx, 0, sizeof(granule) * lay.words(), s));
  hipLaunchKernelGGL(kernel, dim3(8 * G), dim3(threads), lds, s, a);
  DMP_LAUNCH_CHECK();
  return guard.done();
}

}  // namespace dmp
