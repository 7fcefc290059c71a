// The native entity that options "assign_ss", "exposure" and "domains" share: what each of them needs of the score block's native
// trace and of the alignment's first row, prepared once per prediction whichever of the three are on.
//   entity_row    front end, beside msa_weights: the residue codes of the alignment's first row, kept for the prediction's end
//                 (the donor flag of "assign_ss" is code != P, the side-chain flag of "exposure" code != G)
//   entity_whole  dmp_predict_end, in front of assign_ss, one workgroup: whole_x = every row of the native trace has an x that
//                 is no NaN (the predicate of "assign_ss" and "exposure"), whole_xyz = no coordinate of it is NaN (the predicate
//                 of "domains"); include/dmpfold_hip.h states each beside its option
// and, for "assign_ss" and "exposure", the native's backbone from its trace by the model's own device function (coords.hip).
#include "score_common.h"

namespace dmp {

// The scratch of a context of capacity `cap` (bytes from its start, every part 16-aligned): the head = whole_x, whole_xyz | the
// first row's codes [cap] | the native's backbone [cap][5][3].  Nothing in it has to be zero between launches.
struct EntityScratch { int64_t row, bb, total; };
constexpr int64_t ENTITY_HEAD_BYTES = 16;
inline EntityScratch entity_scratch(int cap) {
  auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  EntityScratch s;
  s.row = ENTITY_HEAD_BYTES;
  s.bb = s.row + up(cap);
  s.total = s.bb + up(60 * (int64_t)cap);
  return s;
}
ScratchNeed entity_need(int max_L) { return {entity_scratch(max_L).total, ENTITY_HEAD_BYTES}; }

NativeEntity native_entity(const dmp_ctx* c) {
  const EntityScratch sc = entity_scratch(c->max_L);
  unsigned char* ws = c->entity_ws.p;
  return {(int*)ws, (int*)ws + 1, ws + sc.row, (float*)(ws + sc.bb)};
}

__global__ void entity_row_kernel(const uint8_t* __restrict__ msa, int L, unsigned char* __restrict__ row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) row[i] = msa[i];
}

__global__ __launch_bounds__(256) void entity_whole_kernel(const float* __restrict__ native, int L, int* whole_x, int* whole_xyz) {
  __shared__ int missing;                // bit 0: a NaN x, bit 1: a NaN coordinate
  const int tid = threadIdx.x;
  if (tid == 0) missing = 0;
  __syncthreads();
  int mine = 0;
  for (int k = tid; k < L; k += 256) {
    const float x = native[3 * k], y = native[3 * k + 1], z = native[3 * k + 2];
    mine |= (x == x ? 0 : 1) | (x == x && y == y && z == z ? 0 : 2);
  }
  if (mine) atomicOr(&missing, mine);
  __syncthreads();
  if (tid == 0) {
    *whole_x = missing & 1 ? 0 : 1;
    *whole_xyz = missing & 2 ? 0 : 1;
  }
}

int entity_capture_row(dmp_ctx* c, const uint8_t* d_msa, int L, hipStream_t s) {
  hipLaunchKernelGGL(entity_row_kernel, dim3(cdiv(L, 256)), dim3(256), 0, s, d_msa, L, native_entity(c).row);
  DMP_LAUNCH_CHECK();
  return DMP_OK;
}

int entity_prepare(dmp_ctx* c, const float* d_native, int L, bool backbone, hipStream_t s) {
  const NativeEntity en = native_entity(c);
  hipLaunchKernelGGL(entity_whole_kernel, dim3(1), dim3(256), 0, s, d_native, L, en.whole_x, en.whole_xyz);
  DMP_LAUNCH_CHECK();
  return backbone ? trace_to_backbone(d_native, L, en.bb, s) : DMP_OK;
}

}  // namespace dmp
