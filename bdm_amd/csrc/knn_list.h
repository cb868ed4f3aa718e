// The sorted neighbour list of a wave, one entry per lane, and the step that offers it one candidate per lane: the rule that
// estimate_normals_kernel (normals.hip, bdm_hip.h section 10) and knn_points_kernel (knn.hip, section 15) share, stated once.
//
// Lane l of the wave holds the l-th nearest candidate so far as (key, index); key is the bit pattern of the squared distance
// (d2 >= +0, so the pattern orders like the value), KNN_EMPTY for an unused entry: above +inf (a finite pair whose distance
// overflowed is still a neighbour), below or equal to every NaN pattern (a NaN distance is never accepted).  thr is the key of
// lane k - 1, the same in every lane.  Candidates must arrive in ascending index; the accepted lanes of a step are inserted in
// ascending lane order, so "strictly below the k-th key" and "behind every equal key" order the list by (d2, index) without an
// index taking part in a comparison.
#pragma once
#include <hip/hip_runtime.h>

namespace bdm {

constexpr unsigned int KNN_EMPTY = 0x7f800001u;

// lane l <- lane l - 1 (lane 0 <- 0): DPP wave_shr:1
__device__ __forceinline__ unsigned int lane_shr1(unsigned int v) {
  return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, false);
}

// the key of candidate c against query q: the unfused squared distance of sections 10 and 15
__device__ __forceinline__ unsigned int knn_key(float cx, float cy, float cz, float qx, float qy, float qz) {
  const float dx = cx - qx, dy = cy - qy, dz = cz - qz;
  return __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

// One step: lane l offers the candidate of index first + l with this key.  Every lane of the wave must call it (ballot, readlane).
__device__ __forceinline__ void knn_list_step(unsigned int key, int first, int k, int lane, unsigned int &lkey, int &lidx,
                                              unsigned int &thr) {
  unsigned long long hits = __ballot(key < thr);
  while (hits) {  // wave-uniform
    const int src = __builtin_ctzll(hits);
    hits &= hits - 1;
    const unsigned int kc = (unsigned int)__builtin_amdgcn_readlane((int)key, src);
    if (kc < thr) {  // an earlier insertion of this step may have lowered the k-th key
      const unsigned int pk = lane_shr1(lkey);
      const int pj = (int)lane_shr1((unsigned int)lidx);
      const bool behind = lkey > kc && lane < k, shift = pk > kc;  // lane 0 reads key 0: never a shift
      lidx = behind ? (shift ? pj : first + src) : lidx;
      lkey = behind ? (shift ? pk : kc) : lkey;
      thr = (unsigned int)__builtin_amdgcn_readlane((int)lkey, k - 1);
    }
  }
}

}  // namespace bdm
