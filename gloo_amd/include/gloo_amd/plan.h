// plan.h — per-rank schedules (see include/gloo_amd.h "Schedules").
#pragma once

#include <cstdint>
#include <vector>

#include "gloo_amd.h"

namespace gloo_amd {

using Step = gloo_hip_step_t;

struct Plan {
  std::vector<Step> steps;
  uint64_t arena = 0;  // inbox arena, elements
};

// Build rank `rank`'s plan.  recvElems: reduce-scatter only.
Plan makePlan(int algo, int rank, int size, uint64_t count, int nptrs,
              const std::vector<int>& recvElems = {});

// New-style collective parameters (gloo/allreduce.h:89-193, gloo/reduce.h:19-110).
struct NewStyleOptions {
  int ninputs = 0;
  int noutputs = 1;
  size_t elemSize = 4;
  size_t maxSegmentBytes = 1024 * 1024;  // kMaxSegmentSize, gloo/allreduce.h:78, gloo/reduce.h:98
  int root = 0;                          // gloo::reduce only (ReduceOptions::setRoot)
};
// algo: GLOO_HIP_ALGO_ALLREDUCE_RING, GLOO_HIP_ALGO_ALLREDUCE_BCUBE or
// GLOO_HIP_ALGO_REDUCE, optionally | GLOO_HIP_ALGO_MESH (mesh.h).
Plan makeNewStylePlan(int algo, int rank, int size, uint64_t count, const NewStyleOptions& o);
// GLOO_HIP_ALGO_ALLGATHER (plan.cc planAllgather): `ninputs` inputs per rank
// (0: in place, one block per rank already in its slot of the output) of
// `count` elements each, or of counts[r] on rank r when `counts` has `size`
// entries.  algo | GLOO_HIP_ALGO_MESH and a negative count are refused.
Plan makeAllgatherPlan(int algo, int rank, int size, uint64_t count, int ninputs, const std::vector<int>& counts);
inline bool isAllgather(int algo) { return (algo & ~GLOO_HIP_ALGO_MESH) == GLOO_HIP_ALGO_ALLGATHER; }
// GLOO_HIP_ALGO_ALLTOALL (plan.cc planAlltoall): one input and one output per
// rank.  `counts` empty: the even form, `count` elements per block; else
// 2 * size entries, this rank's in_counts[0..size) then out_counts[0..size).
// algo | GLOO_HIP_ALGO_MESH, ninputs != 1, a negative count and in_counts[rank]
// != out_counts[rank] are refused.
Plan makeAlltoallPlan(int algo, int rank, int size, uint64_t count, int ninputs, const std::vector<int>& counts);
inline bool isAlltoall(int algo) { return (algo & ~GLOO_HIP_ALGO_MESH) == GLOO_HIP_ALGO_ALLTOALL; }
// The executor's description of an alltoall is the same on every rank: no
// list (the even form), or the size x size matrix M with M[q * size + r] the
// elements rank q sends to rank r.  Rank r's lists for makeAlltoallPlan are
// row r (its in_counts) then column r (its out_counts), so in_counts_q[r] ==
// out_counts_r[q] holds for every pair by construction and every rank derives
// every peer's plan.  An empty matrix gives an empty list; any other length
// than size * size is refused.
std::vector<int> alltoallLists(int rank, int size, const std::vector<int>& matrix);
// GLOO_HIP_ALGO_GATHER (plan.cc planGather): one input per rank, one output
// on the root.  recvElems = {root}: every block `count` elements; {root, c_0
// ... c_{size-1}}: gatherv, `count` ignored.  Any other length, a root outside
// [0, size), a negative count and algo | GLOO_HIP_ALGO_MESH are refused.  The
// plan depends on nothing else, so every rank derives every peer's.
Plan makeGatherPlan(int algo, int rank, int size, uint64_t count, const std::vector<int>& recvElems);
inline bool isGather(int algo) { return (algo & ~GLOO_HIP_ALGO_MESH) == GLOO_HIP_ALGO_GATHER; }
// GLOO_HIP_ALGO_SCATTER (plan.cc planScatter): `size` inputs of `count`
// elements on the root, one output per rank.  recvElems = {root}; any other
// length, a root outside [0, size) and algo | GLOO_HIP_ALGO_MESH are refused.
Plan makeScatterPlan(int algo, int rank, int size, uint64_t count, const std::vector<int>& recvElems);
inline bool isScatter(int algo) { return (algo & ~GLOO_HIP_ALGO_MESH) == GLOO_HIP_ALGO_SCATTER; }
inline bool isRooted(int algo) { return isGather(algo) || isScatter(algo); }
// Receives the text of a planner's refusal (an unknown algorithm, a mesh form
// that does not exist, bad sizes) when gloo_hip_plan / gloo_hip_plan_ex return
// GLOO_HIP_EINVAL_ARG.  The library installs its last-error text here
// (errors.cc); a host-only build of the planners alone leaves it null.
extern void (*planErrorSink)(int code, const char* msg);

inline bool isNewStyle(int algo) {
  algo &= ~GLOO_HIP_ALGO_MESH;
  return algo == GLOO_HIP_ALGO_ALLREDUCE_RING || algo == GLOO_HIP_ALGO_ALLREDUCE_BCUBE ||
         algo == GLOO_HIP_ALGO_REDUCE;
}

}  // namespace gloo_amd
