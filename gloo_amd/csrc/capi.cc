// capi.cc — C-ABI over Context / PlanExecutor; no exception crosses it.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "gloo_amd.h"
#include "gloo_amd/common.h"
#include "gloo_amd/context.h"
#include "gloo_amd/errors.h"
#include "gloo_amd/executor.h"
#include "gloo_amd/ipc.h"
#include "gloo_amd/signal.h"
#include "gloo_amd/transport.h"

struct gloo_hip_context {
  std::shared_ptr<gloo_amd::Context> ctx;
  // function-style allreduce: one executor per option set, least recently
  // used first (every rank makes the same calls, so hits and evictions agree)
  std::list<std::pair<std::string, std::unique_ptr<gloo_amd::PlanExecutor>>> cache;
  gloo_amd::PlanExecutor* last = nullptr;  // the executor of the latest function-style call
};
struct gloo_hip_algorithm {
  std::unique_ptr<gloo_amd::PlanExecutor> exec;
};
struct gloo_hip_transport {
  std::unique_ptr<gloo_amd::transport::Device> dev;
};
struct gloo_hip_buffer {
  std::unique_ptr<gloo_amd::transport::Buffer> buf;
};
struct gloo_hip_ubuf {
  std::unique_ptr<gloo_amd::transport::UnboundBuffer> buf;
};

namespace {
template <typename F>
int guarded(F&& f) {
  try {
    f();
    return GLOO_HIP_OK;
  } catch (const gloo_amd::IoException& e) {
    return gloo_amd::setError(GLOO_HIP_EIO, std::string("IoException: ") + e.what());
  } catch (const std::exception& e) {
    return gloo_amd::setError(GLOO_HIP_EINVAL_ARG, e.what());
  } catch (...) {
    return gloo_amd::setError(GLOO_HIP_EINVAL_ARG, "unknown exception");
  }
}

// Function-style collectives: one executor per option set (the plan depends
// on sizes, not pointers; every rank makes the same calls, so hits and
// evictions agree), rebound to the call's buffers and run.
void runCached(gloo_hip_context_t ctx, int algo, int op, int dtype, const std::vector<void*>& ins,
               const std::vector<void*>& outs, size_t elements, size_t maxSeg, uint32_t tag,
               gloo_hip_stream_t stream, const std::vector<int>& extra) {
  // The key holds what the schedule depends on, never a rank-local value
  // such as the stream: ranks that pass different streams for the same call
  // must still hit and evict alike (their construction and tear-down are
  // collective).  The stream is rebound per call, like the buffers.
  std::string key = gloo_amd::strcat_(algo, "/", op, "/", dtype, "/", ins.size(), "/", outs.size(), "/", elements,
                                      "/", maxSeg, "/", tag);
  for (int v : extra) key += gloo_amd::strcat_("/", v);
  auto& cache = ctx->cache;
  auto it = cache.begin();
  for (; it != cache.end(); ++it)
    if (it->first == key) break;
  if (it == cache.end()) {
    constexpr size_t kMaxCached = 16;
    if (cache.size() == kMaxCached) cache.pop_back();
    cache.emplace_front(key, gloo_amd::PlanExecutor::create(ctx->ctx, algo, op, dtype, outs, elements,
                                                                      extra, static_cast<hipStream_t>(stream), ins,
                                                                      maxSeg));
    it = cache.begin();
  } else if (it != cache.begin()) {
    cache.splice(cache.begin(), cache, it);
    it = cache.begin();
  }
  it->second->setStream(static_cast<hipStream_t>(stream));
  it->second->setBuffers(ins, outs);
  ctx->last = it->second.get();
  it->second->run();
}

bool isBroadcast(int algo) { return (algo & ~GLOO_HIP_ALGO_MESH) == GLOO_HIP_ALGO_BROADCAST; }

// GLOO_HIP_ALGO_BROADCAST at the algorithm entry points.  Refused here,
// before any exchange with a peer (every rank makes the same call and fails
// alike): | GLOO_HIP_ALGO_MESH, a root outside [0, size), a root pointer
// outside [0, nptrs).  The executor then gets {root} and the pointer list
// with the root pointer first (order[i] = the caller's index of executor
// pointer i), so LOCAL_BCAST's ptrs[i] = ptrs[0] is the reference's local
// broadcast from devicePtrs_[rootPointerRank].  `op` is not used by a
// broadcast; the executor's copy kernels get SUM, which every dtype has.
void broadcastArgs(int algo, int size, const int* recv_elems, int nptrs, std::vector<int>* re,
                   std::vector<int>* order, int* op) {
  GLOO_AMD_ENFORCE(!(algo & GLOO_HIP_ALGO_MESH), "broadcast has no mesh form: algorithm ", algo,
                   " (GLOO_HIP_ALGO_BROADCAST | GLOO_HIP_ALGO_MESH) is refused");
  const int root = recv_elems ? recv_elems[0] : 0, rootPointer = recv_elems ? recv_elems[1] : 0;
  GLOO_AMD_ENFORCE(root >= 0 && root < size, "broadcast: root rank ", root, " outside [0, ", size, ")");
  GLOO_AMD_ENFORCE(rootPointer >= 0 && rootPointer < nptrs, "broadcast: root pointer ", rootPointer,
                   " outside [0, ", nptrs, ")");
  re->assign(1, root);
  order->assign(1, rootPointer);
  for (int i = 0; i < nptrs; i++)
    if (i != rootPointer) order->push_back(i);
  *op = GLOO_HIP_SUM;
}

// GLOO_HIP_ALGO_ALLGATHER at the algorithm entry points: ptrs = {out, in_0 ...
// in_{k-1}} (nptrs = 1: in place), `count` elements per input on every rank,
// recv_elems NULL.  | GLOO_HIP_ALGO_MESH is refused here, before any exchange
// with a peer.  `op` is not used; the executor gets SUM, which every dtype has.
void allgatherArgs(int algo, void* const* ptrs, int nptrs, const int* recv_elems, std::vector<void*>* outs,
                   std::vector<void*>* ins, int* op) {
  GLOO_AMD_ENFORCE(!(algo & GLOO_HIP_ALGO_MESH), "allgather has no mesh form: algorithm ", algo,
                   " (GLOO_HIP_ALGO_ALLGATHER | GLOO_HIP_ALGO_MESH) is refused");
  GLOO_AMD_ENFORCE(!recv_elems, "allgather: recv_elems must be NULL (per-rank counts: gloo_hip_allgather)");
  outs->assign(1, ptrs[0]);
  ins->assign(ptrs + 1, ptrs + nptrs);
  *op = GLOO_HIP_SUM;
}

// GLOO_HIP_ALGO_GATHER / GLOO_HIP_ALGO_SCATTER at the algorithm entry points
// (include/gloo_amd.h).  Gather: ptrs = {in[, out]}, recv_elems = {root}, or
// {root, c_0 ... c_{size-1}} with count == GLOO_HIP_COUNT_PER_RANK.  Scatter:
// ptrs = {out[, in_0 ... in_{size-1}]}, recv_elems = {root}.  Every refusal is
// made here, before any exchange with a peer: the planner's (the rank's own
// plan is built once for them) and the pointer counts.  A gather rank
// without an output hands the executor its input as "output 0": no step of
// its plan reads or writes output 0, and the executor wants one pointer.
// `op` is not used; the executor gets SUM, which every dtype has.
void rootedArgs(int algo, int rank, int size, void* const* ptrs, int nptrs, size_t* count, const int* recv_elems,
                std::vector<int>* re, std::vector<void*>* outs, std::vector<void*>* ins, int* op) {
  const bool gather = gloo_amd::isGather(algo);
  const char* name = gather ? "gather" : "scatter";
  GLOO_AMD_ENFORCE(recv_elems, name, ": recv_elems is NULL ({root} expected)");
  const bool perRank = gather && *count == GLOO_HIP_COUNT_PER_RANK;
  re->assign(recv_elems, recv_elems + (perRank ? 1 + size : 1));
  if (perRank) *count = 0;
  try {
    (void)(gather ? gloo_amd::makeGatherPlan(algo, rank, size, *count, *re)
                  : gloo_amd::makeScatterPlan(algo, rank, size, *count, *re));
  } catch (const std::invalid_argument& e) {
    GLOO_AMD_ENFORCE(false, e.what());
  }
  const bool root = (*re)[0] == rank;
  if (gather) {
    GLOO_AMD_ENFORCE(!root || nptrs == 2, "gather: the root passes {input, output}, not ", nptrs, " pointers");
    GLOO_AMD_ENFORCE(nptrs == 1 || nptrs == 2, "gather: {input} or {input, output}, not ", nptrs, " pointers");
    ins->assign(1, ptrs[0]);
    outs->assign(1, root ? ptrs[1] : ptrs[0]);
  } else {
    GLOO_AMD_ENFORCE(!root || nptrs == 1 + size, "scatter: the root passes {output, ", size, " inputs}, not ", nptrs,
                     " pointers");
    outs->assign(1, ptrs[0]);
    ins->clear();
    if (root) ins->assign(ptrs + 1, ptrs + nptrs);
  }
  *op = GLOO_HIP_SUM;
}

// GLOO_HIP_ALGO_ALLTOALL at the generic algorithm entry points: refused, as
// before there was an executor for it.  An alltoall's pointers ({input,
// output}, neither of them a list) and its P x P count matrix do not fit that
// signature; gloo_hip_alltoall_create is its algorithm-object form.
void refuseAlltoall(int algo) {
  GLOO_AMD_ENFORCE(!gloo_amd::isAlltoall(algo), "unknown algorithm ", algo,
                   " at this entry point (an alltoall's {input, output} and count matrix do not fit its signature: "
                   "gloo_hip_alltoall_create)");
}

// What both alltoall entries check on this rank before any exchange with a
// peer, given the rank's lists (`lists` empty: the even form of `count`
// elements per block; else in_counts then out_counts, 2 * size ints): the
// planner's own refusals (the rank's plan is built once for them), a NULL
// buffer where there are elements to move, and an input that shares a byte
// with the output (there is no in-place form: the sends read the input while
// the own block and the copy-outs store the output).
void alltoallBuffers(int rank, int size, int dtype, size_t count, const std::vector<int>& lists, const void* input,
                     const void* output) {
  const size_t es = gloo_hip_dtype_size(dtype);
  try {
    (void)gloo_amd::makeAlltoallPlan(GLOO_HIP_ALGO_ALLTOALL, rank, size, count, 1, lists);
  } catch (const std::invalid_argument& e) {
    GLOO_AMD_ENFORCE(false, e.what());
  }
  size_t in = 0, out = 0;  // elements this rank sends (its own block included) and receives
  for (int q = 0; q < size; q++) {
    in += lists.empty() ? count : (size_t)lists[q];
    out += lists.empty() ? count : (size_t)lists[size + q];
  }
  GLOO_AMD_ENFORCE(input || in == 0, "alltoall: null input with ", in, " elements to send");         // alltoallv.cc:118
  GLOO_AMD_ENFORCE(output || out == 0, "alltoall: null output with ", out, " elements to receive");  // alltoallv.cc:119
  const char* a = static_cast<const char*>(input);
  const char* b = static_cast<const char*>(output);
  GLOO_AMD_ENFORCE(in == 0 || out == 0 || a + in * es <= b || b + out * es <= a, "alltoall: input [", input, ", +",
                   in * es, ") and output [", output, ", +", out * es, ") overlap (there is no in-place form)");
}

bool allZero(const std::vector<int>& v) {
  for (int x : v)
    if (x != 0) return false;
  return true;
}
}  // namespace

extern "C" {

int gloo_hip_context_create(int rank, int size, const char* store_url, int device, int timeout_ms,
                            gloo_hip_context_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(out && store_url, "null argument");
    auto c = std::make_unique<gloo_hip_context>();
    c->ctx = std::make_shared<gloo_amd::Context>(
        rank, size, std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 30000));
    c->ctx->connect(gloo_amd::openStore(store_url), device);
    *out = c.release();
  });
}

int gloo_hip_context_create_ex(int rank, int size, int device, int timeout_ms, gloo_hip_allgather_fn allgather,
                               void* user, gloo_hip_context_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(out && allgather, "null argument");
    auto c = std::make_unique<gloo_hip_context>();
    c->ctx = std::make_shared<gloo_amd::Context>(
        rank, size, std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 30000));
    c->ctx->connect(std::make_shared<gloo_amd::CallbackStore>(allgather, user), device);
    *out = c.release();
  });
}

int gloo_hip_context_destroy(gloo_hip_context_t ctx) {
  return guarded([&] {
    if (ctx) ctx->cache.clear();  // executors tear down before the context
    delete ctx;
  });
}

int gloo_hip_algorithm_create_ws(gloo_hip_context_t ctx, int algo, int op, int dtype, void* const* ptrs, int nptrs,
                                 size_t count, const int* recv_elems, gloo_hip_stream_t stream, int workspace,
                                 gloo_hip_algorithm_t* out) {
  // refused on this rank before any exchange: every rank makes the same call
  // and fails alike, so nobody waits for a peer
  // a broadcast / an allgather / a gather / a scatter does not use its op
  if (!isBroadcast(algo) && !gloo_amd::isAllgather(algo) && !gloo_amd::isRooted(algo))
    if (const int rc = gloo_amd::checkBitwiseDtype(op, dtype)) return rc;
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && out && ptrs && nptrs >= 1, "bad arguments");
    refuseAlltoall(algo);
    std::vector<int> re;
    if (algo == GLOO_HIP_ALGO_REDUCE_SCATTER) {
      GLOO_AMD_ENFORCE(recv_elems, "reduce-scatter needs recv_elems");
      re.assign(recv_elems, recv_elems + ctx->ctx->size);
    }
    if (algo == GLOO_HIP_ALGO_BCUBE && recv_elems) re.assign(recv_elems, recv_elems + 1);  // {base}
    std::vector<void*> ps(ptrs, ptrs + nptrs);
    if (isBroadcast(algo)) {
      std::vector<int> order;
      broadcastArgs(algo, ctx->ctx->size, recv_elems, nptrs, &re, &order, &op);
      for (int i = 0; i < nptrs; i++) ps[i] = ptrs[order[i]];
    }
    std::vector<void*> ins;
    if (gloo_amd::isAllgather(algo)) allgatherArgs(algo, ptrs, nptrs, recv_elems, &ps, &ins, &op);
    if (gloo_amd::isRooted(algo))
      rootedArgs(algo, ctx->ctx->rank, ctx->ctx->size, ptrs, nptrs, &count, recv_elems, &re, &ps, &ins, &op);
    auto a = std::make_unique<gloo_hip_algorithm>();
    a->exec = gloo_amd::PlanExecutor::create(ctx->ctx, algo, op, dtype, ps, count, re,
                                                       static_cast<hipStream_t>(stream), ins, 0, workspace);
    *out = a.release();
  });
}

int gloo_hip_algorithm_create_streams(gloo_hip_context_t ctx, int algo, int op, int dtype, void* const* ptrs,
                                      int nptrs, size_t count, const int* recv_elems,
                                      const gloo_hip_stream_t* streams, int nstreams, int workspace,
                                      gloo_hip_algorithm_t* out) {
  if (!isBroadcast(algo) && !gloo_amd::isAllgather(algo) && !gloo_amd::isRooted(algo))
    if (const int rc = gloo_amd::checkBitwiseDtype(op, dtype)) return rc;  // before any exchange, as create_ws
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && out && ptrs && nptrs >= 1, "bad arguments");
    refuseAlltoall(algo);
    // gloo/cuda_allreduce_ring_chunked.cc:55-58
    // a gather / a scatter: a rank's pointer count differs between the root and
    // the others, and so would the stream lists; every rank passes one stream
    // (the plan's) or none, whatever its pointer count
    if (gloo_amd::isRooted(algo))
      GLOO_AMD_ENFORCE(nstreams == 0 || (streams && nstreams == 1), "a gather / a scatter takes one stream or none, not ",
                       nstreams);
    else
      GLOO_AMD_ENFORCE(nstreams == 0 || (streams && nstreams == nptrs), "streams: ", nstreams, ", pointers: ", nptrs,
                       " (one stream per pointer, or none)");
    std::vector<int> re;
    if (algo == GLOO_HIP_ALGO_REDUCE_SCATTER) {
      GLOO_AMD_ENFORCE(recv_elems, "reduce-scatter needs recv_elems");
      re.assign(recv_elems, recv_elems + ctx->ctx->size);
    }
    if (algo == GLOO_HIP_ALGO_BCUBE && recv_elems) re.assign(recv_elems, recv_elems + 1);  // {base}
    std::vector<void*> ps(ptrs, ptrs + nptrs);
    std::vector<hipStream_t> ss;
    for (int i = 0; i < nstreams; i++) ss.push_back(static_cast<hipStream_t>(streams[i]));
    if (isBroadcast(algo)) {  // stream i stays with pointer i
      std::vector<int> order;
      broadcastArgs(algo, ctx->ctx->size, recv_elems, nptrs, &re, &order, &op);
      for (int i = 0; i < nptrs; i++) ps[i] = ptrs[order[i]];
      for (int i = 0; i < nstreams; i++) ss[i] = static_cast<hipStream_t>(streams[order[i]]);
    }
    // Validated before the collective construction: a refusal after it would
    // run the executor's release() on this rank alone, and the peers would
    // wait at its barrier until the context timeout.
    for (hipStream_t t : ss)
      GLOO_AMD_ENFORCE(t != nullptr || ss.size() == 1, "null stream in a list of ", ss.size(),
                       " (one stream per pointer)");
    std::vector<void*> ins;  // an allgather: stream i stays with pointer i of {out, in_0 ...}
    if (gloo_amd::isAllgather(algo)) allgatherArgs(algo, ptrs, nptrs, recv_elems, &ps, &ins, &op);
    if (gloo_amd::isRooted(algo))
      rootedArgs(algo, ctx->ctx->rank, ctx->ctx->size, ptrs, nptrs, &count, recv_elems, &re, &ps, &ins, &op);
    auto a = std::make_unique<gloo_hip_algorithm>();
    a->exec = gloo_amd::PlanExecutor::create(ctx->ctx, algo, op, dtype, ps, count, re,
                                             ss.empty() ? nullptr : ss[0], ins, 0, workspace);
    if (ss.size() > 1) a->exec->setStreams(ss);
    *out = a.release();
  });
}

int gloo_hip_algorithm_set_streams(gloo_hip_algorithm_t a, const gloo_hip_stream_t* streams, int nstreams) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(a && (nstreams == 0 || streams), "bad arguments");
    std::vector<hipStream_t> ss;
    for (int i = 0; i < nstreams; i++) ss.push_back(static_cast<hipStream_t>(streams[i]));
    a->exec->setStreams(ss);
  });
}

int gloo_hip_algorithm_create(gloo_hip_context_t ctx, int algo, int op, int dtype, void* const* ptrs, int nptrs,
                              size_t count, const int* recv_elems, gloo_hip_stream_t stream,
                              gloo_hip_algorithm_t* out) {
  return gloo_hip_algorithm_create_ws(ctx, algo, op, dtype, ptrs, nptrs, count, recv_elems, stream,
                                      GLOO_HIP_WORKSPACE_DEVICE, out);
}

namespace {
int interpBatches(const gloo_hip_interp_desc_t* steps, const gloo_hip_interp_desc_ex_t* ex, int n, int* defer_out) {
  if (n < 0 || (n > 0 && ((!steps && !ex) || !defer_out)))
    return gloo_amd::setError(GLOO_HIP_EINVAL_ARG, "gloo_hip_interp_batches: bad arguments");
  return guarded([&] {
    std::vector<gloo_amd::InterpStep> v((size_t)n);
    for (int i = 0; i < n; i++) {
      const gloo_hip_interp_desc_t& d = ex ? ex[i].step : steps[i];
      GLOO_AMD_ENFORCE(d.kind >= gloo_amd::kInterpCopy && d.kind <= gloo_amd::kInterpFold && d.nsrc >= 0 &&
                           d.nsrc <= GLOO_HIP_MAX_SRCS,
                       "gloo_hip_interp_batches: bad step ", i);
      gloo_amd::InterpStep& t = v[(size_t)i];
      std::memset(&t, 0, sizeof t);
      t.kind = d.kind;
      t.nsrc = d.kind == gloo_amd::kInterpFold ? d.nsrc : 1;
      t.dst = reinterpret_cast<char*>(d.dst);
      for (int j = 0; j < GLOO_HIP_MAX_SRCS; j++) t.src[j] = reinterpret_cast<const char*>(d.src[j]);
      t.n = d.bytes;
      if (ex) {
        const bool data = d.kind == gloo_amd::kInterpCopy;
        GLOO_AMD_ENFORCE(ex[i].nxdst >= 0 && ex[i].nxdst <= (data ? gloo_amd::kMaxCopyEntries : 0),
                         "gloo_hip_interp_batches_ex: bad destination count of step ", i);
        t.nxdst = ex[i].nxdst;
        for (int j = 0; j < t.nxdst; j++) t.xdst[j] = reinterpret_cast<char*>(ex[i].xdst[j]);
      }
    }
    gloo_amd::markInterpBatches(v.data(), v.size(), 1);
    for (int i = 0; i < n; i++) defer_out[i] = v[(size_t)i].flags & gloo_amd::kInterpDefer ? 1 : 0;
  });
}
}  // namespace

int gloo_hip_interp_batches(const gloo_hip_interp_desc_t* steps, int n, int* defer_out) {
  return interpBatches(steps, nullptr, n, defer_out);
}

int gloo_hip_interp_batches_ex(const gloo_hip_interp_desc_ex_t* steps, int n, int* defer_out) {
  return interpBatches(nullptr, steps, n, defer_out);
}

int gloo_hip_ipc_stats(uint64_t* out) {
  return gloo_hip_ipc_stats_ex(out, 5);
}

int gloo_hip_ipc_stats_ex(uint64_t* out, size_t n) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(out, "null argument");
    const gloo_amd::ipc::Stats st = gloo_amd::ipc::stats();
    const uint64_t v[] = {st.slabs, st.slabBytes, st.free, st.imports, st.opens, st.dropped};
    for (size_t i = 0; i < n && i < sizeof(v) / sizeof(v[0]); i++) out[i] = v[i];
  });
}

int gloo_hip_algorithm_run(gloo_hip_algorithm_t a) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(a, "null algorithm");
    a->exec->run();
  });
}

int gloo_hip_algorithm_destroy(gloo_hip_algorithm_t a) {
  return guarded([&] { delete a; });
}

int gloo_hip_allreduce(gloo_hip_context_t ctx, const gloo_hip_allreduce_options_t* o) {
  if (o)  // before the elements == 0 shortcut and any exchange, as create_ws
    if (const int rc = gloo_amd::checkBitwiseDtype(o->op, o->dtype)) return rc;
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    GLOO_AMD_ENFORCE(o->algorithm == 0 || o->algorithm == GLOO_HIP_ALLREDUCE_RING ||
                         o->algorithm == GLOO_HIP_ALLREDUCE_BCUBE,
                     "Algorithm not handled.");  // gloo/allreduce.cc:142-143
    GLOO_AMD_ENFORCE(o->noutputs >= 1 && o->outputs, "need at least one output");
    GLOO_AMD_ENFORCE(o->ninputs == 0 || o->inputs, "null inputs");
    if (o->elements == 0) return;  // gloo/allreduce.cc:98-100
    std::vector<void*> ins(o->inputs, o->inputs + o->ninputs), outs(o->outputs, o->outputs + o->noutputs);
    const int algo = o->algorithm == GLOO_HIP_ALLREDUCE_BCUBE ? GLOO_HIP_ALGO_ALLREDUCE_BCUBE
                                                              : GLOO_HIP_ALGO_ALLREDUCE_RING;
    runCached(ctx, algo, o->op, o->dtype, ins, outs, o->elements, o->max_segment_bytes, o->tag, o->stream, {});
  });
}

int gloo_hip_reduce_to_root(gloo_hip_context_t ctx, const gloo_hip_reduce_options_t* o) {
  if (o)
    if (const int rc = gloo_amd::checkBitwiseDtype(o->op, o->dtype)) return rc;
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    if (o->elements == 0) return;  // gloo/reduce.cc:22-24
    GLOO_AMD_ENFORCE(o->output, "null output");
    GLOO_AMD_ENFORCE(o->root >= 0 && o->root < ctx->ctx->size, "root ", o->root, " out of range");  // :32
    std::vector<void*> ins, outs{o->output};
    if (o->input && o->input != o->output) ins.push_back(o->input);  // :46-48
    runCached(ctx, GLOO_HIP_ALGO_REDUCE, o->op, o->dtype, ins, outs, o->elements, o->max_segment_bytes, o->tag,
              o->stream, {o->root});
  });
}

int gloo_hip_broadcast(gloo_hip_context_t ctx, const gloo_hip_broadcast_options_t* o) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    GLOO_AMD_ENFORCE(gloo_hip_dtype_size(o->dtype) > 0, "unknown dtype ", o->dtype);
    GLOO_AMD_ENFORCE(o->root >= 0 && o->root < ctx->ctx->size, "broadcast: root rank ", o->root, " outside [0, ",
                     ctx->ctx->size, ")");  // gloo/broadcast.cc:28
    if (o->elements == 0) return;
    GLOO_AMD_ENFORCE(o->output, "null output");
    // A root with a separate input: its output takes the input's bytes on the
    // call's stream first (the schedule depends on sizes only, and only the
    // root knows of its input, so the cached executor is the same on every
    // rank: one pointer, the output).
    const bool separate = ctx->ctx->rank == o->root && o->input && o->input != o->output;
    if (separate) {
      hipStream_t s = static_cast<hipStream_t>(o->stream);
      GLOO_AMD_HIP_CHECK(hipSetDevice(ctx->ctx->device()));
      GLOO_AMD_HIP_CHECK(hipMemcpyAsync(o->output, o->input, o->elements * gloo_hip_dtype_size(o->dtype),
                                        hipMemcpyDeviceToDevice, s));
      // no stream given: the executor's own stream does not wait for the null stream
      if (!s) GLOO_AMD_HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    runCached(ctx, GLOO_HIP_ALGO_BROADCAST, GLOO_HIP_SUM, o->dtype, {}, {o->output}, o->elements, 0, o->tag,
              o->stream, {o->root});
  });
}

int gloo_hip_allgather(gloo_hip_context_t ctx, const gloo_hip_allgather_options_t* o) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    GLOO_AMD_ENFORCE(gloo_hip_dtype_size(o->dtype) > 0, "unknown dtype ", o->dtype);
    const int P = ctx->ctx->size;
    // the per-rank counts go down as the plan's recv_elems (ints); none: `elements` everywhere
    std::vector<int> counts;
    size_t total = 0;
    for (int q = 0; o->counts && q < P; q++) {
      GLOO_AMD_ENFORCE(o->counts[q] <= (size_t)INT32_MAX, "allgather: count ", o->counts[q], " of rank ", q,
                       " is too large");
      counts.push_back((int)o->counts[q]);
      total += o->counts[q];
    }
    if (!o->counts) total = o->elements * (size_t)P;
    if (total == 0) return;
    GLOO_AMD_ENFORCE(o->output, "null output");
    // in place or not is part of the cached schedule's key (the plan's
    // exchange does not depend on it: a block is one input either way)
    std::vector<void*> ins;
    if (o->input) ins.push_back(o->input);
    runCached(ctx, GLOO_HIP_ALGO_ALLGATHER, GLOO_HIP_SUM, o->dtype, ins, {o->output}, o->counts ? 0 : o->elements, 0,
              o->tag, o->stream, counts);
  });
}

int gloo_hip_gather(gloo_hip_context_t ctx, const gloo_hip_gather_options_t* o) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    GLOO_AMD_ENFORCE(gloo_hip_dtype_size(o->dtype) > 0, "unknown dtype ", o->dtype);
    const int P = ctx->ctx->size, me = ctx->ctx->rank;
    GLOO_AMD_ENFORCE(o->root >= 0 && o->root < P, "gather: root rank ", o->root, " outside [0, ", P, ")");  // gather.cc:26
    // {root}, or {root, c_0 ...}: the plan's recv_elems (ints)
    std::vector<int> re{o->root};
    size_t total = 0;
    for (int q = 0; o->counts && q < P; q++) {
      GLOO_AMD_ENFORCE(o->counts[q] <= (size_t)INT32_MAX, "gather: count ", o->counts[q], " of rank ", q,
                       " is too large");
      re.push_back((int)o->counts[q]);
      total += o->counts[q];
    }
    if (!o->counts) total = o->elements * (size_t)P;
    if (total == 0) return;
    const size_t mine = o->counts ? o->counts[me] : o->elements;
    GLOO_AMD_ENFORCE(o->input || mine == 0, "null input");  // gatherv.cc:79
    GLOO_AMD_ENFORCE(me != o->root || o->output, "null output on the root");
    // a rank without an output: the executor's one pointer is its input, which
    // no step of its plan reads as output 0 or writes (construction is
    // collective, so a rank with nothing to send still builds its executor)
    void* in = o->input;
    void* out = me == o->root ? o->output : in;
    runCached(ctx, GLOO_HIP_ALGO_GATHER, GLOO_HIP_SUM, o->dtype, {in}, {out}, o->counts ? 0 : o->elements, 0, o->tag,
              o->stream, re);
  });
}

int gloo_hip_scatter(gloo_hip_context_t ctx, const gloo_hip_scatter_options_t* o) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    GLOO_AMD_ENFORCE(gloo_hip_dtype_size(o->dtype) > 0, "unknown dtype ", o->dtype);
    const int P = ctx->ctx->size, me = ctx->ctx->rank;
    GLOO_AMD_ENFORCE(o->root >= 0 && o->root < P, "scatter: root rank ", o->root, " outside [0, ", P, ")");  // scatter.cc:27
    if (o->elements == 0) return;
    GLOO_AMD_ENFORCE(o->output, "null output");  // scatter.cc:28
    std::vector<void*> ins;
    if (me == o->root) {
      GLOO_AMD_ENFORCE(o->inputs, "scatter: the root has no inputs");  // scatter.cc:31
      for (int q = 0; q < P; q++) {
        GLOO_AMD_ENFORCE(o->inputs[q], "scatter: null input for rank ", q);
        ins.push_back(o->inputs[q]);
      }
    }
    runCached(ctx, GLOO_HIP_ALGO_SCATTER, GLOO_HIP_SUM, o->dtype, ins, {o->output}, o->elements, 0, o->tag, o->stream,
              {o->root});
  });
}

int gloo_hip_alltoall_create(gloo_hip_context_t ctx, int dtype, void* input, void* output, size_t count,
                             const int* matrix, gloo_hip_stream_t stream, int workspace, gloo_hip_algorithm_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && out, "null argument");
    GLOO_AMD_ENFORCE(gloo_hip_dtype_size(dtype) > 0, "unknown dtype ", dtype);
    const int P = ctx->ctx->size, me = ctx->ctx->rank;
    std::vector<int> m;
    if (matrix) {
      m.assign(matrix, matrix + (size_t)P * P);
      // the whole matrix, not only this rank's row and column: every rank derives every peer's plan from it
      for (size_t k = 0; k < m.size(); k++)
        GLOO_AMD_ENFORCE(m[k] >= 0, "alltoall: negative count ", m[k], " from rank ", k / P, " to rank ", k % P);
      count = 0;  // ignored with a matrix, and part of the call's hash
    }
    alltoallBuffers(me, P, dtype, count, gloo_amd::alltoallLists(me, P, m), input, output);
    auto a = std::make_unique<gloo_hip_algorithm>();
    a->exec = gloo_amd::PlanExecutor::create(ctx->ctx, GLOO_HIP_ALGO_ALLTOALL, GLOO_HIP_SUM, dtype,
                                             std::vector<void*>{output}, count, m, static_cast<hipStream_t>(stream),
                                             std::vector<void*>{input}, 0, workspace);
    *out = a.release();
  });
}

int gloo_hip_alltoall(gloo_hip_context_t ctx, const gloo_hip_alltoall_options_t* o) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && o, "null argument");
    const size_t es = gloo_hip_dtype_size(o->dtype);
    GLOO_AMD_ENFORCE(es > 0, "unknown dtype ", o->dtype);
    const int P = ctx->ctx->size, me = ctx->ctx->rank;
    GLOO_AMD_ENFORCE(!o->in_counts == !o->out_counts, "alltoall: ", o->in_counts ? "in_counts" : "out_counts",
                     " is given without ", o->in_counts ? "out_counts" : "in_counts", " (both, or neither)");
    const bool lists = o->in_counts != nullptr;
    // every refusal a rank can make from its own arguments comes first: before
    // the count exchange of the own-lists form and before any construction
    std::vector<int> m;  // the P x P matrix, once known
    if (o->matrix) {
      for (size_t k = 0; k < (size_t)P * P; k++) {
        GLOO_AMD_ENFORCE(o->matrix[k] <= (size_t)INT32_MAX, "alltoall: count ", o->matrix[k], " from rank ", k / P,
                         " to rank ", k % P, " is too large");
        m.push_back((int)o->matrix[k]);
      }
    }
    std::vector<int> mine;  // in_counts then out_counts
    if (lists) {
      for (int k = 0; k < 2 * P; k++) {
        const size_t c = k < P ? o->in_counts[k] : o->out_counts[k - P];
        GLOO_AMD_ENFORCE(c <= (size_t)INT32_MAX, "alltoall: ", k < P ? "in" : "out", "_count ", c, " for rank ", k % P,
                         " is too large");
        mine.push_back((int)c);
      }
      GLOO_AMD_ENFORCE(mine[me] == mine[P + me], "alltoall: rank ", me, "'s own block has in_count ", mine[me],
                       " but out_count ", mine[P + me]);  // alltoallv.cc:138
      if (o->matrix) {
        const std::vector<int> want = gloo_amd::alltoallLists(me, P, m);
        for (int k = 0; k < 2 * P; k++)
          GLOO_AMD_ENFORCE(mine[k] == want[k], "alltoall: ", k < P ? "in" : "out", "_counts[", k % P, "] is ", mine[k],
                           " but the matrix has ", want[k], k < P ? " from rank " : " to rank ", me,
                           k < P ? " to rank " : " from rank ", k % P);
      }
    }
    if (!lists && !o->matrix)
      GLOO_AMD_ENFORCE(o->elements <= SIZE_MAX / es / (size_t)P, "alltoall: ", o->elements,
                       " elements per block is too large");
    // the buffers, against what this rank knows of the call so far
    alltoallBuffers(me, P, o->dtype, o->elements, lists ? mine : gloo_amd::alltoallLists(me, P, m), o->input, o->output);
    if (lists && !o->matrix) {
      // The reference's alltoallv shape: a rank knows its own lists only.  The
      // cached schedule's construction is collective, so every rank must hit
      // and miss the cache alike, and a key made of a rank's own lists would
      // not do that (a change between ranks 0 and 1 leaves the others' lists
      // as they were).  So EVERY such call exchanges the lists once (the
      // context's exchange counter advances alike on every rank), every rank
      // assembles the same matrix and checks every pair from the same records,
      // and the call goes on as the matrix form, whose key is the whole matrix.
      std::vector<char> blob(mine.size() * sizeof(int));
      std::memcpy(blob.data(), mine.data(), blob.size());
      const auto all = ctx->ctx->allgather("alltoall/counts", blob);
      m.assign((size_t)P * P, 0);
      std::vector<int> outOf((size_t)P * P, 0);  // outOf[r * P + q]: what rank r expects from rank q
      for (int q = 0; q < P; q++) {
        GLOO_AMD_ENFORCE(all.at(q).size() == blob.size(), "alltoall: rank ", q, " exchanged ", all[q].size() / sizeof(int),
                         " counts, not ", 2 * P, " (every rank must call the same form)");
        std::vector<int> theirs(2 * (size_t)P);
        std::memcpy(theirs.data(), all[q].data(), blob.size());
        for (int r = 0; r < P; r++) {
          m[(size_t)q * P + r] = theirs[r];
          outOf[(size_t)q * P + r] = theirs[P + r];
        }
      }
      for (int q = 0; q < P; q++)
        for (int r = 0; r < P; r++)
          GLOO_AMD_ENFORCE(m[(size_t)q * P + r] == outOf[(size_t)r * P + q], "alltoall: rank ", q, " sends ",
                           m[(size_t)q * P + r], " elements to rank ", r, " (its in_counts[", r, "]) but rank ", r,
                           " expects ", outOf[(size_t)r * P + q], " from rank ", q, " (its out_counts[", q, "])");
    }
    // nothing to move anywhere: every rank sees that from the same values
    if (m.empty() ? o->elements == 0 : allZero(m)) return;
    runCached(ctx, GLOO_HIP_ALGO_ALLTOALL, GLOO_HIP_SUM, o->dtype, {o->input}, {o->output}, m.empty() ? o->elements : 0,
              0, o->tag, o->stream, m);
  });
}

double gloo_hip_algorithm_wait_seconds(gloo_hip_algorithm_t a) { return a ? a->exec->lastWaitSeconds() : 0.0; }

int gloo_hip_algorithm_set_profiling(gloo_hip_algorithm_t a, int on) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(a, "null algorithm");
    // 1: HIP events around every chunk reduction (eager runs);
    // 2: device stamps inside the kernels (graph replay kept)
    a->exec->setProfiling(on == 1);
    a->exec->setStamping(on == 2);
  });
}

int gloo_hip_algorithm_stats(gloo_hip_algorithm_t a, double* stats) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(a && stats, "null argument");
    stats[0] = a->exec->lastReduceSeconds();
    stats[1] = a->exec->lastReduceBytes();
    stats[2] = (double)a->exec->lastReduceCount();
    stats[3] = a->exec->lastWaitSeconds();
  });
}

namespace {
void modeOf(const gloo_amd::PlanExecutor& e, int* mode) {
  mode[0] = e.deviceSignalling() ? 1 : 0;
  mode[1] = e.hostArena() ? 2 : e.fineGrainedArena() ? 1 : 0;
  mode[2] = (e.foldSendUsed() ? 2 : 0) | (e.ownStream() ? 4 : 0);
  mode[3] = e.graphed() ? 1 : e.interpreted() ? 1 + e.interpSlices() : 0;
  gloo_amd::setError(0, e.graphError().empty() ? "" : "graph capture abandoned: " + e.graphError());
}
}  // namespace

int gloo_hip_algorithm_mode(gloo_hip_algorithm_t a, int* mode) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(a && mode, "null argument");
    modeOf(*a->exec, mode);
  });
}

int gloo_hip_context_mode(gloo_hip_context_t ctx, int* mode) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && mode, "null argument");
    GLOO_AMD_ENFORCE(ctx->last, "no function-style call on this context yet");
    modeOf(*ctx->last, mode);
  });
}

int gloo_hip_context_create_kv(int rank, int size, int device, int timeout_ms, gloo_hip_kv_set_fn set,
                               gloo_hip_kv_get_fn get, void* user, gloo_hip_context_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(out && set && get, "null argument");
    auto c = std::make_unique<gloo_hip_context>();
    c->ctx = std::make_shared<gloo_amd::Context>(
        rank, size, std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 30000));
    c->ctx->connect(std::make_shared<gloo_amd::KvCallbackStore>(set, get, user), device);
    *out = c.release();
  });
}

int gloo_hip_transport_create(gloo_hip_context_t ctx, gloo_hip_stream_t stream, gloo_hip_transport_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(ctx && out, "null argument");
    auto t = std::make_unique<gloo_hip_transport>();
    t->dev = std::make_unique<gloo_amd::transport::Device>(ctx->ctx, static_cast<hipStream_t>(stream));
    *out = t.release();
  });
}

int gloo_hip_transport_destroy(gloo_hip_transport_t t) {
  return guarded([&] { delete t; });
}

int gloo_hip_buffer_create(gloo_hip_transport_t t, int peer, int slot, void* ptr, size_t size, int is_send,
                           gloo_hip_buffer_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(t && out, "null argument");
    auto& pair = t->dev->getPair(peer);
    auto b = std::make_unique<gloo_hip_buffer>();
    b->buf = is_send ? pair.createSendBuffer(slot, ptr, size) : pair.createRecvBuffer(slot, ptr, size);
    *out = b.release();
  });
}

int gloo_hip_buffer_destroy(gloo_hip_buffer_t b) {
  return guarded([&] { delete b; });
}

int gloo_hip_buffer_send(gloo_hip_buffer_t b, size_t offset, size_t length, size_t roffset) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->send(offset, length, roffset);
  });
}

int gloo_hip_buffer_wait_recv(gloo_hip_buffer_t b) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->waitRecv();
  });
}

int gloo_hip_buffer_wait_send(gloo_hip_buffer_t b) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->waitSend();
  });
}

int gloo_hip_ubuf_create(gloo_hip_transport_t t, void* ptr, size_t size, gloo_hip_ubuf_t* out) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(t && out && (ptr || size == 0), "bad arguments");
    auto b = std::make_unique<gloo_hip_ubuf>();
    b->buf = std::make_unique<gloo_amd::transport::UnboundBuffer>(t->dev.get(), ptr, size);
    *out = b.release();
  });
}

int gloo_hip_ubuf_destroy(gloo_hip_ubuf_t b) {
  return guarded([&] { delete b; });
}

int gloo_hip_ubuf_send(gloo_hip_ubuf_t b, int dst, uint64_t slot, size_t offset, size_t nbytes) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->send(dst, slot, offset, nbytes);
  });
}

int gloo_hip_ubuf_recv(gloo_hip_ubuf_t b, const int* srcs, int nsrcs, uint64_t slot, size_t offset, size_t nbytes) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b && srcs && nsrcs > 0, "bad arguments");
    b->buf->recv(std::vector<int>(srcs, srcs + nsrcs), slot, offset, nbytes);
  });
}

namespace {
int waitResult(int rc, bool done) { return rc == GLOO_HIP_OK && !done ? 1 : rc; }
}  // namespace

int gloo_hip_ubuf_wait_recv(gloo_hip_ubuf_t b, int* rank, int timeout_ms) {
  bool done = false;
  const int rc = guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    done = b->buf->waitRecv(rank, std::chrono::milliseconds(timeout_ms));
  });
  return waitResult(rc, done);
}

int gloo_hip_ubuf_wait_send(gloo_hip_ubuf_t b, int* rank, int timeout_ms) {
  bool done = false;
  const int rc = guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    done = b->buf->waitSend(rank, std::chrono::milliseconds(timeout_ms));
  });
  return waitResult(rc, done);
}

int gloo_hip_ubuf_abort_wait_recv(gloo_hip_ubuf_t b) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->abortWaitRecv();
  });
}

int gloo_hip_ubuf_abort_wait_send(gloo_hip_ubuf_t b) {
  return guarded([&] {
    GLOO_AMD_ENFORCE(b, "null buffer");
    b->buf->abortWaitSend();
  });
}

}  // extern "C"
