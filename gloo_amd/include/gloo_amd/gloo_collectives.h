// gloo_collectives.h — the reference's new-style collectives, called the way a
// Gloo program calls them, run on the MI355X path.
//
// HEADER-ONLY and compiled on the GLOO side (like gloo_bridge.h): it reads
// the reference's option objects and crosses into libgloo_amd.so only
// through the C-ABI of include/gloo_amd.h.
//
//   gloo::allreduce(const gloo::AllreduceOptions&)  (gloo/allreduce.h:89-193,
//        gloo/allreduce.cc:97-145)  ->  gloo::hip::allreduce(opts[, stream])
//   gloo::reduce(gloo::ReduceOptions&)               (gloo/reduce.h:19-110,
//        gloo/reduce.cc:21-247)     ->  gloo::hip::reduce(opts[, stream])
//   gloo::broadcast(gloo::BroadcastOptions&)         (gloo/broadcast.h:16-89,
//        gloo/broadcast.cc:16-95)   ->  gloo::hip::broadcast(opts[, stream])
//        (bytes only: no reduce function; one-to-all from the root instead of
//        the reference's binomial tree, the same bytes on every rank)
//   gloo::allgather(gloo::AllgatherOptions&)         (gloo/allgather.h,
//        gloo/allgather.cc:19-97)   ->  gloo::hip::allgather(opts[, stream])
//   gloo::allgatherv(gloo::AllgathervOptions&)       (gloo/allgatherv.h,
//        gloo/allgatherv.cc:71-140) ->  gloo::hip::allgatherv(opts[, stream])
//        (bytes only; every rank sends its block straight to every peer
//        instead of round the reference's ring, the same bytes on every rank)
//   gloo::gather(gloo::GatherOptions&)               (gloo/gather.h,
//        gloo/gather.cc)            ->  gloo::hip::gather(opts[, stream])
//   gloo::gatherv(gloo::GathervOptions&)             (gloo/gatherv.h,
//        gloo/gatherv.cc:71-107)    ->  gloo::hip::gatherv(opts[, stream])
//   gloo::scatter(gloo::ScatterOptions&)             (gloo/scatter.h,
//        gloo/scatter.cc:19-61)     ->  gloo::hip::scatter(opts[, stream])
//        (bytes only; the reference's own route, every block one hop to or
//        from the root)
//   gloo::alltoall(gloo::AlltoallOptions&)           (gloo/alltoall.h,
//        gloo/alltoall.cc:19-72)    ->  gloo::hip::alltoall(opts[, stream])
//   gloo::alltoallv(gloo::AlltoallvOptions&)         (gloo/alltoallv.h,
//        gloo/alltoallv.cc:117-170) ->  gloo::hip::alltoallv(opts[, stream])
//        (bytes only; the reference's own route, every block one hop; input
//        and output may share no byte; alltoallv costs one host exchange of
//        the counts per call, include/gloo_amd.h)
//
// The caller fills the SAME option object it would hand to gloo::allreduce /
// gloo::reduce: setInput(s) / setOutput(s) with DEVICE pointers (the
// context's createUnboundBuffer only records pointer and size; nothing is
// sent through it), setReduceFunction, setAlgorithm (RING, BCUBE), setTag,
// setMaxSegmentSize, setRoot.  The options are read through pointers to
// their protected members (taken in a derived class, so no layout is
// assumed).  Results are the reference's bits: the schedules are the
// reference's (RING and BCUBE segment geometry, reduce's ring + gather),
// verified against its outputs (tests/golden/newstyle_golden.npz).
//
// The element type and operation come from the reduce function, which is
// untyped in the options (gloo/allreduce.h:36): the reference's own
// gloo::sum / product / max / min<T> (gloo/math.h:15-73) map to the
// library's kernels for every instantiated T (+ c10::BFloat16 under
// GLOO_USE_TORCH_DTYPES); any other function must be registered with a
// device implementation (registerReduction, ReductionType CUSTOM), because
// a host function cannot run on device memory.
//
// Streams (docs/cuda.md:6-13): without one, the outputs are complete on
// return; with one, the work is ordered on it and the caller synchronises.
//
// The library context behind a gloo::Context is created by the first call on
// it (a collective exchange over gloo::allgather, as for gloo_bridge.h's
// algorithms) and kept, with the cached schedules, until releaseContext —
// a collective call every rank makes while the gloo::Context is alive.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "gloo/allgather.h"
#include "gloo/allgatherv.h"
#include "gloo/allreduce.h"
#include "gloo/alltoall.h"
#include "gloo/alltoallv.h"
#include "gloo/broadcast.h"
#include "gloo/gather.h"
#include "gloo/gatherv.h"
#include "gloo/math.h"
#include "gloo/reduce.h"
#include "gloo/scatter.h"
#include "gloo_amd/gloo_bridge.h"

namespace gloo {
namespace hip {

namespace detail {

using ReduceFn = void (*)(void*, const void*, const void*, size_t);

struct Reduction {
  int op = 0;
  int dtype = -1;
  size_t elementSize = 0;
};

struct Registry {
  std::mutex m;
  std::vector<std::pair<ReduceFn, Reduction>> fns;
  template <typename T>
  void builtins() {
    const int dt = ::gloo::hip_bridge::DType<T>::value;
    fns.push_back({static_cast<ReduceFn>(&::gloo::sum<T>), {GLOO_HIP_SUM, dt, sizeof(T)}});
    fns.push_back({static_cast<ReduceFn>(&::gloo::product<T>), {GLOO_HIP_PRODUCT, dt, sizeof(T)}});
    fns.push_back({static_cast<ReduceFn>(&::gloo::max<T>), {GLOO_HIP_MAX, dt, sizeof(T)}});
    fns.push_back({static_cast<ReduceFn>(&::gloo::min<T>), {GLOO_HIP_MIN, dt, sizeof(T)}});
  }
  static Registry& get() {
    static Registry* r = [] {
      auto* x = new Registry();
      x->builtins<int8_t>();
      x->builtins<uint8_t>();
      x->builtins<int32_t>();
      x->builtins<uint32_t>();
      x->builtins<int64_t>();
      x->builtins<uint64_t>();
      x->builtins<::gloo::float16>();
      x->builtins<float>();
      x->builtins<double>();
#if GLOO_USE_TORCH_DTYPES
      x->builtins<c10::BFloat16>();
#endif
      return x;
    }();
    return *r;
  }
};

// The operation and element type of an options object's reduce function.
inline Reduction classify(const std::function<void(void*, const void*, const void*, size_t)>& f,
                          size_t elementSize) {
  GLOO_ENFORCE(f, "no reduce function set (setReduceFunction)");
  const ReduceFn* target = f.target<ReduceFn>();
  GLOO_ENFORCE(target != nullptr,
               "the device path needs the reduce function as a plain function pointer: one of "
               "gloo::sum/product/max/min<T> or a function registered with gloo::hip::registerReduction");
  Registry& r = Registry::get();
  std::lock_guard<std::mutex> lk(r.m);
  for (const auto& e : r.fns)
    if (e.first == *target) {
      GLOO_ENFORCE_EQ(e.second.elementSize, elementSize, "the reduce function's element size differs from the "
                                                         "buffers' (setInput<T> / setOutput<T>)");
      return e.second;
    }
  GLOO_ENFORCE(false, "unknown reduce function: register its device implementation with "
                      "gloo::hip::registerReduction");
  return {};
}

// The library context of one gloo::Context (kept until releaseContext).
struct Contexts {
  std::mutex m;
  std::map<const ::gloo::Context*, std::pair<std::shared_ptr<::gloo::Context>,
                                             std::unique_ptr<::gloo::hip_bridge::BootstrapContext>>> byContext;
  static Contexts& get() {
    static Contexts* c = new Contexts();  // never destroyed: tear-down is collective (releaseContext)
    return *c;
  }
};

inline gloo_hip_context_t contextFor(const std::shared_ptr<::gloo::Context>& c, const void* anyDevicePtr) {
  Contexts& cs = Contexts::get();
  {
    std::lock_guard<std::mutex> lk(cs.m);
    auto it = cs.byContext.find(c.get());
    if (it != cs.byContext.end()) return it->second.second->handle();
  }
  // The bootstrap is collective: never under the registry's lock, which the
  // other ranks of this process (threads) need for their own contexts.
  std::unique_ptr<::gloo::hip_bridge::BootstrapContext> boot(
      new ::gloo::hip_bridge::BootstrapContext(c, ::gloo::hip_bridge::deviceOf(anyDevicePtr)));
  std::lock_guard<std::mutex> lk(cs.m);
  auto& e = cs.byContext[c.get()];
  e.first = c;
  e.second = std::move(boot);
  return e.second->handle();
}

// Read access to the options' protected state: pointers to members named
// in a derived class (no object of the derived type is ever formed).
struct AllreduceAccess : ::gloo::AllreduceOptions {
  static const ::gloo::detail::AllreduceOptionsImpl& impl(const ::gloo::AllreduceOptions& o) {
    return o.*(&AllreduceAccess::impl_);
  }
};
struct ReduceAccess : ::gloo::ReduceOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::ReduceOptions& o) {
    return o.*(&ReduceAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::ReduceOptions& o) {
    return o.*(&ReduceAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::ReduceOptions& o) {
    return o.*(&ReduceAccess::out);
  }
  static size_t get_elements(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::elements); }
  static size_t get_elementSize(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::elementSize); }
  static int get_root(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::root); }
  static const Func& get_reduce(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::reduce); }
  static uint32_t get_tag(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::tag); }
  static size_t get_maxSegmentSize(const ::gloo::ReduceOptions& o) { return o.*(&ReduceAccess::maxSegmentSize); }
};

struct BroadcastAccess : ::gloo::BroadcastOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::BroadcastOptions& o) {
    return o.*(&BroadcastAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::BroadcastOptions& o) {
    return o.*(&BroadcastAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::BroadcastOptions& o) {
    return o.*(&BroadcastAccess::out);
  }
  static size_t get_elements(const ::gloo::BroadcastOptions& o) { return o.*(&BroadcastAccess::elements); }
  static size_t get_elementSize(const ::gloo::BroadcastOptions& o) { return o.*(&BroadcastAccess::elementSize); }
  static int get_root(const ::gloo::BroadcastOptions& o) { return o.*(&BroadcastAccess::root); }
  static uint32_t get_tag(const ::gloo::BroadcastOptions& o) { return o.*(&BroadcastAccess::tag); }
};

struct AllgatherAccess : ::gloo::AllgatherOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::AllgatherOptions& o) {
    return o.*(&AllgatherAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::AllgatherOptions& o) {
    return o.*(&AllgatherAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::AllgatherOptions& o) {
    return o.*(&AllgatherAccess::out);
  }
  static size_t get_elementSize(const ::gloo::AllgatherOptions& o) { return o.*(&AllgatherAccess::elementSize); }
  static uint32_t get_tag(const ::gloo::AllgatherOptions& o) { return o.*(&AllgatherAccess::tag); }
};

struct AllgathervAccess : ::gloo::AllgathervOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::AllgathervOptions& o) {
    return o.*(&AllgathervAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::AllgathervOptions& o) {
    return o.*(&AllgathervAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::AllgathervOptions& o) {
    return o.*(&AllgathervAccess::out);
  }
  static const std::vector<size_t>& get_elements(const ::gloo::AllgathervOptions& o) {
    return o.*(&AllgathervAccess::elements);
  }
  static size_t get_elementSize(const ::gloo::AllgathervOptions& o) { return o.*(&AllgathervAccess::elementSize); }
  static uint32_t get_tag(const ::gloo::AllgathervOptions& o) { return o.*(&AllgathervAccess::tag); }
};

struct GatherAccess : ::gloo::GatherOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::GatherOptions& o) {
    return o.*(&GatherAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::GatherOptions& o) {
    return o.*(&GatherAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::GatherOptions& o) {
    return o.*(&GatherAccess::out);
  }
  static size_t get_elementSize(const ::gloo::GatherOptions& o) { return o.*(&GatherAccess::elementSize); }
  static int get_root(const ::gloo::GatherOptions& o) { return o.*(&GatherAccess::root); }
  static uint32_t get_tag(const ::gloo::GatherOptions& o) { return o.*(&GatherAccess::tag); }
};

struct GathervAccess : ::gloo::GathervOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::GathervOptions& o) {
    return o.*(&GathervAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::GathervOptions& o) {
    return o.*(&GathervAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::GathervOptions& o) {
    return o.*(&GathervAccess::out);
  }
  static const std::vector<size_t>& get_elementsPerRank(const ::gloo::GathervOptions& o) {
    return o.*(&GathervAccess::elementsPerRank);
  }
  static size_t get_elementSize(const ::gloo::GathervOptions& o) { return o.*(&GathervAccess::elementSize); }
  static int get_root(const ::gloo::GathervOptions& o) { return o.*(&GathervAccess::root); }
  static uint32_t get_tag(const ::gloo::GathervOptions& o) { return o.*(&GathervAccess::tag); }
};

struct ScatterAccess : ::gloo::ScatterOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::ScatterOptions& o) {
    return o.*(&ScatterAccess::context);
  }
  static const std::vector<std::unique_ptr<::gloo::transport::UnboundBuffer>>& get_in(
      const ::gloo::ScatterOptions& o) {
    return o.*(&ScatterAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::ScatterOptions& o) {
    return o.*(&ScatterAccess::out);
  }
  static size_t get_elementSize(const ::gloo::ScatterOptions& o) { return o.*(&ScatterAccess::elementSize); }
  static int get_root(const ::gloo::ScatterOptions& o) { return o.*(&ScatterAccess::root); }
  static uint32_t get_tag(const ::gloo::ScatterOptions& o) { return o.*(&ScatterAccess::tag); }
};

struct AlltoallAccess : ::gloo::AlltoallOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::AlltoallOptions& o) {
    return o.*(&AlltoallAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::AlltoallOptions& o) {
    return o.*(&AlltoallAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::AlltoallOptions& o) {
    return o.*(&AlltoallAccess::out);
  }
  static size_t get_elementSize(const ::gloo::AlltoallOptions& o) { return o.*(&AlltoallAccess::elementSize); }
  static uint32_t get_tag(const ::gloo::AlltoallOptions& o) { return o.*(&AlltoallAccess::tag); }
};

struct AlltoallvAccess : ::gloo::AlltoallvOptions {
  static const std::shared_ptr<::gloo::Context>& get_context(const ::gloo::AlltoallvOptions& o) {
    return o.*(&AlltoallvAccess::context);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_in(const ::gloo::AlltoallvOptions& o) {
    return o.*(&AlltoallvAccess::in);
  }
  static const std::unique_ptr<::gloo::transport::UnboundBuffer>& get_out(const ::gloo::AlltoallvOptions& o) {
    return o.*(&AlltoallvAccess::out);
  }
  // byte lengths per rank (alltoallv.cc:19-31 splitOffsetsAndLengths); the offsets are their prefix sums
  static const std::vector<size_t>& get_inLengths(const ::gloo::AlltoallvOptions& o) {
    return o.*(&AlltoallvAccess::inLengthPerRank);
  }
  static const std::vector<size_t>& get_outLengths(const ::gloo::AlltoallvOptions& o) {
    return o.*(&AlltoallvAccess::outLengthPerRank);
  }
  static size_t get_elementSize(const ::gloo::AlltoallvOptions& o) { return o.*(&AlltoallvAccess::elementSize); }
  static uint32_t get_tag(const ::gloo::AlltoallvOptions& o) { return o.*(&AlltoallvAccess::tag); }
};

}  // namespace detail

// A CUSTOM reduce function for the new-style calls: `host` is what the
// caller passes to setReduceFunction (the reference calls it on host
// memory), `device` its device implementation (gloo_bridge.h), which must
// outlive every call that uses it.
template <typename T>
void registerReduction(detail::ReduceFn host, const ::gloo::HipReductionFunction<T>& device) {
  GLOO_ENFORCE(host != nullptr, "null host function");
  detail::Registry& r = detail::Registry::get();
  std::lock_guard<std::mutex> lk(r.m);
  for (auto& e : r.fns)
    if (e.first == host) {
      e.second = {device.op(), ::gloo::hip_bridge::DType<T>::value, sizeof(T)};
      return;
    }
  r.fns.push_back({host, {device.op(), ::gloo::hip_bridge::DType<T>::value, sizeof(T)}});
}

// gloo::allreduce(opts) (gloo/allreduce.cc:97-145) on device buffers.
inline void allreduce(const ::gloo::AllreduceOptions& opts, hipStream_t stream = nullptr) {
  const auto& o = detail::AllreduceAccess::impl(opts);
  GLOO_ENFORCE(o.out.size() > 0, "no output buffer");  // gloo/allreduce.cc:102
  if (o.elements == 0) return;                          // gloo/allreduce.cc:98-100
  const detail::Reduction red = detail::classify(o.reduce, o.elementSize);
  std::vector<void*> ins, outs;
  for (const auto& b : o.in) {
    GLOO_ENFORCE_GE(b->size, o.elements * o.elementSize, "input buffer too small");
    ins.push_back(b->ptr);
  }
  for (const auto& b : o.out) {
    GLOO_ENFORCE_GE(b->size, o.elements * o.elementSize, "output buffer too small");
    outs.push_back(b->ptr);
  }
  GLOO_ENFORCE(o.algorithm == ::gloo::detail::AllreduceOptionsImpl::UNSPECIFIED ||
                   o.algorithm == ::gloo::detail::AllreduceOptionsImpl::RING ||
                   o.algorithm == ::gloo::detail::AllreduceOptionsImpl::BCUBE,
               "Algorithm not handled.");  // gloo/allreduce.cc:142-143
  gloo_hip_context_t ctx = detail::contextFor(o.context, outs[0]);
  gloo_hip_allreduce_options_t a;
  a.algorithm = o.algorithm == ::gloo::detail::AllreduceOptionsImpl::BCUBE ? GLOO_HIP_ALLREDUCE_BCUBE
                                                                            : GLOO_HIP_ALLREDUCE_RING;
  a.op = red.op;
  a.dtype = red.dtype;
  a.inputs = ins.empty() ? nullptr : ins.data();
  a.ninputs = (int)ins.size();
  a.outputs = outs.data();
  a.noutputs = (int)outs.size();
  a.elements = o.elements;
  a.max_segment_bytes = o.maxSegmentSize;
  a.tag = o.tag;
  a.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_allreduce(ctx, &a), "gloo::hip::allreduce");
}

// gloo::reduce(opts) (gloo/reduce.cc:21-247) on device buffers: only the
// root's output holds the result, as in the reference.
inline void reduce(::gloo::ReduceOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::ReduceAccess;
  const auto& ctxp = A::get_context(opts);
  const size_t elements = A::get_elements(opts);
  if (elements == 0) return;  // gloo/reduce.cc:22-24
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");
  const int root = A::get_root(opts);
  GLOO_ENFORCE(root >= 0 && root < ctxp->size, "invalid root ", root);  // gloo/reduce.cc:31-32
  const detail::Reduction red = detail::classify(A::get_reduce(opts), A::get_elementSize(opts));
  void* out = A::get_out(opts)->ptr;
  void* in = A::get_in(opts) ? A::get_in(opts)->ptr : nullptr;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, out);
  gloo_hip_reduce_options_t r;
  r.op = red.op;
  r.dtype = red.dtype;
  r.input = in;
  r.output = out;
  r.elements = elements;
  r.root = root;
  r.max_segment_bytes = A::get_maxSegmentSize(opts);
  r.tag = A::get_tag(opts);
  r.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_reduce_to_root(ctx, &r), "gloo::hip::reduce");
}

// gloo::broadcast(opts) (gloo/broadcast.cc:16-95) on device buffers: every
// rank's output receives the bytes of the root's input (of its output, when
// it set none).  The options carry an element size and no type, and a
// broadcast moves bytes, so the call goes down as elements * elementSize
// elements of uint8.
inline void broadcast(::gloo::BroadcastOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::BroadcastAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");
  const int root = A::get_root(opts);
  GLOO_ENFORCE(root >= 0 && root < ctxp->size, "invalid root ", root);  // gloo/broadcast.cc:28
  const size_t bytes = A::get_elements(opts) * A::get_elementSize(opts);
  void* out = A::get_out(opts)->ptr;
  const bool isRoot = ctxp->rank == root;
  GLOO_ENFORCE(isRoot || !A::get_in(opts), "Non-root may not specify input");  // gloo/broadcast.cc:38
  if (bytes == 0) return;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, out);
  gloo_hip_broadcast_options_t b;
  b.dtype = GLOO_HIP_U8;
  b.input = isRoot && A::get_in(opts) ? A::get_in(opts)->ptr : nullptr;
  b.output = out;
  b.elements = bytes;
  b.root = root;
  b.tag = A::get_tag(opts);
  b.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_broadcast(ctx, &b), "gloo::hip::broadcast");
}

// gloo::allgather(opts) (gloo/allgather.cc:19-97) on device buffers: every
// rank's output receives rank 0's input, rank 1's input, ... back to back; no
// input is the in-place form (:47-54).  The options carry an element size and
// no type, and an allgather moves bytes, so the call goes down in uint8.
inline void allgather(::gloo::AllgatherOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::AllgatherAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");
  GLOO_ENFORCE(A::get_elementSize(opts) > 0);  // gloo/allgather.cc:26
  const size_t outBytes = A::get_out(opts)->size;
  if (A::get_in(opts)) {
    GLOO_ENFORCE_EQ(outBytes, A::get_in(opts)->size * ctxp->size);  // gloo/allgather.cc:39
  } else {
    GLOO_ENFORCE_EQ(outBytes % ctxp->size, 0);  // gloo/allgather.cc:41
  }
  if (outBytes == 0) return;
  void* out = A::get_out(opts)->ptr;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, out);
  gloo_hip_allgather_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.input = A::get_in(opts) ? A::get_in(opts)->ptr : nullptr;
  g.output = out;
  g.elements = outBytes / ctxp->size;
  g.counts = nullptr;
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_allgather(ctx, &g), "gloo::hip::allgather");
}

// gloo::allgatherv(opts) (gloo/allgatherv.cc:71-140): rank q contributes
// elements[q] elements, the output at their prefix offsets (:90-101).
inline void allgatherv(::gloo::AllgathervOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::AllgathervAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");
  const size_t es = A::get_elementSize(opts);
  GLOO_ENFORCE(es > 0);  // gloo/allgatherv.cc:78
  std::vector<size_t> bytes;
  size_t total = 0;
  for (size_t e : A::get_elements(opts)) {
    bytes.push_back(e * es);
    total += e * es;
  }
  GLOO_ENFORCE_EQ(bytes.size(), (size_t)ctxp->size);
  if (A::get_in(opts)) GLOO_ENFORCE_EQ(bytes[ctxp->rank], A::get_in(opts)->size);  // gloo/allgatherv.cc:105
  if (total == 0) return;
  void* out = A::get_out(opts)->ptr;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, out);
  gloo_hip_allgather_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.input = A::get_in(opts) ? A::get_in(opts)->ptr : nullptr;
  g.output = out;
  g.elements = 0;
  g.counts = bytes.data();
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_allgather(ctx, &g), "gloo::hip::allgatherv");
}

// gloo::gather(opts) (gloo/gather.cc) on device buffers: the root's output
// receives rank 0's input, rank 1's input, ... back to back; a rank that is
// not the root needs no output.  The options carry an element size and no
// type, and a gather moves bytes, so the call goes down in uint8.
inline void gather(::gloo::GatherOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::GatherAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_elementSize(opts) > 0);
  GLOO_ENFORCE(A::get_in(opts), "no input buffer");
  const int root = A::get_root(opts);
  GLOO_ENFORCE(root >= 0 && root < ctxp->size);
  const size_t inBytes = A::get_in(opts)->size;
  if (ctxp->rank == root) {
    GLOO_ENFORCE(A::get_out(opts), "no output buffer on the root");
    GLOO_ENFORCE_EQ(A::get_out(opts)->size, inBytes * ctxp->size);
  }
  if (inBytes == 0) return;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, A::get_in(opts)->ptr);
  gloo_hip_gather_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.root = root;
  g.input = A::get_in(opts)->ptr;
  g.output = ctxp->rank == root ? A::get_out(opts)->ptr : nullptr;
  g.elements = inBytes;
  g.counts = nullptr;
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_gather(ctx, &g), "gloo::hip::gather");
}

// gloo::gatherv(opts) (gloo/gatherv.cc:71-107): rank q contributes
// elementsPerRank[q] elements, the root's output at their prefix offsets
// (:82-96).
inline void gatherv(::gloo::GathervOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::GathervAccess;
  const auto& ctxp = A::get_context(opts);
  const size_t es = A::get_elementSize(opts);
  GLOO_ENFORCE(es > 0);                              // gloo/gatherv.cc:78
  GLOO_ENFORCE(A::get_in(opts), "no input buffer");  // :79
  const int root = A::get_root(opts);
  GLOO_ENFORCE(root >= 0 && root < ctxp->size);
  std::vector<size_t> bytes;
  size_t total = 0;
  for (size_t e : A::get_elementsPerRank(opts)) {
    bytes.push_back(e * es);
    total += e * es;
  }
  GLOO_ENFORCE_EQ(bytes.size(), (size_t)ctxp->size);
  GLOO_ENFORCE_GE(A::get_in(opts)->size, bytes[ctxp->rank]);  // :103
  if (ctxp->rank == root) GLOO_ENFORCE(A::get_out(opts), "no output buffer on the root");
  if (total == 0) return;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, A::get_in(opts)->ptr);
  gloo_hip_gather_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.root = root;
  g.input = A::get_in(opts)->ptr;
  g.output = ctxp->rank == root ? A::get_out(opts)->ptr : nullptr;
  g.elements = 0;
  g.counts = bytes.data();
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_gather(ctx, &g), "gloo::hip::gatherv");
}

// gloo::scatter(opts) (gloo/scatter.cc:19-61): rank q's output receives the
// root's input q; the root's inputs are separate buffers (:31-35).
inline void scatter(::gloo::ScatterOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::ScatterAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_elementSize(opts) > 0);  // gloo/scatter.cc:26
  const int root = A::get_root(opts);
  GLOO_ENFORCE(root >= 0 && root < ctxp->size);  // :27
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");  // :28
  const size_t outBytes = A::get_out(opts)->size;
  std::vector<void*> ins;
  if (ctxp->rank == root) {
    GLOO_ENFORCE_EQ(A::get_in(opts).size(), (size_t)ctxp->size);  // :31
    for (const auto& b : A::get_in(opts)) {
      GLOO_ENFORCE_EQ(b->size, outBytes);  // :34
      ins.push_back(b->ptr);
    }
  }
  if (outBytes == 0) return;
  void* out = A::get_out(opts)->ptr;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, out);
  gloo_hip_scatter_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.root = root;
  g.output = out;
  g.inputs = ctxp->rank == root ? ins.data() : nullptr;
  g.elements = outBytes;
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_scatter(ctx, &g), "gloo::hip::scatter");
}

// gloo::alltoall(opts) (gloo/alltoall.cc:19-72) on device buffers: block q of
// rank r's output receives block r of rank q's input, every block in->size /
// P bytes.  The options carry an element size and no type, and an alltoall
// moves bytes, so the call goes down in uint8.  Input and output may share no
// byte (the reference's memcpy of the own block asks the same).
inline void alltoall(::gloo::AlltoallOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::AlltoallAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_elementSize(opts) > 0);            // gloo/alltoall.cc:26
  GLOO_ENFORCE(A::get_in(opts), "no input buffer");      // :27
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");    // :28
  const size_t bytes = A::get_in(opts)->size;
  GLOO_ENFORCE(bytes % (size_t)ctxp->size == 0);         // :29
  GLOO_ENFORCE(bytes == A::get_out(opts)->size);         // :30
  if (bytes == 0) return;
  gloo_hip_context_t ctx = detail::contextFor(ctxp, A::get_out(opts)->ptr);
  gloo_hip_alltoall_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.input = A::get_in(opts)->ptr;
  g.output = A::get_out(opts)->ptr;
  g.elements = bytes / (size_t)ctxp->size;
  g.in_counts = g.out_counts = g.matrix = nullptr;
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_alltoall(ctx, &g), "gloo::hip::alltoall");
}

// gloo::alltoallv(opts) (gloo/alltoallv.cc:117-170): this rank sends
// inLengthPerRank[q] bytes to rank q and receives outLengthPerRank[q] from it,
// at the prefix offsets (:19-31).  A rank knows its own lists only, so every
// call exchanges them once on the host and every rank checks every pair
// (include/gloo_amd.h, the own-lists form of gloo_hip_alltoall).
inline void alltoallv(::gloo::AlltoallvOptions& opts, hipStream_t stream = nullptr) {
  using A = detail::AlltoallvAccess;
  const auto& ctxp = A::get_context(opts);
  GLOO_ENFORCE(A::get_elementSize(opts) > 0);            // gloo/alltoallv.cc:130
  GLOO_ENFORCE(A::get_in(opts), "no input buffer");      // :131
  GLOO_ENFORCE(A::get_out(opts), "no output buffer");    // :132
  const std::vector<size_t>& in = A::get_inLengths(opts);
  const std::vector<size_t>& out = A::get_outLengths(opts);
  GLOO_ENFORCE_EQ(in.size(), (size_t)ctxp->size);        // :52
  GLOO_ENFORCE_EQ(out.size(), (size_t)ctxp->size);       // :89
  GLOO_ENFORCE(in[ctxp->rank] == out[ctxp->rank]);       // :138
  gloo_hip_context_t ctx = detail::contextFor(ctxp, A::get_out(opts)->ptr);
  gloo_hip_alltoall_options_t g;
  g.dtype = GLOO_HIP_U8;
  g.input = A::get_in(opts)->ptr;
  g.output = A::get_out(opts)->ptr;
  g.elements = 0;
  g.in_counts = in.data();
  g.out_counts = out.data();
  g.matrix = nullptr;
  g.tag = A::get_tag(opts);
  g.stream = stream;
  ::gloo::hip_bridge::check(gloo_hip_alltoall(ctx, &g), "gloo::hip::alltoallv");
}

// Collective: tears down the library context (and its cached schedules)
// behind `context`; every rank calls it, in the same order relative to its
// other collectives, while the gloo::Context is alive.
inline void releaseContext(const std::shared_ptr<::gloo::Context>& context) {
  detail::Contexts& cs = detail::Contexts::get();
  std::unique_ptr<::gloo::hip_bridge::BootstrapContext> boot;
  {
    std::lock_guard<std::mutex> lk(cs.m);
    auto it = cs.byContext.find(context.get());
    if (it == cs.byContext.end()) return;
    boot = std::move(it->second.second);
    cs.byContext.erase(it);
  }
  boot.reset();
}

}  // namespace hip
}  // namespace gloo
