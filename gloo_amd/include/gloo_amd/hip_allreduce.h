// hip_allreduce.h — C++ drop-in surface for Gloo's GPU reducing algorithms.
//
//   gloo::CudaReductionFunction<T>      -> gloo_amd::HipReductionFunction<T>
//                                          (gloo/cuda.h:286-358)
//   gloo::CudaAllreduceRingChunked<T,W> -> gloo_amd::HipAllreduceRingChunked<T>
//                                          (gloo/cuda_allreduce_ring_chunked.h:19-26)
//   gloo::CudaAllreduceHalvingDoubling  -> gloo_amd::HipAllreduceHalvingDoubling<T>
//                                          (gloo/cuda_allreduce_halving_doubling.h:25-30)
//   gloo::CudaAllreduceRing             -> gloo_amd::HipAllreduceRing<T>
//   gloo::CudaAllreduceLocal            -> gloo_amd::HipAllreduceLocal<T>
//   gloo::ReduceScatterHalvingDoubling  -> gloo_amd::HipReduceScatterHalvingDoubling<T>
//                                          (gloo/reduce_scatter.h:112-117)
//   gloo::allreduce(AllreduceOptions)   -> gloo_amd::allreduce(AllreduceOptions)
//                                          (gloo/allreduce.h:89-193), RING / BCUBE
//   gloo::reduce(ReduceOptions)         -> gloo_amd::reduce(ReduceOptions)
//                                          (gloo/reduce.h:19-112)
// Same constructor shapes (context, ptrs, count[, recvElems][, streams][, fn])
// and run().  Differences, by design: one rank drives one GPU (all `ptrs` of
// a rank live on that rank's device — ranks are processes or threads), the
// workspace is always device memory (inboxes in HBM, chunks moved over
// xGMI), and `count` is computed in size_t internally.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "gloo_amd.h"
#include "gloo_amd/common.h"
#include "gloo_amd/context.h"
#include "gloo_amd/executor.h"

namespace gloo_amd {

// 16-bit float storage types (gloo::float16, gloo/types.h:96; c10::BFloat16).
struct float16 {
  uint16_t x;
};
struct bfloat16 {
  uint16_t x;
};
// OCP FP8 storage types (c10::Float8_e4m3fn, c10::Float8_e5m2).
struct float8_e4m3fn {
  uint8_t x;
};
struct float8_e5m2 {
  uint8_t x;
};

template <typename T> struct DType;
template <> struct DType<int8_t> { static constexpr int value = GLOO_HIP_I8; };
template <> struct DType<uint8_t> { static constexpr int value = GLOO_HIP_U8; };
template <> struct DType<int32_t> { static constexpr int value = GLOO_HIP_I32; };
template <> struct DType<uint32_t> { static constexpr int value = GLOO_HIP_U32; };
template <> struct DType<int64_t> { static constexpr int value = GLOO_HIP_I64; };
template <> struct DType<uint64_t> { static constexpr int value = GLOO_HIP_U64; };
template <> struct DType<float16> { static constexpr int value = GLOO_HIP_F16; };
template <> struct DType<bfloat16> { static constexpr int value = GLOO_HIP_BF16; };
template <> struct DType<float> { static constexpr int value = GLOO_HIP_F32; };
template <> struct DType<double> { static constexpr int value = GLOO_HIP_F64; };
template <> struct DType<float8_e4m3fn> { static constexpr int value = GLOO_HIP_F8E4M3; };
template <> struct DType<float8_e5m2> { static constexpr int value = GLOO_HIP_F8E5M2; };

// gloo::ReductionType values (gloo/algorithm.h:49-57), extended by the
// bitwise ops of the integer types (include/gloo_amd.h gloo_hip_op_t).
enum ReductionType {
  SUM = GLOO_HIP_SUM,
  PRODUCT = GLOO_HIP_PRODUCT,
  MAX = GLOO_HIP_MAX,
  MIN = GLOO_HIP_MIN,
  BAND = GLOO_HIP_BAND,
  BOR = GLOO_HIP_BOR,
  BXOR = GLOO_HIP_BXOR,
};

// Device reduction function: call() enqueues dst = dst op src on `stream`
// (the device overload of CudaReductionFunction<T>::call, gloo/cuda.h:326-333).
template <typename T>
class HipReductionFunction {
 public:
  static const HipReductionFunction<T>* sum;
  static const HipReductionFunction<T>* product;
  static const HipReductionFunction<T>* min;
  static const HipReductionFunction<T>* max;
  // integer T only: call() and the algorithms' constructors refuse them for
  // float16, bfloat16, float, double and the two float8 types
  // (GLOO_HIP_EINVAL_OP)
  static const HipReductionFunction<T>* band;
  static const HipReductionFunction<T>* bor;
  static const HipReductionFunction<T>* bxor;

  explicit HipReductionFunction(ReductionType t) : type_(t) {}
  ReductionType type() const { return type_; }
  void call(T* dst, const T* src, size_t n, hipStream_t stream) const {
    const int rc = gloo_hip_reduce(type_, DType<T>::value, dst, src, n, stream);
    if (rc != GLOO_HIP_OK) throw EnforceNotMet(gloo_hip_last_error());
  }

 private:
  ReductionType type_;
};
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::sum = new HipReductionFunction<T>(SUM);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::product = new HipReductionFunction<T>(PRODUCT);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::min = new HipReductionFunction<T>(MIN);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::max = new HipReductionFunction<T>(MAX);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::band = new HipReductionFunction<T>(BAND);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::bor = new HipReductionFunction<T>(BOR);
template <typename T>
const HipReductionFunction<T>* HipReductionFunction<T>::bxor = new HipReductionFunction<T>(BXOR);

// gloo::Algorithm (gloo/algorithm.h:20-38).
class Algorithm {
 public:
  explicit Algorithm(const std::shared_ptr<Context>& context)
      : context_(context), contextRank_(context->rank), contextSize_(context->size) {}
  virtual ~Algorithm() = default;
  virtual void run() = 0;

 protected:
  std::shared_ptr<Context> context_;
  const int contextRank_;
  const int contextSize_;
};

// Workspaces (gloo/cuda_workspace.h:20-31): where the inboxes live.  The
// reference defaults to the host workspace with CPU reductions; here both
// reduce on the GPU, and the device workspace is the default.
template <typename T>
struct HipDeviceWorkspace {
  static constexpr int kind = GLOO_HIP_WORKSPACE_DEVICE;
};
template <typename T>
struct HipHostWorkspace {
  static constexpr int kind = GLOO_HIP_WORKSPACE_HOST;
};

template <typename T, int ALGO, typename W = HipDeviceWorkspace<T>>
class HipPlanAlgorithm : public Algorithm {
 public:
  HipPlanAlgorithm(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                   const std::vector<int>& recvElems, const std::vector<hipStream_t>& streams,
                   const HipReductionFunction<T>* fn, int algo = ALGO /* a run-time variant of ALGO */)
      : Algorithm(context) {
    // one stream per pointer, or none (gloo/cuda_allreduce_ring_chunked.cc:55-58)
    GLOO_AMD_ENFORCE(streams.empty() || streams.size() == ptrs.size(), "one stream per pointer, or none");
    std::vector<void*> p(ptrs.begin(), ptrs.end());
    exec_ = PlanExecutor::create(context, algo, fn->type(), DType<T>::value, p,
                                           static_cast<size_t>(count), recvElems,
                                           streams.empty() ? nullptr : streams[0], std::vector<void*>{}, 0,
                                           W::kind);
    if (streams.size() > 1) exec_->setStreams(streams);
  }
  void run() override { exec_->run(); }

 protected:
  std::unique_ptr<PlanExecutor> exec_;
};

template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceRingChunked : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_RING_CHUNKED, W> {
 public:
  HipAllreduceRingChunked(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                          const std::vector<hipStream_t>& streams = {},
                          const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_RING_CHUNKED, W>(context, ptrs, count, {}, streams, fn) {}
};

template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceHalvingDoubling : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_HALVING_DOUBLING, W> {
 public:
  HipAllreduceHalvingDoubling(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                              const std::vector<hipStream_t>& streams = {},
                              const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_HALVING_DOUBLING, W>(context, ptrs, count, {}, streams, fn) {}
  // The reference's exact signature (gloo/cuda_allreduce_halving_doubling.h:25-30).
  // pipelineBroadcastAndReduce = true selects
  // GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED: the same exchange and result
  // bytes, with the local fold of a rank's pointers cut into the first send's
  // and the first receive's range (each in one pass with that send / that
  // receive's reduction) and each range broadcast to the other pointers in
  // the pass that takes it out of its inbox.  That order stays
  // on the reference's route at every size; false keeps the default, which
  // runs as the mesh plan at 2-8 ranks.
  HipAllreduceHalvingDoubling(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                              const std::vector<hipStream_t>& streams, bool pipelineBroadcastAndReduce)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_HALVING_DOUBLING, W>(
            context, ptrs, count, {}, streams, HipReductionFunction<T>::sum,
            pipelineBroadcastAndReduce ? GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED : GLOO_HIP_ALGO_HALVING_DOUBLING) {}
};

template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceRing : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_RING, W> {
 public:
  HipAllreduceRing(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                   const std::vector<hipStream_t>& streams = {},
                   const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_RING, W>(context, ptrs, count, {}, streams, fn) {}
};

template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceLocal : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_LOCAL, W> {
 public:
  HipAllreduceLocal(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                    const std::vector<hipStream_t>& streams = {},
                    const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_LOCAL, W>(context, ptrs, count, {}, streams, fn) {}
};

template <typename T, typename W = HipDeviceWorkspace<T>>
class HipReduceScatterHalvingDoubling : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_REDUCE_SCATTER, W> {
 public:
  HipReduceScatterHalvingDoubling(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs,
                                  int count, const std::vector<int>& recvElems,
                                  const std::vector<hipStream_t>& streams = {},
                                  const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_REDUCE_SCATTER, W>(context, ptrs, count, recvElems, streams, fn) {}
};

// AllreduceBcube / CudaAllreduceBcube (gloo/allreduce_bcube.h:265-346,
// gloo/cuda_allreduce_bcube.h:50-58): groups of context->base ranks (0 = 2,
// gloo/cuda_allreduce_bcube.cc:57).
template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceBcube : public HipPlanAlgorithm<T, GLOO_HIP_ALGO_BCUBE, W> {
 public:
  HipAllreduceBcube(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                    const std::vector<hipStream_t>& streams = {},
                    const HipReductionFunction<T>* fn = HipReductionFunction<T>::sum)
      : HipPlanAlgorithm<T, GLOO_HIP_ALGO_BCUBE, W>(context, ptrs, count, {context->base}, streams, fn) {}
};

// CudaAllreduceHalvingDoublingPipelined
// (gloo/cuda_allreduce_halving_doubling_pipelined.h:13-28): halving-doubling
// with pipelineBroadcastAndReduce set (GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED,
// see HipAllreduceHalvingDoubling).
template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllreduceHalvingDoublingPipelined : public HipAllreduceHalvingDoubling<T, W> {
 public:
  HipAllreduceHalvingDoublingPipelined(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs,
                                       int count, const std::vector<hipStream_t>& streams = {})
      : HipAllreduceHalvingDoubling<T, W>(context, ptrs, count, streams, true) {}
};

// New-style function API (gloo/allreduce.h:89-193): options object + free
// function; RING algorithm.  Same setter names as gloo::AllreduceOptions.
class AllreduceOptions {
 public:
  explicit AllreduceOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInputs(std::vector<T*> ptrs, size_t elements) {
    inputs_.assign(ptrs.begin(), ptrs.end());
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setInput(T* ptr, size_t elements) { setInputs(std::vector<T*>{ptr}, elements); }
  template <typename T>
  void setOutputs(std::vector<T*> ptrs, size_t elements) {
    outputs_.assign(ptrs.begin(), ptrs.end());
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) { setOutputs(std::vector<T*>{ptr}, elements); }
  void setReduceFunction(ReductionType op) { op_ = op; }   // built-in ops only on the device
  void setTag(uint32_t tag) { tag_ = tag; }
  void setMaxSegmentSize(size_t bytes) { maxSegmentBytes_ = bytes; }
  void setStream(hipStream_t s) { stream_ = s; }
  // AllreduceOptions::Algorithm (gloo/allreduce.h:38-42)
  enum class Algorithm { UNSPECIFIED = 0, RING = 1, BCUBE = 2 };
  void setAlgorithm(Algorithm a) { algorithm_ = a; }

  std::shared_ptr<Context> context_;
  std::vector<void*> inputs_, outputs_;
  size_t elements_ = 0;
  int dtype_ = GLOO_HIP_F32;
  ReductionType op_ = SUM;
  uint32_t tag_ = 0;
  size_t maxSegmentBytes_ = 0;
  hipStream_t stream_ = nullptr;
  Algorithm algorithm_ = Algorithm::UNSPECIFIED;
};

// One call = one allreduce (builds a PlanExecutor each time; the C-ABI
// gloo_hip_allreduce caches them per option set).
inline void allreduce(const AllreduceOptions& o) {
  if (o.elements_ == 0) return;
  const int algo = o.algorithm_ == AllreduceOptions::Algorithm::BCUBE ? GLOO_HIP_ALGO_ALLREDUCE_BCUBE
                                                                       : GLOO_HIP_ALGO_ALLREDUCE_RING;
  PlanExecutor exec(o.context_, algo, o.op_, o.dtype_, o.outputs_, o.elements_, {}, o.stream_, o.inputs_,
                    o.maxSegmentBytes_);
  exec.run();
}

// gloo::ReduceOptions (gloo/reduce.h:19-110) over device pointers.
class ReduceOptions {
 public:
  explicit ReduceOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, size_t elements) {
    input_ = ptr;
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  void setRoot(int root) { root_ = root; }
  void setReduceFunction(ReductionType op) { op_ = op; }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setMaxSegmentSize(size_t bytes) { maxSegmentBytes_ = bytes; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;
  void* output_ = nullptr;
  size_t elements_ = 0;
  int dtype_ = GLOO_HIP_F32;
  int root_ = -1;
  ReductionType op_ = SUM;
  uint32_t tag_ = 0;
  size_t maxSegmentBytes_ = 0;
  hipStream_t stream_ = nullptr;
};

// gloo::reduce(opts) (gloo/reduce.cc:21-247).
inline void reduce(const ReduceOptions& o) {
  if (o.elements_ == 0) return;
  GLOO_AMD_ENFORCE(o.root_ >= 0 && o.root_ < o.context_->size, "root ", o.root_, " out of range");
  std::vector<void*> ins;
  if (o.input_ && o.input_ != o.output_) ins.push_back(o.input_);
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_REDUCE, o.op_, o.dtype_, {o.output_}, o.elements_, {o.root_},
                    o.stream_, ins, o.maxSegmentBytes_);
  exec.run();
}

// CudaBroadcastOneToAll (gloo/cuda_broadcast_one_to_all.h:20-31): after run()
// every pointer of every rank holds the bytes of the root rank's
// ptrs[rootPointerRank].  GLOO_HIP_ALGO_BROADCAST: the executor gets the
// pointers (and their streams) with the root pointer first, as the C-ABI
// entry points hand them over.  No reduction function: a broadcast has none.
template <typename T, typename W = HipDeviceWorkspace<T>>
class HipBroadcastOneToAll : public Algorithm {
 public:
  HipBroadcastOneToAll(const std::shared_ptr<Context>& context, const std::vector<T*>& ptrs, int count,
                       int rootRank = 0, int rootPointerRank = 0, const std::vector<hipStream_t>& streams = {})
      : Algorithm(context) {
    GLOO_AMD_ENFORCE(rootRank >= 0 && rootRank < context->size, "broadcast: root rank ", rootRank, " outside [0, ",
                     context->size, ")");  // .cc:30-31
    GLOO_AMD_ENFORCE(rootPointerRank >= 0 && rootPointerRank < (int)ptrs.size(), "broadcast: root pointer ",
                     rootPointerRank, " outside [0, ", ptrs.size(), ")");
    GLOO_AMD_ENFORCE(streams.empty() || streams.size() == ptrs.size(), "one stream per pointer, or none");  // .cc:35
    std::vector<void*> p{ptrs[rootPointerRank]};
    std::vector<hipStream_t> s;
    if (!streams.empty()) s.push_back(streams[rootPointerRank]);
    for (size_t i = 0; i < ptrs.size(); i++) {
      if ((int)i == rootPointerRank) continue;
      p.push_back(ptrs[i]);
      if (!streams.empty()) s.push_back(streams[i]);
    }
    exec_ = PlanExecutor::create(context, GLOO_HIP_ALGO_BROADCAST, GLOO_HIP_SUM /* not used */, DType<T>::value, p,
                                 static_cast<size_t>(count), std::vector<int>{rootRank}, s.empty() ? nullptr : s[0],
                                 std::vector<void*>{}, 0, W::kind);
    if (s.size() > 1) exec_->setStreams(s);
  }
  void run() override { exec_->run(); }

 protected:
  std::unique_ptr<PlanExecutor> exec_;
};

// gloo::BroadcastOptions (gloo/broadcast.h:16-87) over device pointers.
class BroadcastOptions {
 public:
  explicit BroadcastOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, size_t elements) {
    input_ = ptr;
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    elements_ = elements;
    dtype_ = DType<T>::value;
  }
  void setRoot(int root) { root_ = root; }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;  // the root's only; null: the output is the input
  void* output_ = nullptr;
  size_t elements_ = 0;
  int dtype_ = GLOO_HIP_U8;
  int root_ = -1;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};

// gloo::broadcast(opts) (gloo/broadcast.cc:16-95).  The reference walks a
// binomial tree over its pairs; here the root sends to every rank itself
// (GLOO_HIP_ALGO_BROADCAST: a root GPU has a direct link to every peer), and
// the bytes that arrive are the same.  A root with a separate input runs with
// the pointers {input, output}: its output is filled in the pass that sends.
inline void broadcast(const BroadcastOptions& o) {
  GLOO_AMD_ENFORCE(o.root_ >= 0 && o.root_ < o.context_->size, "broadcast: root rank ", o.root_, " outside [0, ",
                   o.context_->size, ")");
  if (o.elements_ == 0) return;
  std::vector<void*> ptrs;
  if (o.context_->rank == o.root_ && o.input_ && o.input_ != o.output_) ptrs.push_back(o.input_);
  ptrs.push_back(o.output_);
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_BROADCAST, GLOO_HIP_SUM /* not used */, o.dtype_, ptrs, o.elements_,
                    {o.root_}, o.stream_);
  exec.run();
}

// AllgatherRing (gloo/allgather_ring.h:25-32) over device pointers: after
// run() outPtr holds, for every rank q in order, that rank's inPtrs side by
// side (outPtr[q * inPtrs.size() * count], :19-24).  GLOO_HIP_ALGO_ALLGATHER:
// the blocks go straight from every rank to every peer instead of round the
// reference's ring, the same bytes.  streams: none, one (the plan's), or one
// per pointer of {outPtr, inPtrs...}.
template <typename T, typename W = HipDeviceWorkspace<T>>
class HipAllgatherRing : public Algorithm {
 public:
  HipAllgatherRing(const std::shared_ptr<Context>& context, const std::vector<const T*>& inPtrs, T* outPtr, int count,
                   const std::vector<hipStream_t>& streams = {})
      : Algorithm(context) {
    GLOO_AMD_ENFORCE(!inPtrs.empty(), "allgather: no input");
    GLOO_AMD_ENFORCE(count >= 0, "allgather: negative count ", count);
    GLOO_AMD_ENFORCE(streams.size() <= 1 || streams.size() == inPtrs.size() + 1,
                     "one stream per pointer (the output first), one, or none");
    std::vector<void*> ins;
    for (const T* p : inPtrs) ins.push_back(const_cast<T*>(p));
    exec_ = PlanExecutor::create(context, GLOO_HIP_ALGO_ALLGATHER, GLOO_HIP_SUM /* not used */, DType<T>::value,
                                 std::vector<void*>{outPtr}, static_cast<size_t>(count), std::vector<int>{},
                                 streams.empty() ? nullptr : streams[0], ins, 0, W::kind);
    if (streams.size() > 1) exec_->setStreams(streams);
  }
  void run() override { exec_->run(); }

 protected:
  std::unique_ptr<PlanExecutor> exec_;
};

// gloo::AllgatherOptions (gloo/allgather.h) and gloo::AllgathervOptions
// (gloo/allgatherv.h) over device pointers, in one class: setOutput with one
// element count (the whole output, a multiple of the ranks) is the former,
// with per-rank counts the latter.
class AllgatherOptions {
 public:
  explicit AllgatherOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, size_t elements) {
    input_ = ptr;
    inputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    outputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, std::vector<size_t> counts) {
    output_ = ptr;
    counts_ = std::move(counts);
    dtype_ = DType<T>::value;
  }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;  // null: in place
  void* output_ = nullptr;
  size_t inputElements_ = 0, outputElements_ = 0;
  std::vector<size_t> counts_;  // allgatherv: elements per rank
  int dtype_ = GLOO_HIP_U8;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};
using AllgathervOptions = AllgatherOptions;

// gloo::allgatherv(opts) (gloo/allgatherv.cc:71-140): per-rank counts, the
// output at their prefix offsets (:90-101).
inline void allgatherv(const AllgatherOptions& o) {
  const int P = o.context_->size;
  GLOO_AMD_ENFORCE((int)o.counts_.size() == P, "allgatherv: ", o.counts_.size(), " counts for ", P, " ranks");  // .cc:66
  std::vector<int> counts;
  size_t total = 0;
  for (size_t c : o.counts_) {
    GLOO_AMD_ENFORCE(c <= (size_t)INT32_MAX, "allgatherv: count ", c, " is too large");
    counts.push_back((int)c);
    total += c;
  }
  GLOO_AMD_ENFORCE(!o.input_ || o.inputElements_ == o.counts_[o.context_->rank], "allgatherv: the input has ",
                   o.inputElements_, " elements, this rank's count is ", o.counts_[o.context_->rank]);  // .cc:105
  if (total == 0) return;
  std::vector<void*> ins;
  if (o.input_) ins.push_back(o.input_);
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_ALLGATHER, GLOO_HIP_SUM /* not used */, o.dtype_, {o.output_}, 0, counts,
                    o.stream_, ins);
  exec.run();
}

// gloo::allgather(opts) (gloo/allgather.cc:19-97): the same count on every rank.
inline void allgather(const AllgatherOptions& o) {
  if (!o.counts_.empty()) return allgatherv(o);
  const size_t P = (size_t)o.context_->size;
  if (o.input_)
    GLOO_AMD_ENFORCE(o.outputElements_ == o.inputElements_ * P, "allgather: output of ", o.outputElements_,
                     " elements, ", P, " inputs of ", o.inputElements_);  // .cc:39
  else
    GLOO_AMD_ENFORCE(o.outputElements_ % P == 0, "allgather: output of ", o.outputElements_, " elements over ", P,
                     " ranks");  // .cc:41
  if (o.outputElements_ == 0) return;
  std::vector<void*> ins;
  if (o.input_) ins.push_back(o.input_);
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_ALLGATHER, GLOO_HIP_SUM /* not used */, o.dtype_, {o.output_},
                    o.outputElements_ / P, {}, o.stream_, ins);
  exec.run();
}

// gloo::GatherOptions (gloo/gather.h) and gloo::GathervOptions
// (gloo/gatherv.h) over device pointers, in one class: setOutput with one
// element count (the whole output, a multiple of the ranks) is the former,
// with per-rank counts the latter.  Only the root sets an output.
class GatherOptions {
 public:
  explicit GatherOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, size_t elements) {
    input_ = ptr;
    inputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    outputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, std::vector<size_t> counts) {
    output_ = ptr;
    counts_ = std::move(counts);
    dtype_ = DType<T>::value;
  }
  // gatherv on a rank that is not the root: the counts without an output
  void setCounts(std::vector<size_t> counts) { counts_ = std::move(counts); }
  void setRoot(int root) { root_ = root; }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;
  void* output_ = nullptr;  // the root's; null elsewhere
  size_t inputElements_ = 0, outputElements_ = 0;
  std::vector<size_t> counts_;  // gatherv: elements per rank
  int root_ = -1;
  int dtype_ = GLOO_HIP_U8;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};
using GathervOptions = GatherOptions;

namespace detail {
// A rank without an output hands the executor its input as the one pointer it
// wants; no step of that rank's plan reads or writes output 0.
inline void runGather(const GatherOptions& o, size_t count, const std::vector<int>& recvElems) {
  const bool root = o.context_->rank == o.root_;
  GLOO_AMD_ENFORCE(!root || o.output_, "gather: the root has no output");
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_GATHER, GLOO_HIP_SUM /* not used */, o.dtype_,
                    {root ? o.output_ : o.input_}, count, recvElems, o.stream_, {o.input_});
  exec.run();
}
}  // namespace detail

// gloo::gatherv(opts) (gloo/gatherv.cc:71-107): per-rank counts, the root's
// output at their prefix offsets (:82-96).
inline void gatherv(const GatherOptions& o) {
  const int P = o.context_->size;
  GLOO_AMD_ENFORCE(o.root_ >= 0 && o.root_ < P, "gatherv: root rank ", o.root_, " outside [0, ", P, ")");
  GLOO_AMD_ENFORCE((int)o.counts_.size() == P, "gatherv: ", o.counts_.size(), " counts for ", P, " ranks");  // .cc:66
  std::vector<int> re{o.root_};
  size_t total = 0;
  for (size_t c : o.counts_) {
    GLOO_AMD_ENFORCE(c <= (size_t)INT32_MAX, "gatherv: count ", c, " is too large");
    re.push_back((int)c);
    total += c;
  }
  GLOO_AMD_ENFORCE(o.inputElements_ >= o.counts_[o.context_->rank], "gatherv: the input has ", o.inputElements_,
                   " elements, this rank's count is ", o.counts_[o.context_->rank]);  // .cc:90, :103
  if (total == 0) return;
  detail::runGather(o, 0, re);
}

// gloo::gather(opts) (gloo/gather.cc): the same count on every rank.
inline void gather(const GatherOptions& o) {
  if (!o.counts_.empty()) return gatherv(o);
  const size_t P = (size_t)o.context_->size;
  GLOO_AMD_ENFORCE(o.root_ >= 0 && o.root_ < (int)P, "gather: root rank ", o.root_, " outside [0, ", P, ")");  // .cc:26
  if (o.context_->rank == o.root_)
    GLOO_AMD_ENFORCE(o.outputElements_ == o.inputElements_ * P, "gather: output of ", o.outputElements_,
                     " elements, ", P, " inputs of ", o.inputElements_);  // .cc:32
  if (o.inputElements_ == 0) return;
  detail::runGather(o, o.inputElements_, {o.root_});
}

// gloo::ScatterOptions (gloo/scatter.h) over device pointers: the root sets
// one input per rank (separate buffers, or slices of one allocation), every
// rank one output of the same element count.
class ScatterOptions {
 public:
  explicit ScatterOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInputs(std::vector<T*> ptrs, size_t elements) {
    inputs_.assign(ptrs.begin(), ptrs.end());
    inputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    outputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  void setRoot(int root) { root_ = root; }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  std::vector<void*> inputs_;  // the root's; empty elsewhere
  void* output_ = nullptr;
  size_t inputElements_ = 0, outputElements_ = 0;
  int root_ = -1;
  int dtype_ = GLOO_HIP_U8;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};

// gloo::scatter(opts) (gloo/scatter.cc:19-61).
inline void scatter(const ScatterOptions& o) {
  const int P = o.context_->size;
  GLOO_AMD_ENFORCE(o.root_ >= 0 && o.root_ < P, "scatter: root rank ", o.root_, " outside [0, ", P, ")");  // .cc:27
  GLOO_AMD_ENFORCE(o.output_ || o.outputElements_ == 0, "scatter: no output");                             // .cc:28
  const bool root = o.context_->rank == o.root_;
  if (root) {
    GLOO_AMD_ENFORCE((int)o.inputs_.size() == P, "scatter: ", o.inputs_.size(), " inputs for ", P, " ranks");  // .cc:31
    GLOO_AMD_ENFORCE(o.inputElements_ == o.outputElements_, "scatter: inputs of ", o.inputElements_,
                     " elements, an output of ", o.outputElements_);  // .cc:34
  }
  if (o.outputElements_ == 0) return;
  PlanExecutor exec(o.context_, GLOO_HIP_ALGO_SCATTER, GLOO_HIP_SUM /* not used */, o.dtype_, {o.output_},
                    o.outputElements_, {o.root_}, o.stream_, root ? o.inputs_ : std::vector<void*>{});
  exec.run();
}

// gloo::AlltoallOptions (gloo/alltoall.h) over device pointers: one input and
// one output of the same element count, a multiple of the ranks; block q of
// the input goes to rank q.  Input and output may share no byte.
class AlltoallOptions {
 public:
  explicit AlltoallOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, size_t elements) {
    input_ = ptr;
    inputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, size_t elements) {
    output_ = ptr;
    outputElements_ = elements;
    dtype_ = DType<T>::value;
  }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;
  void* output_ = nullptr;
  size_t inputElements_ = 0, outputElements_ = 0;
  int dtype_ = GLOO_HIP_U8;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};

// gloo::AlltoallvOptions (gloo/alltoallv.h) over device pointers: this rank
// sends inCounts[q] elements to rank q and receives outCounts[q] from it, at
// the prefix offsets (alltoallv.cc:19-31).  setMatrix (optional): the whole
// P x P matrix, [q * P + r] the elements from rank q to rank r, the same on
// every rank; alltoallv then skips its host exchange of the counts.
class AlltoallvOptions {
 public:
  explicit AlltoallvOptions(const std::shared_ptr<Context>& context) : context_(context) {}
  template <typename T>
  void setInput(T* ptr, std::vector<size_t> counts) {
    input_ = ptr;
    inCounts_ = std::move(counts);
    dtype_ = DType<T>::value;
  }
  template <typename T>
  void setOutput(T* ptr, std::vector<size_t> counts) {
    output_ = ptr;
    outCounts_ = std::move(counts);
    dtype_ = DType<T>::value;
  }
  void setMatrix(std::vector<int> matrix) { matrix_ = std::move(matrix); }
  void setTag(uint32_t tag) { tag_ = tag; }
  void setStream(hipStream_t s) { stream_ = s; }

  std::shared_ptr<Context> context_;
  void* input_ = nullptr;
  void* output_ = nullptr;
  std::vector<size_t> inCounts_, outCounts_;
  std::vector<int> matrix_;
  int dtype_ = GLOO_HIP_U8;
  uint32_t tag_ = 0;
  hipStream_t stream_ = nullptr;
};

namespace detail {
// `matrix` empty: the even form of `count` elements per block.  in / out: the
// elements this rank sends and receives (for the buffers' overlap check).
inline void runAlltoall(const std::shared_ptr<Context>& ctx, int dtype, void* input, void* output, size_t count,
                        const std::vector<int>& matrix, size_t in, size_t out, hipStream_t stream) {
  const size_t es = gloo_hip_dtype_size(dtype);
  GLOO_AMD_ENFORCE(es > 0, "alltoall: unknown dtype ", dtype);
  const char* a = static_cast<const char*>(input);
  const char* b = static_cast<const char*>(output);
  GLOO_AMD_ENFORCE(in == 0 || out == 0 || a + in * es <= b || b + out * es <= a,
                   "alltoall: input and output overlap (there is no in-place form)");
  PlanExecutor exec(ctx, GLOO_HIP_ALGO_ALLTOALL, GLOO_HIP_SUM /* not used */, dtype, {output}, count, matrix, stream,
                    {input});
  exec.run();
}
}  // namespace detail

// gloo::alltoall(opts) (gloo/alltoall.cc:19-72).
inline void alltoall(const AlltoallOptions& o) {
  const size_t P = (size_t)o.context_->size;
  GLOO_AMD_ENFORCE(o.inputElements_ % P == 0, "alltoall: an input of ", o.inputElements_, " elements for ", P,
                   " ranks");  // .cc:29
  GLOO_AMD_ENFORCE(o.inputElements_ == o.outputElements_, "alltoall: an input of ", o.inputElements_,
                   " elements, an output of ", o.outputElements_);  // .cc:30
  if (o.inputElements_ == 0) return;
  GLOO_AMD_ENFORCE(o.input_ && o.output_, "alltoall: no input or no output");  // .cc:27-28
  detail::runAlltoall(o.context_, o.dtype_, o.input_, o.output_, o.inputElements_ / P, {}, o.inputElements_,
                      o.outputElements_, o.stream_);
}

// gloo::alltoallv(opts) (gloo/alltoallv.cc:117-170).  Without setMatrix the
// ranks exchange their lists once on the host (every call), every rank
// assembles the matrix from the same records and checks every pair, so a
// mismatch raises on every rank alike before any byte moves.
inline void alltoallv(const AlltoallvOptions& o) {
  const int P = o.context_->size, me = o.context_->rank;
  GLOO_AMD_ENFORCE((int)o.inCounts_.size() == P, "alltoallv: ", o.inCounts_.size(), " in_counts for ", P, " ranks");  // .cc:52
  GLOO_AMD_ENFORCE((int)o.outCounts_.size() == P, "alltoallv: ", o.outCounts_.size(), " out_counts for ", P,
                   " ranks");  // .cc:89
  std::vector<int> mine;
  size_t in = 0, out = 0;
  for (int k = 0; k < 2 * P; k++) {
    const size_t c = k < P ? o.inCounts_[k] : o.outCounts_[k - P];
    GLOO_AMD_ENFORCE(c <= (size_t)INT32_MAX, "alltoallv: count ", c, " is too large");
    mine.push_back((int)c);
    (k < P ? in : out) += c;
  }
  GLOO_AMD_ENFORCE(mine[me] == mine[P + me], "alltoallv: rank ", me, "'s own block has in_count ", mine[me],
                   " but out_count ", mine[P + me]);  // .cc:138
  GLOO_AMD_ENFORCE(o.input_ || in == 0, "alltoallv: no input");    // .cc:131
  GLOO_AMD_ENFORCE(o.output_ || out == 0, "alltoallv: no output");  // .cc:132
  std::vector<int> m = o.matrix_;
  if (m.empty()) {
    std::vector<char> blob(mine.size() * sizeof(int));
    std::memcpy(blob.data(), mine.data(), blob.size());
    const auto all = o.context_->allgather("alltoall/counts", blob);
    m.assign((size_t)P * P, 0);
    std::vector<int> expect((size_t)P * P, 0);  // [r * P + q]: what rank r expects from rank q
    for (int q = 0; q < P; q++) {
      GLOO_AMD_ENFORCE(all.at(q).size() == blob.size(), "alltoallv: bad count record from rank ", q);
      std::memcpy(&m[(size_t)q * P], all[q].data(), P * sizeof(int));
      std::memcpy(&expect[(size_t)q * P], all[q].data() + P * sizeof(int), P * sizeof(int));
    }
    for (int q = 0; q < P; q++)
      for (int r = 0; r < P; r++)
        GLOO_AMD_ENFORCE(m[(size_t)q * P + r] == expect[(size_t)r * P + q], "alltoallv: rank ", q, " sends ",
                         m[(size_t)q * P + r], " elements to rank ", r, " but rank ", r, " expects ",
                         expect[(size_t)r * P + q], " from rank ", q);
  } else {
    const std::vector<int> want = alltoallLists(me, P, m);
    GLOO_AMD_ENFORCE(want == mine, "alltoallv: the matrix's row and column ", me, " differ from this rank's counts");
  }
  bool any = false;
  for (int v : m) any = any || v != 0;
  if (!any) return;
  detail::runAlltoall(o.context_, o.dtype_, o.input_, o.output_, 0, m, in, out, o.stream_);
}

}  // namespace gloo_amd
