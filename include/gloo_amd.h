/*
 * gloo_amd.h — C-ABI of the MI355X-native Gloo per-chunk reduction.
 *
 * This is the drop-in boundary for Gloo's hot path: the element-wise
 * sum / product / max / min that every allreduce / reduce-scatter schedule
 * applies to each arriving chunk.  Plain pointers, sizes and integer enums
 * only; no HIP, torch or C++ types cross this boundary, and no C++ exception
 * ever escapes it (every entry point returns a status code).
 *
 * Reference interfaces replaced (paths relative to facebookincubator/gloo):
 *   gloo_hip_reduce   <- gloo::cudaSum/cudaProduct/cudaMax/cudaMin<T>
 *                        (gloo/cuda.h:274-284, kernels gloo/cuda.cu:283-401),
 *                        i.e. the device overload of
 *                        CudaReductionFunction<T>::call (gloo/cuda.h:326-333):
 *                        dst[i] = dst[i] (op) src[i], async on `stream`.
 *   gloo_hip_reduce3  <- the 3-operand host form gloo::sum/product/max/min<T>
 *                        (void* c, const void* a, const void* b, size_t n)
 *                        (gloo/math.h:15-73), which is also the new-style
 *                        reduce `Func` signature (gloo/allreduce.h:36).
 *   gloo_hip_op_t     <- gloo::ReductionType (gloo/algorithm.h:49-57).
 *   gloo_hip_dtype_t  <- the union of the instantiation lists of
 *                        gloo/cuda.cu:265-272,394-401 and
 *                        gloo/test/math_test.cc:23-32.
 *
 * Semantics (bit-exact with gloo/math.h evaluated in the listed order):
 *   SUM      c = a + b      (integers wrap modulo 2^bits)
 *   PRODUCT  c = a * b      (integers wrap modulo 2^bits)
 *   MAX      c = (a < b) ? b : a      == std::max(a, b)  (gloo/math.h:51)
 *   MIN      c = (b < a) ? b : a      == std::min(a, b)  (gloo/math.h:66)
 *   For the in-place form a := dst, b := src, so a NaN already in dst is kept
 *   and a NaN arriving in src is ignored by MAX/MIN, exactly as
 *   `if (src op dst) dst = src` in gloo/cuda.cu:337-355.
 *   f16 / bf16: both operands widened to f32, op in f32, rounded back to
 *   nearest-even (gloo/math.cc:17-97 F16C path; c10::BFloat16 for bf16);
 *   MAX/MIN compare in f32 and copy the raw 16-bit operand.
 *
 * Buffers may start at any element-aligned address and `c` may alias `a`
 * (the in-place call).  n may be 0.  The functions never allocate, free or
 * synchronise: they enqueue one kernel on `stream` and return.
 */
#ifndef GLOO_AMD_H_
#define GLOO_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SUM..MIN mirror gloo::ReductionType (gloo/algorithm.h:49-57).  BAND, BOR
 * and BXOR extend it; they do not mirror it (the reference's enum stops at
 * MIN).  Their model is the BAND / BOR / BXOR of PyTorch's ReduceOp, which
 * its Gloo process group builds from custom functions:
 *   BAND  c = a & b      BOR  c = a | b      BXOR  c = a ^ b
 * on the element's bits, exact in every schedule and fold order.  They are
 * defined for I8, U8, I32, U32, I64, U64; with F16, BF16, F32, F64, F8E4M3
 * or F8E5M2 every
 * entry point that takes an op returns GLOO_HIP_EINVAL_OP (the message names
 * the op and the dtype) before it looks at n or at a pointer, and the
 * collective entry points (gloo_hip_algorithm_create*, gloo_hip_allreduce,
 * gloo_hip_reduce_to_root) before any exchange with a peer, so every rank
 * fails locally.  They take every kernel path the arithmetic ops take.
 * Codes 8..999 are invalid. */
typedef enum {
  GLOO_HIP_SUM = 1,
  GLOO_HIP_PRODUCT = 2,
  GLOO_HIP_MAX = 3,
  GLOO_HIP_MIN = 4,
  GLOO_HIP_BAND = 5,
  GLOO_HIP_BOR = 6,
  GLOO_HIP_BXOR = 7,
} gloo_hip_op_t;

typedef enum {
  GLOO_HIP_I8 = 0,
  GLOO_HIP_U8 = 1,
  GLOO_HIP_I32 = 2,
  GLOO_HIP_U32 = 3,
  GLOO_HIP_I64 = 4,
  GLOO_HIP_U64 = 5,
  GLOO_HIP_F16 = 6,
  GLOO_HIP_BF16 = 7,
  GLOO_HIP_F32 = 8,
  GLOO_HIP_F64 = 9,
  GLOO_HIP_F8E4M3 = 10, /* OCP e4m3fn, torch.float8_e4m3fn */
  GLOO_HIP_F8E5M2 = 11, /* OCP e5m2, torch.float8_e5m2 */
  GLOO_HIP_NUM_DTYPES = 12,
} gloo_hip_dtype_t;

/* F8E4M3 and F8E5M2 (1 byte each; the FNUZ variants are not part of this)
 * extend the reference's type list; they do not mirror it.  Their model is
 * c10::Float8_e4m3fn / c10::Float8_e5m2, i.e. torch on the CPU, as
 * c10::BFloat16 is for BF16.
 *   e4m3fn: no infinity, NaN is 0x7F / 0xFF, the largest finite value is 448.
 *   e5m2:   infinity is 0x7C / 0xFC, NaNs are 0x7D..0x7F / 0xFD..0xFF.
 *   SUM, PRODUCT: both operands widened to f32 (exact), one IEEE f32 op,
 *     rounded to nearest even back to the format with c10's overflow rule,
 *     which does not saturate: e4m3fn, a finite r with |r| > 464 becomes the
 *     NaN with r's sign (0x7F / 0xFF; 464 itself rounds to 448 = 0x7E); e5m2,
 *     |r| >= 61440 becomes the infinity with r's sign.
 *     Where the f32 result r is itself a NaN (a NaN operand, inf - inf,
 *     0 * inf) the stored byte is 0x7F in both formats.  torch's own byte
 *     there carries the sign of whichever operand its x86 vector code picked
 *     (the second for +, the first for *, negative for an invalid operation):
 *     an artefact of one build, not a rule; the same reasoning as BF16's
 *     canonical 0x7FC0.
 *   MAX, MIN: (a < b) ? b : a and (b < a) ? b : a compared in f32, the raw
 *     operand byte copied, as for F16 / BF16: a NaN in a stays, a NaN in b
 *     is ignored, max(+0, -0) is +0.
 *   Multi-source folds round to the format after every op (left to right, or
 *     as a tree where the schedule folds as one), so a k-source fold is
 *     byte-identical to k - 1 two-operand calls and every schedule agrees
 *     with its mesh form.
 *   BAND / BOR / BXOR are refused (GLOO_HIP_EINVAL_OP) as for the other
 *     floating dtypes; registered custom ops take them like any known dtype. */

/* Status codes: 0 = success, > 0 = a hipError_t, < 0 = argument error. */
#define GLOO_HIP_OK 0
#define GLOO_HIP_EINVAL_OP (-1)
#define GLOO_HIP_EINVAL_DTYPE (-2)
#define GLOO_HIP_EINVAL_PTR (-3)
#define GLOO_HIP_EINVAL_ARG (-4)
#define GLOO_HIP_EIO (-5) /* a peer did not answer within the context timeout (gloo::IoException) */

/* A hipStream_t passed as an opaque pointer (NULL = the default stream). */
typedef void* gloo_hip_stream_t;

/* In-place per-chunk reduction: dst[i] = dst[i] (op) src[i], i < n.
 * Replaces cudaSum/cudaProduct/cudaMax/cudaMin<T> (gloo/cuda.cu:283-401). */
int gloo_hip_reduce(int op, int dtype, void* dst, const void* src, size_t n,
                    gloo_hip_stream_t stream);

/* Three-operand form: c[i] = a[i] (op) b[i]; c may alias a or b.
 * Replaces gloo::sum/product/max/min<T>(c, a, b, n) (gloo/math.h:15-73). */
int gloo_hip_reduce3(int op, int dtype, void* c, const void* a, const void* b,
                     size_t n, gloo_hip_stream_t stream);

/* Multi-source local reduction: dst[i] = (((srcs[0][i] op srcs[1][i]) op
 * srcs[2][i]) ... op srcs[k-1][i]), left to right, in ONE pass over HBM.
 * dst may alias srcs[0].  This is the fused form of the reference's local
 * multi-pointer loop `for i in 1..k: fn(ptrs[0], ptrs[i], count)`
 * (gloo/allreduce_local.cc:28-33, gloo/allreduce_ring_chunked.h:89-91),
 * bit-identical to it because the association order is the same.
 * k must be in [1, GLOO_HIP_MAX_SRCS]; srcs is a HOST array of k device
 * pointers. */
#define GLOO_HIP_MAX_SRCS 8
int gloo_hip_reduce_multi(int op, int dtype, void* dst,
                          const void* const* srcs, int k, size_t n,
                          gloo_hip_stream_t stream);

/* Host-staged chunk reduction: host_dst[i] = host_dst[i] (op) host_src[i]
 * for a chunk that starts and ends in (pinned) host memory — a transport's
 * receive buffer — computed by the HIP kernel through device scratch
 * dev_dst / dev_src (n elements each, caller-owned).  piece_elems = 0:
 * when both host buffers are pinned AND mapped (hipHostGetDevicePointer
 * succeeds), one kernel reduces them in place over PCIe (zero-copy, the
 * scratch is unused, the fastest way measured); otherwise, and for any
 * piece_elems > 0, the chunk is staged through the scratch in pieces of
 * max(piece_elems, 16 MiB) elements' bytes: H2D of piece k+1, the kernel of
 * piece k and D2H of piece k-1 overlap on per-thread copy streams (smaller
 * pieces measured slower than one pass); a chunk of at most one piece goes
 * H2D, kernel, D2H in one pass on `stream`.  Ordered after the work already
 * on `stream`; the host result is complete once `stream` has drained.  The device side of the reference's CudaLocalHostReduce
 * (gloo/cuda_collectives_host.h:22-136), with the reduction on the GPU. */
int gloo_hip_reduce_staged(int op, int dtype, void* host_dst, const void* host_src, size_t n,
                           void* dev_dst, void* dev_src, size_t piece_elems, gloo_hip_stream_t stream);

/* Custom reductions: gloo::ReductionType::CUSTOM (= 1000) with a user
 * function (gloo/algorithm.h:49-95) and the new-style reduce `Func`
 * (gloo/allreduce.h:36), on device memory.  The function enqueues
 * c[i] = a[i] (op) b[i], i < n, on `stream` (c may alias a; it must not
 * allocate, free or synchronise — it may be captured into a hipGraph).
 * gloo_hip_register_op returns an op code >= GLOO_HIP_CUSTOM that every
 * entry point taking an `op` accepts.  Algorithms with a custom op run the
 * reference's own exchange routes (no mesh plans), call the function for
 * every REDUCE and FOLD step (a k-source fold as k - 1 calls, left to
 * right), and never use the fused or interpreted kernels. */
#define GLOO_HIP_CUSTOM 1000
typedef void (*gloo_hip_custom_fn)(void* user, void* c, const void* a, const void* b, size_t n,
                                   gloo_hip_stream_t stream);
int gloo_hip_register_op(gloo_hip_custom_fn fn, void* user, int* op_out);

/* The kernel copy engine of a plan's SEND steps (copy_signal_kernel
 * without a flag): dst[0, bytes) = src[0, bytes) in 16-byte packets at any
 * relative misalignment, with `blocks` workgroups (0: one per 16 KiB tile,
 * capped at 1024).  Exported for measurement tools (blit vs kernel copies;
 * DESIGN.md §4) and callers that want a copy with no DMA-engine dependence. */
int gloo_hip_copy_kernel(void* dst, const void* src, size_t bytes, unsigned blocks, gloo_hip_stream_t stream);

/* (new, measurement) Up to 8 such copies in ONE launch, all in flight together
 * — the mesh schedules' sends to every peer (one xGMI link each): copy j gets
 * at most `blocks` workgroups (0: 64, the executor's per-peer default). */
int gloo_hip_copy_kernel_multi(void* const* dsts, const void* const* srcs, const size_t* bytes, int n,
                               unsigned blocks, gloo_hip_stream_t stream);

/* (new, measurement) One source to up to 8 local destinations in ONE pass:
 * each 16 KiB tile of src is loaded once and stored to every dsts[j] at that
 * destination's own 16-byte misalignment (the root's fan-out of
 * GLOO_HIP_ALGO_BROADCAST without its flags; tools/bcast_bench.py compares it
 * with gloo_hip_copy_kernel_multi, which reads the source once per copy).
 * blocks: workgroups (0: one per tile, capped at 256). */
int gloo_hip_fanout_kernel(void* const* dsts, int n, const void* src, size_t bytes, unsigned blocks,
                           gloo_hip_stream_t stream);

/* (new, tests and measurement) k <= 8 sources of `bytes` bytes each to up to
 * 8 local destinations in ONE pass: every dsts[j] receives the sources
 * concatenated (source i at dsts[j] + i * bytes), each 16 KiB source tile
 * loaded once and stored to every destination at that (source, destination)
 * pair's own 16-byte misalignment (the sender's pass of
 * GLOO_HIP_ALGO_ALLGATHER without its flags; tools/allgather_bench.py).  With
 * k = 1 it makes the stores of gloo_hip_fanout_kernel.  blocks: workgroups
 * (0: one per tile, capped at 256). */
int gloo_hip_gather_fanout_kernel(void* const* dsts, int n, const void* const* srcs, int k, size_t bytes,
                                  unsigned blocks, gloo_hip_stream_t stream);

/* (new, tests) The k-source fold kernels as a plan's executor launches them,
 * without a peer: dst[i] = fold of srcs[0..k)[i], i < n, in `mode`'s order
 * (0 left: acc = acc op s_j; 1 reverse: acc = s_j op acc; 2 balanced tree over
 * the sources in order, k a power of two).  nfwd = 0: the FOLD step
 * (reduce_multi_vec_kernel with plain stores).  nfwd in 1..8: the fold +
 * forward (fold_send_kernel): every result element also goes to fwd[r] (any
 * element-aligned address, its own 16-byte misalignment), and the launch's last
 * workgroup stores fwd_values[r] to every non-null fwd_flags[r] and leaves
 * *ticket (a zeroed device word, needed with any flag) at 0 again.  fwd[r] ==
 * NULL with a flag is a credit: the flag alone.  fwd, fwd_flags and fwd_values
 * may each be NULL (all entries NULL / 0).  dst may alias a source.  Built-in
 * ops only.  Every argument is checked before any GPU call; n == 0 launches
 * nothing.  Nothing in it waits on a flag (tests/test_fold_kernel_gpu.py). */
int gloo_hip_fold_kernel(int op, int dtype, void* dst, const void* const* srcs, int k, size_t n, int mode,
                         void* const* fwd, uint64_t* const* fwd_flags, const uint64_t* fwd_values, int nfwd,
                         unsigned* ticket, gloo_hip_stream_t stream);

/* 1 when the kernels implement `op` on `dtype`: a built-in op on a dtype it
 * is defined for (SUM..MIN on all twelve, BAND / BOR / BXOR on the six integer
 * dtypes) or a registered custom op on a known dtype; 0 otherwise.  Never
 * touches the GPU. */
int gloo_hip_op_supported(int op, int dtype);

/* Size in bytes of one element of `dtype`, or 0 when dtype is unknown. */
size_t gloo_hip_dtype_size(int dtype);

/* Human-readable text of the last error raised on the calling thread. */
const char* gloo_hip_last_error(void);

/* Library version, "MAJOR.MINOR.PATCH". */
const char* gloo_hip_version(void);

/* Tuning knob for the measurement harness: select the kernel variant used by
 * the fp32 SUM path.  0 = default (tuned).  Returns the previous value. */
int gloo_hip_set_variant(int variant);

/* ------------------------------------------------------------------------
 * Schedules.  Each of the reference's reducing algorithms is restated as a
 * per-rank PLAN: the exact sequence of one-sided sends, receive waits,
 * reductions, copies and notifications its run() performs (same offsets,
 * lengths, peers, order — hence the same association order and bit-identical
 * results).  The HIP executor (gloo_hip_algo_*) walks a plan over device
 * memory; tests simulate all ranks' plans on the CPU against golden vectors.
 * ---------------------------------------------------------------------- */
typedef enum {
  GLOO_HIP_ALGO_RING_CHUNKED = 0,     /* gloo/allreduce_ring_chunked.h        */
  GLOO_HIP_ALGO_HALVING_DOUBLING = 1, /* gloo/allreduce_halving_doubling.h    */
  GLOO_HIP_ALGO_RING = 2,             /* gloo/allreduce_ring.h                */
  GLOO_HIP_ALGO_LOCAL = 3,            /* gloo/allreduce_local.{h,cc}          */
  GLOO_HIP_ALGO_REDUCE_SCATTER = 4,   /* gloo/reduce_scatter.h (HD)           */
  GLOO_HIP_ALGO_ALLREDUCE_RING = 5,   /* new-style gloo::allreduce(opts), RING
                                         (gloo/allreduce.cc:147-392)          */
  /* AllreduceRingChunked's RESULT with mesh data movement: each chunk pair
   * goes straight from every rank to the rank where the ring finishes it,
   * over all xGMI links at once, and is folded there in the ring's exact
   * association and operand order (bit-identical), then sent to every rank.
   * 2 <= size <= GLOO_HIP_MAX_SRCS.  RING_CHUNKED executes as this plan in
   * that range unless GLOO_AMD_MESH=0. */
  GLOO_HIP_ALGO_RING_CHUNKED_MESH = 6,
  GLOO_HIP_ALGO_ALLREDUCE_BCUBE = 7,  /* new-style gloo::allreduce(opts), BCUBE
                                         (gloo/allreduce.cc:397-669)          */
  GLOO_HIP_ALGO_REDUCE = 8,           /* new-style gloo::reduce(opts)
                                         (gloo/reduce.cc:21-247); the root is
                                         recv_elems[0] in gloo_hip_plan*      */
  /* AllreduceRingChunked's own ring route (its hops, association and bytes)
   * with three inboxes per channel, so that each round's reduce and the send
   * of its result run as one pass (plan.cc planRingChunkedPipe).  RING_CHUNKED
   * executes as this plan wherever it keeps the ring route (GLOO_AMD_MESH=0
   * or size > GLOO_HIP_MAX_SRCS) with a built-in op; a custom op keeps the
   * literal ring order. */
  GLOO_HIP_ALGO_RING_CHUNKED_PIPE = 9,
  /* AllreduceBcube (gloo/allreduce_bcube.h) and its GPU twin
   * CudaAllreduceBcube (gloo/cuda_allreduce_bcube.{h,cc}): groups of `base`
   * ranks, log_base(P) reduce-scatter steps and the all-gather back.  The
   * base (gloo::Context::base, gloo/context.h:28-33; 0 or absent = 2) is
   * recv_elems[0] in gloo_hip_plan* and gloo_hip_algorithm_create.  For
   * 2 <= size <= 8 it executes as its derived mesh plan (| GLOO_HIP_ALGO_MESH)
   * wherever every rank ends with the same expression trees (P a power of
   * the base, counts of about P and more), else on the reference's route. */
  GLOO_HIP_ALGO_BCUBE = 10,
  /* CudaAllreduceHalvingDoubling with pipelineBroadcastAndReduce = true
   * (gloo/cuda_allreduce_halving_doubling.cc:246-455, pipelined_): the
   * halving-doubling exchange unchanged, with the local multi-pointer steps
   * cut per range.  The first send's range is reduced before it is sent and
   * the first receive's range while that message is in flight; each range is
   * broadcast to the other pointers as the all-gather delivers it, with no
   * whole-range pass at either end.  Identical to HALVING_DOUBLING's plan for
   * one pointer, one rank, no elements and a rank in a binary block of one.
   * It is an order of the reference's route: there is no mesh form
   * (| GLOO_HIP_ALGO_MESH is refused) and the executor never promotes it, so
   * at 2-8 ranks plain HALVING_DOUBLING (mesh) is the faster choice where
   * the flag is not wanted.  The executor runs each local step and its
   * neighbour in one pass (local fold + first send, local fold + first
   * receive-reduce, receive + broadcast; executor_run.cc). */
  GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED = 11,
  /* CudaBroadcastOneToAll (gloo/cuda_broadcast_one_to_all.{h,cc}): after a
   * run every pointer of every rank holds, byte for byte, what the root
   * rank's root pointer held.  Not a reduction:
   *   op     is NOT USED.  Any value is accepted (0, a pair the reductions
   *          refuse such as BXOR with F32): no refusal looks at it.
   *   dtype  gives the element size only; all twelve are valid.
   *   recv_elems, when not NULL, points to TWO ints {root rank, root pointer
   *          rank}; NULL means {0, 0} (the front ends pad an absent second
   *          entry with 0).  This is how GLOO_HIP_ALGO_REDUCE passes its root.
   *          A root outside [0, size), a root pointer outside [0, nptrs) and
   *          | GLOO_HIP_ALGO_MESH are refused with GLOO_HIP_EINVAL_ARG; the
   *          last-error text names the value.
   * Order (the reference's, .cc:87-156).  Root: for each peer in ascending
   * rank WAIT_NOTIFY (its clear-to-send) then SEND of the whole range; then
   * LOCAL_BCAST when nptrs > 1; then WAIT_SEND per peer.  Non-root: DECL_RECV,
   * NOTIFY (clear-to-send), WAIT_RECV, COPY inbox -> pointer 0, LOCAL_BCAST
   * when nptrs > 1.  In a plan pointer 0 IS the root pointer: the algorithm
   * entry points hand the executor the pointer list with it first.  One rank:
   * the LOCAL_BCAST alone; count 0, or one rank with one pointer: no steps.
   * The clear-to-send orders the root's next send after the receiver's copy
   * out of its inbox, so runs need no barrier.  The executor never promotes
   * this plan to another route; it runs the root's sends and local broadcast
   * as one pass over the source (reduce.hip fanout_kernel) and the receiver's
   * COPY + LOCAL_BCAST as one pass over the inbox. */
  GLOO_HIP_ALGO_BROADCAST = 12,
  /* AllgatherRing (gloo/allgather_ring.h), gloo::allgather and
   * gloo::allgatherv (gloo/allgather.cc, gloo/allgatherv.cc): rank r
   * contributes k >= 1 inputs of counts[r] elements each; block r is those
   * inputs concatenated (k * counts[r] elements), and after a run every
   * rank's ONE output holds block 0, block 1, ... block P-1 back to back
   * (allgather_ring.h:19-24: outPtr[rank * ninputs * count] consecutively;
   * allgatherv.cc:90-101: prefix offsets).  Not a reduction:
   *   op     is NOT USED; any value is accepted, as for the broadcast.
   *   dtype  gives the element size only; all twelve are valid.
   *   ptrs   at gloo_hip_algorithm_create*: {out, in_0 ... in_{k-1}}, nptrs =
   *          k + 1; nptrs = 1 is the in-place form (allgather.cc:47-54, in ==
   *          nullptr): the rank's own block already sits in its slot of out.
   *   count  elements per input; recv_elems NULL there.  In gloo_hip_plan_ex:
   *          ninputs = k (0: in place, and then k is 1), noutputs = 1,
   *          recv_elems = `size` per-rank counts or NULL for `count`
   *          everywhere.  A negative count and | GLOO_HIP_ALGO_MESH are
   *          refused with GLOO_HIP_EINVAL_ARG; the last-error text names the
   *          value.
   * Route: direct exchange.  The reference passes blocks round a ring in
   * P - 1 dependent hops (allgather_ring.h:70-91, allgather.cc:69-96,
   * allgatherv.cc:119-139); a GPU has a link to every peer, so every rank
   * sends its block straight to every peer and the bytes that arrive are the
   * same (the argument that made the broadcast one-to-all).
   * Arena: laid out like the output, k * sum(counts) elements; the inbox for
   * peer q is arena[offset(q), +k * counts[q]) on GLOO_HIP_SLOT_DATA0.
   * Order, for P > 1 and a total > 0: DECL_RECVs; LOCAL_GATHER into the own
   * slot (the reference's copy of the inputs, allgather_ring.h:65-68; absent
   * in place); for each peer rank+1, rank+2, ...: WAIT_NOTIFY |
   * GLOO_HIP_PREV_RUN on GLOO_HIP_SLOT_NOTIFY (the credit: that peer has
   * copied LAST run's block out of its inbox), then SEND of the own block out
   * of the output; for each peer rank-1, rank-2, ...: WAIT_RECV; one COPY
   * arena -> output per peer; one NOTIFY (the credit) per peer; WAIT_SEND per
   * peer sent to.  Empty blocks are skipped on both sides (both know the
   * counts).  One rank: the LOCAL_GATHER alone; one rank in place, or a total
   * of 0: no steps.  The credit orders run r + 1's send after run r's copy
   * out of the inbox, so runs need no barrier.  The executor never promotes
   * this plan; with device signalling the LOCAL_GATHER and every SEND are ONE
   * pass that reads each input tile once (reduce.hip gather_fanout_kernel). */
  GLOO_HIP_ALGO_ALLGATHER = 13,
  /* gloo::alltoall and gloo::alltoallv (gloo/alltoall.cc, gloo/alltoallv.cc).
   * Run through gloo_hip_alltoall_create (the algorithm object) and
   * gloo_hip_alltoall (function style), both below; gloo_hip_algorithm_create*
   * keep refusing the code as an unknown algorithm, because an alltoall's
   * pointers ({input, output}, neither a list) and its P x P count matrix do
   * not fit their signature.  ONE input and ONE output per rank, separate
   * buffers that share no byte (there is no in-place form).  Rank r's
   * input is P blocks back to back, block q (in_counts[q] elements) for rank
   * q; its output is P blocks back to back, block q (out_counts[q] elements)
   * from rank q; offsets are the prefix sums (alltoallv.cc:19-31):
   *   out_r[outOff_r[q], +out_counts_r[q]) == in_q[inOff_q[r], +in_counts_q[r])
   * Not a reduction: there is no op, dtype gives the element size.
   * gloo_hip_plan_ex(14, rank, size, count, ninputs = 1, noutputs = 1, ...,
   * recv_elems): recv_elems NULL is the even form, `count` elements per block
   * (alltoall.cc:29-30); otherwise it has 2 * size entries, in_counts[0..size)
   * then out_counts[0..size), and count is ignored.  ninputs != 1, noutputs !=
   * 1, a negative count, in_counts[rank] != out_counts[rank]
   * (alltoallv.cc:138) and | GLOO_HIP_ALGO_MESH are refused with
   * GLOO_HIP_EINVAL_ARG; the last-error text names the value.  gloo_hip_plan
   * (the short form) takes the even form only.
   * Route: the reference's own direct exchange, one hop per block.
   * Arena: laid out like the output; the inbox for peer q is
   * arena[outOff[q], +out_counts[q]) on GLOO_HIP_SLOT_DATA0; 0 at P = 1.
   * Order, empty blocks skipped on both sides: DECL_RECVs; COPY |
   * GLOO_HIP_FROM_INPUTS of the own block input -> output
   * (alltoallv.cc:137-145); for each peer rank+1, rank+2, ...: WAIT_NOTIFY |
   * GLOO_HIP_PREV_RUN on GLOO_HIP_SLOT_NOTIFY (the credit: that peer has
   * copied LAST run's block out of its inbox), then SEND |
   * GLOO_HIP_FROM_INPUTS of input block q; for each peer rank-1, rank-2, ...:
   * WAIT_RECV; one COPY arena -> output per peer; one NOTIFY (the credit)
   * per peer; WAIT_SEND per peer sent to.  One rank: the COPY alone.  A total
   * of 0: no steps.  The credit orders run r + 1's send after run r's copy out
   * of the inbox, so runs need no barrier.  The executor never promotes this
   * plan.
   * A sender writes one-sidedly, so in_counts_q[r] == out_counts_r[q] must
   * hold for every pair before a byte moves.  The executor gets it by
   * construction: it describes the call by the whole P x P matrix M (M[q * P +
   * r]: elements from rank q to rank r), the same on every rank, and plans
   * rank r from row r and column r (gloo_hip_alltoall_lists).  A rank that
   * passed another matrix is refused on every rank at construction.  With
   * device signalling a run is two multi-copy launches between two multi-flag
   * waits (the sends and the own block; the copy-outs), and one launch of
   * credits; no kernel is specific to it. */
  GLOO_HIP_ALGO_ALLTOALL = 14,
  /* gloo::gather and gloo::gatherv (gloo/gather.cc, gloo/gatherv.cc): every
   * rank contributes ONE input of counts[rank] elements; afterwards the
   * root's ONE output holds block 0, block 1, ... block P-1 back to back
   * (gather.cc:40-47; gatherv.cc:82-96: prefix offsets).  A non-root rank has
   * no output.  Not a reduction: op is NOT USED, dtype gives the element size.
   *   recv_elems  is required.  {root}: the even form, `count` elements per
   *          block.  {root, c_0 ... c_{P-1}}: gatherv, count ignored; every
   *          rank passes the full list, as in the reference (gatherv.cc:102).
   *          A C pointer carries no length, so gloo_hip_plan_ex and
   *          gloo_hip_algorithm_create* read the second form exactly when
   *          count == GLOO_HIP_COUNT_PER_RANK; gloo_hip_plan (the short form)
   *          takes it the same way.
   *   ptrs   at gloo_hip_algorithm_create*: {in} with nptrs = 1 on a rank
   *          without an output, {in, out} with nptrs = 2 on the root.  A
   *          non-root rank that passes a second pointer has it ignored (it
   *          may be NULL).  In gloo_hip_plan_ex: ninputs = 1; noutputs = 1 on
   *          the root, 0 ("no output") or 1 (ignored) elsewhere.
   * Refused with GLOO_HIP_EINVAL_ARG before any exchange, the last-error text
   * naming the value: a root outside [0, size), a negative count, a NULL
   * recv_elems (a count list of the wrong length, where the length is known:
   * gloo_amd::makeGatherPlan, gloo_amd.gather), ninputs != 1, a root without
   * an output, | GLOO_HIP_ALGO_MESH.
   * Route: the reference's own, every block straight to the root.
   * Arena, on the root: laid out like the output, sum(counts) elements; the
   * inbox for peer q is arena[offset(q), +c_q) on GLOO_HIP_SLOT_DATA0.
   * Root order (peers in ascending rank, empty blocks skipped on both sides):
   * DECL_RECVs; COPY | GLOO_HIP_FROM_INPUTS of the own block input -> output;
   * WAIT_RECV per peer; COPY arena -> output per peer; NOTIFY per peer on
   * GLOO_HIP_SLOT_NOTIFY (the credit: the block is out of the inbox).
   * Non-root order: WAIT_NOTIFY | GLOO_HIP_PREV_RUN (the root's credit of the
   * LAST run, met at once in the first); SEND | GLOO_HIP_FROM_INPUTS to the
   * root; WAIT_SEND.  One rank: the COPY alone.  A total of 0: no steps.  The
   * executor never promotes this plan.
   * Streams: gloo_hip_algorithm_create_streams takes ONE stream (the plan's)
   * or none for this algorithm and for GLOO_HIP_ALGO_SCATTER, whatever the
   * rank's pointer count: that count differs between the root and the rest.
   * Buffers: the root's input may BE its own slot of the output (in place:
   * the COPY then moves nothing); otherwise no input may share a byte with
   * the output. */
  GLOO_HIP_ALGO_GATHER = 15,
  /* gloo::scatter (gloo/scatter.cc): the root has P inputs of `count`
   * elements, one per destination rank (P separate buffers, scatter.cc:31-35;
   * they may be slices of one allocation); afterwards rank q's ONE output
   * holds the root's input q.  There is no scatterv.  Not a reduction: op is
   * NOT USED, dtype gives the element size.
   *   recv_elems  is required: {root}.
   *   ptrs   at gloo_hip_algorithm_create*: {out} with nptrs = 1 on a rank
   *          that is not the root (further pointers are ignored), {out, in_0
   *          ... in_{P-1}} with nptrs = 1 + size on the root.  In
   *          gloo_hip_plan_ex: noutputs = 1; ninputs = size on the root, any
   *          value elsewhere (0: none).
   * Refused with GLOO_HIP_EINVAL_ARG before any exchange, naming the value: a
   * root outside [0, size), a NULL recv_elems, noutputs != 1, a root whose
   * ninputs is not size, | GLOO_HIP_ALGO_MESH.
   * Arena: `count` elements on a non-root rank (its one inbox, from the root,
   * on GLOO_HIP_SLOT_DATA0); nothing on the root.
   * Root order: for each peer q in ascending rank WAIT_NOTIFY (its
   * clear-to-send) then SEND | GLOO_HIP_FROM_INPUTS | GLOO_HIP_INPUT(q); COPY |
   * GLOO_HIP_FROM_INPUTS | GLOO_HIP_INPUT(root) of the own block input ->
   * output; WAIT_SEND per peer.  Non-root order: DECL_RECV; NOTIFY
   * (clear-to-send, the broadcast's protocol); WAIT_RECV; COPY arena ->
   * output.  One rank: the COPY alone; count 0: no steps.  The clear-to-send
   * orders the root's next send after the receiver's copy out of its inbox,
   * so runs need no barrier.  The executor never promotes this plan.
   * Buffers: the root's output may BE its input `root` (in place); otherwise
   * the output may share no byte with any input (the sends read the inputs
   * while the own block is stored). */
  GLOO_HIP_ALGO_SCATTER = 16,
} gloo_hip_algo_t;

/* GLOO_HIP_ALGO_GATHER: `count` of the gatherv form, recv_elems = {root, c_0 ...
 * c_{size-1}} (a legitimate count never reaches it). */
#define GLOO_HIP_COUNT_PER_RANK ((size_t)-1)

/* algo | GLOO_HIP_ALGO_MESH: the algorithm's result with mesh data movement,
 * derived mechanically (gloo_amd/csrc/mesh.cc): every rank's plan is run
 * symbolically to find, per element range, the exact expression tree the
 * reference evaluates and the rank that finishes it; raw pieces then go
 * straight to that rank (all links at once), which evaluates the same tree,
 * and (allreduce) sends the result to every rank.  Bit-identical results.
 * For HALVING_DOUBLING and REDUCE_SCATTER (and RING_CHUNKED), 2 <= size <= 8. */
#define GLOO_HIP_ALGO_MESH 0x100

typedef enum {
  GLOO_HIP_STEP_DECL_RECV = 0,   /* inbox region for (peer, slot): arena[dst_off, +length) */
  GLOO_HIP_STEP_SEND = 1,        /* src[src_off, +length) -> peer's (me, slot) region       */
  GLOO_HIP_STEP_WAIT_RECV = 2,   /* wait for the next message from (peer, slot)             */
  GLOO_HIP_STEP_REDUCE = 3,      /* user[dst_off..] = user[dst_off..] op arena[src_off..]   */
  GLOO_HIP_STEP_COPY = 4,        /* dst[dst_off..] = src[src_off..] (memmove semantics)     */
  GLOO_HIP_STEP_NOTIFY = 5,      /* one notification to (peer, slot)                        */
  GLOO_HIP_STEP_WAIT_NOTIFY = 6, /* wait for the next notification from (peer, slot)        */
  GLOO_HIP_STEP_WAIT_SEND = 7,   /* wait until our last send to (peer, slot) has completed  */
  GLOO_HIP_STEP_LOCAL_REDUCE = 8,/* ptrs[0] = ((ptrs[0] op ptrs[1]) op ...), length elts    */
  GLOO_HIP_STEP_LOCAL_BCAST = 9, /* ptrs[i] = ptrs[0] for i >= 1, length elements           */
  GLOO_HIP_STEP_FOLD_SRC = 10,   /* next source of the following FOLD: src[src_off..]        */
  GLOO_HIP_STEP_FOLD = 11,       /* user[dst_off, +length) = fold of the pending FOLD_SRCs:
                                    acc = s0; acc = acc op s_k (or s_k op acc with
                                    GLOO_HIP_FOLD_REVERSE), k = 1.. in order             */
  GLOO_HIP_STEP_LOCAL_GATHER = 12,/* for every input i: user[dst_off + i * length, +length)
                                    = input_i[0, +length)  (GLOO_HIP_ALGO_ALLGATHER)      */
} gloo_hip_step_kind_t;

/* Message channels between a pair of ranks (the reference's slot roles). */
#define GLOO_HIP_SLOT_DATA0 0
#define GLOO_HIP_SLOT_DATA1 1
#define GLOO_HIP_SLOT_NOTIFY 2
#define GLOO_HIP_SLOT_DIST 3
#define GLOO_HIP_SLOT_DIST_NOTIFY 4
#define GLOO_HIP_SLOT_AUX0 5
#define GLOO_HIP_SLOT_AUX1 6
#define GLOO_HIP_SLOT_AUX_NOTIFY 7
#define GLOO_HIP_NUM_SLOTS 8

/* flags: which space each side of a data step lives in. */
#define GLOO_HIP_SRC_ARENA 1 /* else the user buffer ptrs[0] */
#define GLOO_HIP_DST_ARENA 2
/* LOCAL_REDUCE over [dst_off, +length) folds the separate INPUT buffers into
 * output 0 (new-style allreduce; one input = copy), instead of folding the
 * outputs into output 0.  On REDUCE: user[dst] = input0[dst] op arena[src]
 * (gloo::reduce's out = in op tmp); on SEND: the source is input 0; on COPY
 * (the own block of GLOO_HIP_ALGO_ALLTOALL and of the rooted collectives): the
 * source is input 0 as well, user[dst_off, +length) = input0[src_off, +length).
 * WHICH input a SEND or a COPY reads is in bits 8 and up of `flags`:
 * GLOO_HIP_INPUT(q) names input q, GLOO_HIP_INPUT_OF(flags) reads it back.
 * Every plan that knows one input leaves those bits 0 and so emits the steps
 * it always did; GLOO_HIP_ALGO_SCATTER's root names input q for rank q
 * (GLOO_HIP_ALGO_GATHER reads input 0).  The bits mean nothing without
 * GLOO_HIP_FROM_INPUTS, and nothing on REDUCE, LOCAL_REDUCE and LOCAL_GATHER. */
#define GLOO_HIP_FROM_INPUTS 4
#define GLOO_HIP_INPUT_SHIFT 8
#define GLOO_HIP_INPUT(q) ((int32_t)((uint32_t)(q) << GLOO_HIP_INPUT_SHIFT))
#define GLOO_HIP_INPUT_OF(flags) ((int)((uint32_t)(flags) >> GLOO_HIP_INPUT_SHIFT))
/* FOLD: each new source is the LEFT operand (acc = s_k op acc). */
#define GLOO_HIP_FOLD_REVERSE 8
/* FOLD: balanced pairwise tree over the sources in order (k a power of two):
 * ((s0 op s1) op (s2 op s3)) op ((s4 op s5) op (s6 op s7)).  FOLD also takes
 * GLOO_HIP_DST_ARENA (result into the arena). */
#define GLOO_HIP_FOLD_TREE 16
/* WAIT_NOTIFY: wait for the notification of the PREVIOUS run (a credit the
 * receiver returns after consuming; satisfied at once in the first run). */
#define GLOO_HIP_PREV_RUN 32

typedef struct {
  int32_t kind;
  int32_t peer;
  int32_t slot;
  int32_t flags;
  uint64_t dst_off; /* elements */
  uint64_t src_off; /* elements */
  uint64_t length;  /* elements */
} gloo_hip_step_t;

/* Build rank `rank`'s plan of algorithm `algo` for `size` ranks, `count`
 * elements and `nptrs` local pointers.  recv_elems (size entries) is used by
 * GLOO_HIP_ALGO_REDUCE_SCATTER only.  With steps == NULL only *nsteps is
 * filled.  *arena_elems receives the inbox arena size this rank needs. */
int gloo_hip_plan(int algo, int rank, int size, size_t count, int nptrs,
                  const int* recv_elems, gloo_hip_step_t* steps, size_t capacity,
                  size_t* nsteps, size_t* arena_elems);

/* Full form: `ninputs` separate input buffers (0 = the outputs are the
 * inputs), `noutputs` outputs, element size and the new-style allreduce's
 * maximum segment size in bytes (0 = 1 MiB, gloo/allreduce.h:78). */
int gloo_hip_plan_ex(int algo, int rank, int size, size_t count, int ninputs, int noutputs,
                     size_t elem_size, size_t max_segment_bytes, const int* recv_elems,
                     gloo_hip_step_t* steps, size_t capacity, size_t* nsteps,
                     size_t* arena_elems);

/* (new, tests and tooling) The batching rule of the one-launch plan
 * interpreter: which steps of a step list are not drained before the next
 * (signal.h kInterpDefer).  Each step is a kind (0 copy, 1 send, 2 signal,
 * 3 wait, 4 fold), its destination and nsrc source addresses and its length
 * in bytes; addresses are only compared, never dereferenced.  defer_out[i]
 * receives 1 where step i and step i+1 share one drain. */
typedef struct {
  int32_t kind;
  int32_t nsrc;
  uint64_t dst;
  uint64_t src[GLOO_HIP_MAX_SRCS];
  uint64_t bytes;
} gloo_hip_interp_desc_t;
int gloo_hip_interp_batches(const gloo_hip_interp_desc_t* steps, int n, int* defer_out);
/* The same for step lists with multi-destination copies: a copy (kind 0)
 * may store its bytes to nxdst further local destinations (a broadcast to a
 * rank's other pointers, one load per tile), every one of which counts as
 * written by the step.  nxdst is 0 for every other kind. */
#define GLOO_HIP_MAX_XDSTS 8
typedef struct {
  gloo_hip_interp_desc_t step;
  int32_t nxdst;
  int32_t reserved; /* 0 */
  uint64_t xdst[GLOO_HIP_MAX_XDSTS];
} gloo_hip_interp_desc_ex_t;
int gloo_hip_interp_batches_ex(const gloo_hip_interp_desc_ex_t* steps, int n, int* defer_out);

/* (new, tests) The one-launch plan interpreter (reduce.hip plan_interp_kernel)
 * on a caller's step list, without a peer.  One step: */
typedef struct {
  int32_t kind;    /* 0 copy, 1 send, 2 signal, 3 wait, 4 fold (as gloo_hip_interp_desc_t) */
  int32_t mode;    /* fold: 0 left (acc = acc op s_j), 1 reverse (acc = s_j op acc), 2 balanced tree */
  int32_t nsrc;    /* fold: sources, 1..GLOO_HIP_MAX_SRCS (a power of two under mode 2); copy / send: src[0] */
  int32_t defer;   /* 1: this step and the next share one drain (gloo_hip_interp_batches_ex) */
  uint64_t* flag;  /* send / signal: slice g stores base + run * per_run (mod 2^64) to flag[g]; wait: polls flag[g] */
  uint64_t base, per_run;
  void* dst;
  const void* src[GLOO_HIP_MAX_SRCS];
  uint64_t n;      /* elements of `dtype` */
  int32_t nxdst;   /* copy: further destinations of the same bytes */
  int32_t reserved; /* 0 */
  void* xdst[GLOO_HIP_MAX_XDSTS];
} gloo_hip_interp_step_t;
/* steps: a HOST array of nsteps <= 512 steps.  The entry stages it in device
 * memory of its own, launches `slices` (1..256) workgroups on `stream` —
 * workgroup g takes elements [min(n, g q), min(n, g q + q)) of every data
 * step, q = ceil(n / slices) rounded up to 16 bytes, and flag word g —
 * SYNCHRONISES the stream and frees the staging: a synchronous test entry,
 * not a hot path.  A wait is met by signed 64-bit difference (a target below
 * the counter passes at once); one that is not met within timeout_ticks
 * (1..10^9 ticks of the 100 MHz clock, 10 s at the most) stores 1 to *err and
 * ends its workgroup: no later step, no later flag, no done.  done /
 * done_ticket (both or neither; the ticket a zeroed device word): the
 * workgroup finishing last stores `run` to *done and leaves the ticket at 0.
 * Built-in ops only.  Every argument and every step is checked before any
 * GPU call (the last-error text names the step and the value): kind, mode,
 * nsrc, the defer bit (0 / 1, never on the last step, never between a wait
 * and a step that is none), a flag on send / signal / wait, and with n > 0
 * non-null element-aligned dst, sources and extra destinations, a copy's or
 * send's source disjoint from its destinations, nxdst 0..8 and 0 on every
 * kind but copy.  nsteps == 0 launches nothing. */
int gloo_hip_interp_kernel(int op, int dtype, const gloo_hip_interp_step_t* steps, int nsteps, uint64_t run,
                           int slices, uint64_t timeout_ticks, uint32_t* err, uint64_t* done, unsigned* done_ticket,
                           gloo_hip_stream_t stream);

/* (new, tests) The fused small step (reduce.hip fused_small_kernel), one
 * workgroup: [wait until *wait_flag >= wait value, by signed difference] ->
 * dst[i] = dst[i] op src[i], i < n (op 0: dst[i] = src[i]) -> [*sig_flag =
 * signal value].  A value is base + *epoch * per_run (mod 2^64), or base with
 * epoch == NULL (epoch: a device word).  A wait not met within timeout_ticks
 * (1..10^9) stores 1 to *err (never NULL): no work, no signal.  dst and src
 * are element-aligned and disjoint.  Asynchronous on `stream`; every argument
 * is checked before any GPU call; n == 0 without a flag launches nothing. */
int gloo_hip_fused_step(int op, int dtype, void* dst, const void* src, size_t n, const uint64_t* wait_flag,
                        uint64_t wait_base, uint64_t wait_per_run, uint64_t timeout_ticks, uint32_t* err,
                        uint64_t* sig_flag, uint64_t sig_base, uint64_t sig_per_run, const uint64_t* epoch,
                        gloo_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * Contexts and algorithms (the GPU allreduce / reduce-scatter drop-ins).
 *
 *   gloo_hip_context_create  <- rendezvous::Context(rank, size) +
 *                               connectFullMesh(store, device)
 *                               (gloo/rendezvous/context.cc:25-35); the store
 *                               is "file:<dir>" (ranks = processes of one
 *                               node) or "mem:<name>" (ranks = threads).
 *   gloo_hip_algorithm_create <- the constructors of CudaAllreduceRingChunked
 *                               (gloo/cuda_allreduce_ring_chunked.h:19-26),
 *                               CudaAllreduceHalvingDoubling
 *                               (gloo/cuda_allreduce_halving_doubling.h:25-30),
 *                               CudaAllreduceRing, CudaAllreduceLocal and
 *                               ReduceScatterHalvingDoubling
 *                               (gloo/reduce_scatter.h:112-117): device
 *                               pointers `ptrs` (nptrs of them, on this
 *                               rank's device), `count` elements each.
 *                               Collective: every rank creates its
 *                               algorithms in the same order.
 *   gloo_hip_algorithm_run   <- Algorithm::run() (gloo/algorithm.h:26).  With
 *                               stream == NULL outputs are complete on
 *                               return; otherwise the work is ordered on
 *                               `stream` and the caller synchronises.
 * ---------------------------------------------------------------------- */
typedef struct gloo_hip_context* gloo_hip_context_t;
typedef struct gloo_hip_algorithm* gloo_hip_algorithm_t;

int gloo_hip_context_create(int rank, int size, const char* store_url, int device,
                            int timeout_ms, gloo_hip_context_t* out);
int gloo_hip_context_destroy(gloo_hip_context_t ctx);

/* Bootstrap over an existing collective context instead of a store: the
 * caller supplies an all-gather of fixed `block`-byte records (every rank
 * passes `in`; `out` receives size * block bytes, rank r's record at
 * r * block; return 0 on success).  Every exchange the library makes (the
 * control block's name, each algorithm's inbox-arena / IPC records,
 * set-up and tear-down barriers) is one such collective call, made in the
 * same order on every rank from the calling thread.  This is how a Gloo
 * program hands over its own gloo::Context (gloo/context.h:26-59): the
 * header-only bridge gloo_amd/include/gloo_amd/gloo_bridge.h passes
 * gloo::allgather over that context's pairs, so there is no second
 * rendezvous. */
typedef int (*gloo_hip_allgather_fn)(void* user, const void* in, void* out, size_t block);
int gloo_hip_context_create_ex(int rank, int size, int device, int timeout_ms, gloo_hip_allgather_fn allgather,
                               void* user, gloo_hip_context_t* out);

int gloo_hip_algorithm_create(gloo_hip_context_t ctx, int algo, int op, int dtype,
                              void* const* ptrs, int nptrs, size_t count,
                              const int* recv_elems, gloo_hip_stream_t stream,
                              gloo_hip_algorithm_t* out);
/* Where the inboxes (the transport's receive buffers) live — the reference's
 * workspace template argument (gloo/cuda_workspace.h:20-31):
 *   DEVICE  HBM of the rank's GPU (CudaDeviceWorkspace; the default here);
 *   HOST    pinned host memory shared by the node's ranks (CudaHostWorkspace:
 *           chunks arrive in host memory, as from a socket/NIC); peers write
 *           them over PCIe and the reduce kernel reads them in place
 *           (zero-copy) while accumulating into the device buffer. */
typedef enum { GLOO_HIP_WORKSPACE_DEVICE = 0, GLOO_HIP_WORKSPACE_HOST = 1 } gloo_hip_workspace_t;

/* gloo_hip_algorithm_create with an explicit workspace. */
int gloo_hip_algorithm_create_ws(gloo_hip_context_t ctx, int algo, int op, int dtype, void* const* ptrs, int nptrs,
                                 size_t count, const int* recv_elems, gloo_hip_stream_t stream, int workspace,
                                 gloo_hip_algorithm_t* out);

/* gloo_hip_algorithm_create_ws with one stream per pointer, the reference's
 * `const std::vector<cudaStream_t>& streams` (gloo/cuda_allreduce_ring_chunked.h:19-26,
 * GLOO_ENFORCE_EQ(streams.size(), ptrs.size()) at .cc:55-58): nstreams is 0
 * (run() returns with the outputs complete) or nptrs.  run() orders its use
 * of ptrs[i] after the work already queued on streams[i], and on return
 * every streams[i] is ordered after the collective (docs/cuda.md:7-11): the
 * caller synchronises with any of them.  The library never uses a stream
 * outside create/run, so a caller may destroy it between runs (each run()
 * then needs the streams it was created with, or those of
 * gloo_hip_algorithm_set_streams). */
int gloo_hip_algorithm_create_streams(gloo_hip_context_t ctx, int algo, int op, int dtype, void* const* ptrs,
                                      int nptrs, size_t count, const int* recv_elems,
                                      const gloo_hip_stream_t* streams, int nstreams, int workspace,
                                      gloo_hip_algorithm_t* out);
/* Rebind the streams of later runs (same rule: 0 or nptrs of them). */
int gloo_hip_algorithm_set_streams(gloo_hip_algorithm_t algo, const gloo_hip_stream_t* streams, int nstreams);

int gloo_hip_algorithm_run(gloo_hip_algorithm_t algo);

/* This process's pool of cross-process slabs (gloo_amd/include/gloo_amd/ipc.h:
 * HIP VMM blocks shared as dma-buf fds, never freed while the process lives,
 * reused by size class; no reference counterpart, for tests and tools):
 * out5[0] = slabs exported, [1] = their bytes, [2] = slabs free for reuse,
 * [3] = peer slabs mapped, [4] = imports made (a peer slab is mapped once and
 * kept). */
int gloo_hip_ipc_stats(uint64_t* out5);
/* The same, up to 6 words: + mappings of exited peers (their pid reused)
 * dropped. */
int gloo_hip_ipc_stats_ex(uint64_t* out, size_t n);
int gloo_hip_algorithm_destroy(gloo_hip_algorithm_t algo);
/* Host seconds the last run() spent blocked waiting for peers. */
double gloo_hip_algorithm_wait_seconds(gloo_hip_algorithm_t algo);
/* Measurement.  on = 1: bracket every chunk reduction of run() with HIP
 * events (runs are then enqueued eagerly); on = 2: device-side stamps inside
 * the reduce kernels (each records its first-workgroup start and
 * last-workgroup end on the GPU's 100 MHz clock), which keeps hipGraph
 * replay; 0: off.  After a run: stats[0] = summed reduce-kernel seconds,
 * stats[1] = algorithmic bytes reduced (3 * n * sizeof(T) per two-operand
 * chunk, (k + 1) * n * sizeof(T) per k-source fold), stats[2] = chunk
 * reductions, stats[3] = host seconds blocked on peers. */
int gloo_hip_algorithm_set_profiling(gloo_hip_algorithm_t algo, int on);
int gloo_hip_algorithm_stats(gloo_hip_algorithm_t algo, double* stats4);

/* How the algorithm executes (no reference counterpart; for tests and
 * tools): mode4[0] = device-side signalling, [1] = inbox arena (0 device
 * memory no peer writes, 1 device fine-grained, 2 pinned host),
 * [2] = bit 1: some run fused a fold with the SENDs of its result
 * (fold+forward), bit 2: runs on the algorithm's own stream (run() returns
 * with the outputs complete), [3] = how run() launches the plan: 0 enqueued
 * step by step, 1 a captured hipGraph replayed, k >= 2 the one-launch plan
 * interpreter with k - 1 workgroups (> 1: sliced).  If graph capture was
 * abandoned, gloo_hip_last_error() says why. */
int gloo_hip_algorithm_mode(gloo_hip_algorithm_t algo, int* mode4);
/* The same for the schedule that ran the latest function-style call
 * (gloo_hip_allreduce / gloo_hip_reduce_to_root / gloo_hip_broadcast /
 * gloo_hip_allgather / gloo_hip_gather / gloo_hip_scatter / gloo_hip_alltoall)
 * on `ctx`. */
int gloo_hip_context_mode(gloo_hip_context_t ctx, int* mode4);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::allreduce(const AllreduceOptions&)
 * (gloo/allreduce.h:89-193, gloo/allreduce.cc:97-145), RING algorithm.
 * inputs may be empty (the outputs are the inputs); every output receives
 * the result.  Collective: all ranks call with the same options in the same
 * order.  The first call with a given option set builds the schedule and
 * inbox arena (a store exchange); later calls reuse it with the buffers of
 * the call.
 * ---------------------------------------------------------------------- */
#define GLOO_HIP_ALLREDUCE_RING 1  /* AllreduceOptions::Algorithm::RING  */
#define GLOO_HIP_ALLREDUCE_BCUBE 2 /* AllreduceOptions::Algorithm::BCUBE (gloo/allreduce.h:38-42) */
typedef struct {
  int algorithm;            /* 0 (unspecified = RING), RING or BCUBE      */
  int op;                   /* gloo_hip_op_t: the reduce Func             */
  int dtype;                /* gloo_hip_dtype_t: setInputs<T>/setOutputs<T> */
  void* const* inputs;      /* device pointers, may be NULL               */
  int ninputs;
  void* const* outputs;     /* device pointers, at least one              */
  int noutputs;
  size_t elements;
  size_t max_segment_bytes; /* setMaxSegmentSize; 0 = 1 MiB               */
  uint32_t tag;             /* setTag                                     */
  gloo_hip_stream_t stream; /* NULL: outputs complete on return           */
} gloo_hip_allreduce_options_t;

int gloo_hip_allreduce(gloo_hip_context_t ctx, const gloo_hip_allreduce_options_t* opts);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::reduce(ReduceOptions&) (gloo/reduce.h:19-112,
 * gloo/reduce.cc:21-247): a ring reduce-scatter over <= max_segment_bytes
 * segments, then every rank's reduced chunk is gathered at `root`.  `input`
 * may be NULL (the output is the input).  Only the root's output holds the
 * full result; the other ranks' outputs hold the same partial reductions the
 * reference leaves there.  Collective, cached per option set like
 * gloo_hip_allreduce.
 * ---------------------------------------------------------------------- */
typedef struct {
  int op;                   /* gloo_hip_op_t: the reduce Func              */
  int dtype;                /* gloo_hip_dtype_t: setInput<T>/setOutput<T>  */
  void* input;              /* device pointer, may be NULL                 */
  void* output;             /* device pointer                              */
  size_t elements;
  int root;                 /* setRoot                                     */
  size_t max_segment_bytes; /* setMaxSegmentSize; 0 = 1 MiB (reduce.h:98)  */
  uint32_t tag;             /* setTag                                      */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return      */
} gloo_hip_reduce_options_t;

int gloo_hip_reduce_to_root(gloo_hip_context_t ctx, const gloo_hip_reduce_options_t* opts);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::broadcast(BroadcastOptions&)
 * (gloo/broadcast.h:16-89, gloo/broadcast.cc): afterwards `output` on every
 * rank holds the bytes of the root's `input` (the root's `output` when its
 * input is NULL or the same pointer).  The reference walks a binomial tree
 * over its pairs; this runs the one-to-all route of CudaBroadcastOneToAll
 * (GLOO_HIP_ALGO_BROADCAST), because a root GPU has a direct link to every
 * peer and the bytes that arrive are the same.  A root with a separate input
 * first copies it to its output on the call's stream.  Collective, cached per
 * option set (dtype, elements, root, tag) like gloo_hip_allreduce;
 * gloo_hip_context_mode reports the schedule that ran.
 * ---------------------------------------------------------------------- */
typedef struct {
  int dtype;                /* gloo_hip_dtype_t: setInput<T>/setOutput<T>            */
  void* input;              /* device pointer; used on the root only; NULL: the output is the input */
  void* output;             /* device pointer                                        */
  size_t elements;
  int root;                 /* setRoot                                               */
  uint32_t tag;             /* setTag                                                */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return                */
} gloo_hip_broadcast_options_t;

int gloo_hip_broadcast(gloo_hip_context_t ctx, const gloo_hip_broadcast_options_t* opts);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::allgather(AllgatherOptions&)
 * (gloo/allgather.h, gloo/allgather.cc) and gloo::allgatherv
 * (gloo/allgatherv.h, gloo/allgatherv.cc) in one call: afterwards `output` on
 * every rank holds rank 0's input, rank 1's input, ... back to back
 * (`elements` each, or counts[r] with counts given: allgatherv's prefix
 * offsets, allgatherv.cc:90-101).  input NULL is the in-place form
 * (allgather.cc:47-54): the rank's own block already sits in its slot of the
 * output.  The reference passes blocks round a ring; this runs the direct
 * exchange of GLOO_HIP_ALGO_ALLGATHER (every rank sends its block straight to
 * every peer), the same bytes.  Collective, cached per option set (dtype,
 * counts, in place or not, tag) like gloo_hip_broadcast;
 * gloo_hip_context_mode reports the schedule that ran.
 * ---------------------------------------------------------------------- */
typedef struct {
  int dtype;                /* gloo_hip_dtype_t: setInput<T>/setOutput<T>            */
  void* input;              /* device pointer; NULL: in place                        */
  void* output;             /* device pointer, the sum of the counts in elements     */
  size_t elements;          /* per rank; ignored when counts is given                */
  const size_t* counts;     /* NULL: `elements` on every rank; else `size` entries   */
  uint32_t tag;             /* setTag                                                */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return                */
} gloo_hip_allgather_options_t;

int gloo_hip_allgather(gloo_hip_context_t ctx, const gloo_hip_allgather_options_t* opts);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::gather(GatherOptions&) (gloo/gather.h,
 * gloo/gather.cc) and gloo::gatherv (gloo/gatherv.h, gloo/gatherv.cc) in one
 * call: afterwards `output` on the ROOT holds rank 0's input, rank 1's input,
 * ... back to back (`elements` each, or counts[r] with counts given:
 * gatherv's prefix offsets, gatherv.cc:82-96).  A rank that is not the root
 * has no output: it leaves `output` NULL (a pointer given there is ignored and
 * never written).  Every rank passes the same root, elements and counts (the
 * full list, gatherv.cc:102).  Runs GLOO_HIP_ALGO_GATHER.  Collective, cached
 * per option set (dtype, counts, root, tag) like gloo_hip_allgather;
 * gloo_hip_context_mode reports the schedule that ran.  A bad dtype, a root
 * outside [0, size), a count above INT32_MAX, a NULL input with elements to
 * send and a NULL output on the root are refused before any exchange.
 * ---------------------------------------------------------------------- */
typedef struct {
  int dtype;                /* gloo_hip_dtype_t                                      */
  int root;                 /* setRoot                                               */
  void* input;              /* device pointer, this rank's block                     */
  void* output;             /* root: device pointer, the sum of the counts; else NULL */
  size_t elements;          /* per rank; ignored when counts is given                */
  const size_t* counts;     /* NULL: `elements` on every rank; else `size` entries   */
  uint32_t tag;             /* setTag                                                */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return                */
} gloo_hip_gather_options_t;

int gloo_hip_gather(gloo_hip_context_t ctx, const gloo_hip_gather_options_t* opts);

/* ------------------------------------------------------------------------
 * New-style function API: gloo::scatter(ScatterOptions&) (gloo/scatter.h,
 * gloo/scatter.cc): afterwards `output` on rank q holds the root's inputs[q],
 * `elements` elements.  inputs is a HOST array of `size` device pointers that
 * the root alone sets (P separate buffers, scatter.cc:31-35; they may be
 * slices of one allocation); every other rank leaves it NULL (it is not read
 * there).  Runs GLOO_HIP_ALGO_SCATTER.  Collective, cached per option set
 * (dtype, elements, root, tag).  A bad dtype, a root outside [0, size), a NULL
 * output and, on the root, a NULL inputs array or entry are refused before
 * any exchange.
 * ---------------------------------------------------------------------- */
typedef struct {
  int dtype;                /* gloo_hip_dtype_t                                      */
  int root;                 /* setRoot                                               */
  void* output;             /* device pointer, `elements` elements                   */
  void* const* inputs;      /* root: host array of `size` device pointers; else NULL */
  size_t elements;          /* per rank                                              */
  uint32_t tag;             /* setTag                                                */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return                */
} gloo_hip_scatter_options_t;

int gloo_hip_scatter(gloo_hip_context_t ctx, const gloo_hip_scatter_options_t* opts);

/* ------------------------------------------------------------------------
 * gloo::alltoall(AlltoallOptions&) (gloo/alltoall.h, gloo/alltoall.cc) and
 * gloo::alltoallv(AlltoallvOptions&) (gloo/alltoallv.h, gloo/alltoallv.cc):
 * GLOO_HIP_ALGO_ALLTOALL above.  Afterwards block q of rank r's `output` holds
 * block r of rank q's `input`.
 *
 * gloo_hip_alltoall_create is the algorithm object (create once,
 * gloo_hip_algorithm_run many times, gloo_hip_algorithm_destroy; the stats,
 * mode and profiling calls apply).  matrix NULL: the even form, `count`
 * elements per block.  Otherwise matrix has size * size ints, matrix[q * size
 * + r] the elements rank q sends to rank r, THE SAME ON EVERY RANK, and count
 * is ignored; this rank's input is row `rank` back to back, its output column
 * `rank`.  Collective.  One stream, or NULL for the algorithm's own (run()
 * then returns with the output complete).  workspace: GLOO_HIP_WORKSPACE_*.
 * Refused on this rank before any exchange, the last-error text naming the
 * value: a bad dtype, a negative count anywhere in the matrix, a NULL input or
 * output where this rank has elements to send or receive, an input that
 * shares a byte with the output.  A rank that passed another matrix (or
 * count, or dtype) than rank 0 makes the construction fail on EVERY rank,
 * before a byte moves.
 *
 * gloo_hip_alltoall is the function-style call, cached per option set like
 * gloo_hip_allgather; gloo_hip_context_mode reports the schedule that ran.
 * Three forms:
 *   even       in_counts, out_counts and matrix NULL: `elements` per block.
 *              Cached per (dtype, elements, tag).
 *   matrix     matrix given (size * size entries, the same on every rank; the
 *              own lists may be given too and must then equal its row and
 *              column `rank`).  Cached per (dtype, matrix, tag).  No count
 *              exchange: ranks that disagree are refused at construction.
 *   own lists  in_counts and out_counts only, `size` entries each: the
 *              reference's alltoallv, where a rank knows its own blocks only.
 *              EVERY call of this form costs one host exchange of the 2 * size
 *              counts through the context's store: every rank assembles the
 *              matrix from the same records and checks every pair, so a
 *              mismatch is refused on every rank alike, naming the pair and
 *              both values, before any schedule is built or any byte moves;
 *              the call then goes on as the matrix form.  (The cache key must
 *              be the same on every rank, because building a schedule is
 *              collective; a rank's own lists are not.)  Callers with fixed
 *              counts, and callers who can supply the matrix, should use the
 *              other two forms.
 * in_counts and out_counts are both given or both NULL.  Refused before any
 * exchange, naming the value: a bad dtype, only one of the two lists, a count
 * above INT32_MAX, in_counts[rank] != out_counts[rank] (alltoallv.cc:138), a
 * matrix whose row or column `rank` differs from the own lists, a NULL input
 * or output where there are elements to move, overlapping input and output.
 * A total of 0 on every rank returns at once.
 *
 * gloo_hip_alltoall_lists writes row `rank` then column `rank` of `matrix`
 * (size * size ints) to lists[0, 2 * size): the recv_elems gloo_hip_plan_ex
 * takes for that rank, as the executor derives them.
 * ---------------------------------------------------------------------- */
typedef struct {
  int dtype;                /* gloo_hip_dtype_t                                      */
  void* input;              /* device pointer: `size` blocks back to back            */
  void* output;             /* device pointer: `size` blocks back to back            */
  size_t elements;          /* per block; the even form only                         */
  const size_t* in_counts;  /* NULL, or `size` entries: elements for each rank       */
  const size_t* out_counts; /* NULL, or `size` entries: elements from each rank      */
  const size_t* matrix;     /* NULL, or size * size entries, [q * size + r]: q to r  */
  uint32_t tag;             /* setTag                                                */
  gloo_hip_stream_t stream; /* NULL: the output is complete on return                */
} gloo_hip_alltoall_options_t;

int gloo_hip_alltoall(gloo_hip_context_t ctx, const gloo_hip_alltoall_options_t* opts);
int gloo_hip_alltoall_create(gloo_hip_context_t ctx, int dtype, void* input, void* output, size_t count,
                             const int* matrix /* NULL: even */, gloo_hip_stream_t stream, int workspace,
                             gloo_hip_algorithm_t* out);
int gloo_hip_alltoall_lists(int rank, int size, const int* matrix, int* lists);

/* ------------------------------------------------------------------------
 * The xGMI transport: bound buffers of gloo::transport::Pair / Buffer
 * (gloo/transport/pair.h:33-41, gloo/transport/buffer.h:26-34) over device
 * memory.  gloo_amd/include/gloo_amd/gloo_transport.h wraps these into a
 * gloo::transport::Device (gloo/transport/device.h:34-54) that
 * gloo::rendezvous::Context::connectFullMesh accepts.
 *
 *   gloo_hip_context_create_kv  <- transport::Context::createAndConnectAllPairs
 *       (gloo/transport/context.cc:26-89): the caller's key/value store
 *       (gloo::IStore set / wait+get) carries the set-up records.  set: store
 *       `len` bytes under `key`; get: wait up to timeout_ms for `key`, copy up
 *       to `cap` bytes into `out` and its full length into *len (the library
 *       calls again with a larger buffer when *len > cap).  Both return 0 on
 *       success, nonzero on failure (a timeout: GLOO_HIP_EIO).  The store
 *       must outlive the context: receive buffers publish records in it.
 *   gloo_hip_transport_create   <- transport::Device::createContext: one per
 *       context (collective, in the same order as algorithm creation); sends
 *       are ordered on `stream` (NULL: a stream of its own).
 *   gloo_hip_buffer_create      <- Pair::createSendBuffer (is_send = 1) /
 *       createRecvBuffer (is_send = 0) for the pair to `peer`.  A receive
 *       buffer is memory the peer writes into: device memory (HIP IPC across
 *       processes, the pointer itself within one process) or host memory
 *       (written directly within one process; across processes carried in
 *       the channel's 48 payload bytes, the reference's notification
 *       buffers).  ptr == NULL / size 0: a notification buffer.  Any number
 *       of distinct slots may be live (up to 128 receive buffers per peer).
 *   gloo_hip_buffer_send        <- Buffer::send(offset, length, roffset): a
 *       copy into the peer's receive buffer (a direct xGMI copy between
 *       GPUs), then, stream-ordered after the bytes landed, an arrival.
 *   gloo_hip_buffer_wait_recv   <- Buffer::waitRecv: the next arrival, or
 *       GLOO_HIP_EIO after the context timeout (gloo::IoException).
 *   gloo_hip_buffer_wait_send   <- Buffer::waitSend: the last send's copy out
 *       of this buffer has completed.
 * ---------------------------------------------------------------------- */
typedef int (*gloo_hip_kv_set_fn)(void* user, const char* key, const void* data, size_t len);
typedef int (*gloo_hip_kv_get_fn)(void* user, const char* key, int timeout_ms, void* out, size_t cap, size_t* len);
int gloo_hip_context_create_kv(int rank, int size, int device, int timeout_ms, gloo_hip_kv_set_fn set,
                               gloo_hip_kv_get_fn get, void* user, gloo_hip_context_t* out);

typedef struct gloo_hip_transport* gloo_hip_transport_t;
typedef struct gloo_hip_buffer* gloo_hip_buffer_t;
int gloo_hip_transport_create(gloo_hip_context_t ctx, gloo_hip_stream_t stream, gloo_hip_transport_t* out);
int gloo_hip_transport_destroy(gloo_hip_transport_t t);
int gloo_hip_buffer_create(gloo_hip_transport_t t, int peer, int slot, void* ptr, size_t size, int is_send,
                           gloo_hip_buffer_t* out);
int gloo_hip_buffer_destroy(gloo_hip_buffer_t b);
int gloo_hip_buffer_send(gloo_hip_buffer_t b, size_t offset, size_t length, size_t roffset);
int gloo_hip_buffer_wait_recv(gloo_hip_buffer_t b);
int gloo_hip_buffer_wait_send(gloo_hip_buffer_t b);

/* Unbound buffers (gloo/transport/unbound_buffer.h:32-121) on the same
 * transport: two-sided send / recv matched per (source, slot) in order,
 * recv-from-any over `srcs`.  Sends are eager (the bytes are staged in node
 * shared memory at once, so waitSend never blocks); the receiver copies them
 * out in wait_recv.  Host or device memory.  nbytes = SIZE_MAX: the rest of
 * the buffer from offset.
 *   gloo_hip_ubuf_wait_recv / wait_send: 0 = done (*rank = the peer),
 *   1 = aborted (abort_wait_*), GLOO_HIP_EIO = timed out (timeout_ms < 0:
 *   the context's timeout). */
typedef struct gloo_hip_ubuf* gloo_hip_ubuf_t;
int gloo_hip_ubuf_create(gloo_hip_transport_t t, void* ptr, size_t size, gloo_hip_ubuf_t* out);
int gloo_hip_ubuf_destroy(gloo_hip_ubuf_t b);
int gloo_hip_ubuf_send(gloo_hip_ubuf_t b, int dst, uint64_t slot, size_t offset, size_t nbytes);
int gloo_hip_ubuf_recv(gloo_hip_ubuf_t b, const int* srcs, int nsrcs, uint64_t slot, size_t offset, size_t nbytes);
int gloo_hip_ubuf_wait_recv(gloo_hip_ubuf_t b, int* rank, int timeout_ms);
int gloo_hip_ubuf_wait_send(gloo_hip_ubuf_t b, int* rank, int timeout_ms);
int gloo_hip_ubuf_abort_wait_recv(gloo_hip_ubuf_t b);
int gloo_hip_ubuf_abort_wait_send(gloo_hip_ubuf_t b);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GLOO_AMD_H_ */
