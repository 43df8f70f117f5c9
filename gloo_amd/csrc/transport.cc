// transport.cc — see transport.h.
#include "gloo_amd/transport.h"

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <thread>

#include "gloo_amd.h"
#include "gloo_amd/common.h"
#include "gloo_amd/errors.h"
#include "gloo_amd/ipc.h"
#include "gloo_amd/signal.h"

namespace gloo_amd {
namespace transport {
namespace {

// What a receive buffer publishes for the peer that writes into it.
struct RecvRecord {
  int32_t pid;
  int32_t device;
  uint64_t ptr;     // the buffer itself (same process)
  uint64_t size;    // bytes the peer may write
  int32_t exported; // device memory shared as a dma-buf range (ipc.h exportRange): exportId / exportOffset
  int32_t host;     // host memory: written directly within one process, through `landing` across processes
  int32_t channel;  // this buffer's channel of the transport block
  int32_t pad;
  uint64_t exportId, exportOffset, incarnation;
  uint64_t baseline;  // the channel's arrival count when the buffer was created
  char landing[48];   // host memory: the landing segment a peer process writes messages into
  int32_t deviceLanding;  // device memory the runtime could not export: a landing slab (ipc.h) instead
  int32_t pad2;
  uint64_t landingSlab;
};

// A device receive buffer reached by a peer process: its allocation is
// exported as a dma-buf (ipc.h exportRange) and the sender maps the range
// into a virtual range of its own (VMM import) and writes in place — the
// reference's TCP pair writes any registered buffer the same way
// (gloo/transport/tcp/pair.cc:413-426).  Rounds 1-5 used hipIpc handles
// here, whose imports of 2 GiB or more hung in the runtime's open call
// (profiles/round3/r3t_*, r3u_*) and whose handles named a freed block's
// successor at the same address stale; a dma-buf names its block.  Should
// the runtime refuse the export, the buffer gets a LANDING slab of its own
// size from the cross-process pool instead (peer processes write their
// messages there and waitRecv copies each message's range into the buffer).

// Most workgroups one device-to-device message's copy kernel takes: a few
// dozen saturate an xGMI link (a link, not HBM, bounds a peer copy), a copy
// within one GPU's HBM takes more (the executor's defaults, executor.h).
constexpr unsigned kSendBlocks = 64;
constexpr unsigned kSendBlocksLocal = 256;

std::string recordKey(uint64_t inst, int sender, int receiver, uint64_t slot) {
  return strcat_("gloo_amd/xgmi/", inst, "/", sender, "->", receiver, "/", slot);
}

bool isDevice(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  const bool dev = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice;
  (void)hipGetLastError();
  return dev;
}

// Polls `done` with back-off until it holds, `abort` is set (returns false)
// or the deadline passes (IoException with `what`).
template <typename F>
bool pollUntil(F done, const std::atomic<bool>* abort, std::chrono::milliseconds timeout, const std::string& what) {
  const auto deadline = std::chrono::steady_clock::now() + timeout;
  for (uint64_t i = 0;; i++) {
    if (done()) return true;
    if (abort && abort->load(std::memory_order_acquire)) return false;
    if (i < 4096) {
      __builtin_ia32_pause();
    } else if (i < 8192) {
      sched_yield();
    } else {
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if ((i & 255) == 255 && std::chrono::steady_clock::now() > deadline)
      throw IoException(strcat_("Timed out ", what, " after ", timeout.count(), " ms"));
  }
}

std::atomic<uint64_t> g_staged{0};
std::atomic<uint64_t> g_landing{0};

// Transport blocks in pinned memory, between rank 0's allocation and the
// other ranks of the process taking their hold (Device::Device).
std::mutex g_pinnedMutex;
std::map<std::string, std::shared_ptr<void>> g_pinnedBlocks;

// A named node shared-memory segment of `bytes` (zero-filled, pages on first
// touch), mapped read-write.
void* createSegment(const std::string& name, size_t bytes) {
  const int fd = ::shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
  GLOO_AMD_ENFORCE(fd >= 0, "shm_open(create) failed for ", name);
  void* m = ::ftruncate(fd, (off_t)bytes) == 0 ? ::mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0)
                                               : MAP_FAILED;
  ::close(fd);
  if (m == MAP_FAILED) {
    ::shm_unlink(name.c_str());
    GLOO_AMD_ENFORCE(false, "landing segment of ", bytes, " B: ftruncate/mmap failed");
  }
  return m;
}

// An arrival published by the host, in stream order (SendBuffer::send).
struct Arrival {
  std::atomic<uint64_t>* count;
  uint64_t k;
};
void publishArrival(void* p) {
  Arrival* a = static_cast<Arrival*>(p);
  a->count->store(a->k, std::memory_order_release);
  delete a;
}

class SendBuffer : public Buffer {
 public:
  SendBuffer(Device* dev, int peer, uint64_t slot, void* ptr, size_t size)
      : Buffer(slot, ptr, size), dev_(dev), peer_(peer), srcDevice_(isDevice(ptr)) {
    dev_->claim(true, peer_, slot_);
    GLOO_AMD_HIP_CHECK(hipEventCreateWithFlags(&sent_, hipEventDisableTiming));
  }
  ~SendBuffer() override {
    (void)hipEventSynchronize(sent_);
    (void)hipEventDestroy(sent_);
    if (ticket_) GLOO_AMD_HIP_RELEASE(hipFree(ticket_));
    if (landingRegistered_) GLOO_AMD_HIP_RELEASE(hipHostUnregister(landing_));
    if (landing_) ::munmap(landing_, peerSize_);
    ipc::unimportRange(&imported_);
    if (landingImport_) ipc::unimport(landingImport_);
    dev_->release(true, peer_, slot_);
  }

  void send(size_t offset, size_t length, size_t roffset) override {
    Context& ctx = *dev_->context();
    GLOO_AMD_HIP_CHECK(hipSetDevice(ctx.device()));
    resolve();
    GLOO_AMD_ENFORCE(offset + length <= size_, "send of [", offset, ", +", length, ") beyond a ", size_,
                     "-byte send buffer");
    GLOO_AMD_ENFORCE(roffset + length <= peerSize_, "send of ", length, " bytes at ", roffset, " beyond rank ", peer_,
                     "'s ", peerSize_, "-byte receive buffer (slot ", slot_, ")");
    // this message's arrival number on the channel (from the
    // channel's line, not from this buffer's own count, so it continues
    // across send buffers of this slot while the receive buffer lives)
    const uint64_t k = channel_->sent.fetch_add(1, std::memory_order_acq_rel) + 1;
    hipStream_t s = dev_->stream();
    const char* src = ptr_ + offset;
    char* dst = nullptr;
    if (viaLanding_) {
      // a buffer of another process reached through its landing segment or
      // slab: the message lands there, described by the record of its
      // arrival number, which must be free
      Device::MsgRecord& rec = dev_->msgRecord(ctx.rank, peer_, channelIdx_, k);
      pollUntil(
          [&] {
            const uint64_t q = rec.seq.load(std::memory_order_acquire);
            return q == 0 || rec.ack.load(std::memory_order_acquire) == q;
          },
          nullptr, ctx.timeout(),
          strcat_("waiting for rank ", peer_, " to consume ", kMsgRing, " earlier messages (slot ", slot_, ")"));
      rec.off = roffset;
      rec.len = length;
      rec.seq.store(k, std::memory_order_release);  // read only once the arrival count reaches k
      dst = (landing_ ? landing_ : remote_) + roffset;
    } else if (remote_) {
      dst = remote_ + roffset;
    }
    if (!srcDevice_ && !dstDevice_) {
      // host to host (or a notification from host memory): the sending
      // thread writes and publishes; nothing of this buffer is on the stream
      if (length) std::memcpy(dst, src, length);
      channel_->count.store(k, std::memory_order_release);
      return;
    }
    // (arrivals are published from the device: 9.1 us one way at 1 KiB
    // against 26.4 us through a stream host function)
    if (!channelDev_) {
      // the GPU cannot address the block the processes share: the bytes move
      // by a stream-ordered copy and a host function behind it publishes the
      // arrival (the executor's host-signalled SENDs do the same)
      if (length) GLOO_AMD_HIP_CHECK(hipMemcpyAsync(dst, src, length, hipMemcpyDefault, s));
      auto* a = new Arrival{&channel_->count, k};
      const hipError_t e = hipLaunchHostFunc(s, publishArrival, a);
      if (e != hipSuccess) delete a;
      GLOO_AMD_HIP_CHECK(e);
    } else if (srcDevice_ && dstDevice_ && length) {
      // device to device: one copy kernel, the arrival published by its last workgroup
      checkRc(launchCopySignal(dst, src, length, channelDev_, Seq{k, 0}, ticket_, nullptr,
                               copySignalGrid(length, sameGpu_ ? kSendBlocksLocal : kSendBlocks), s),
              "transport copy_signal_kernel");
    } else {
      if (length) GLOO_AMD_HIP_CHECK(hipMemcpyAsync(dst, src, length, hipMemcpyDefault, s));
      // stream-ordered: the arrival is published once the bytes landed
      GLOO_AMD_HIP_CHECK(launchSignal(channelDev_, Seq{k, 0}, nullptr, s));
    }
    GLOO_AMD_HIP_CHECK(hipEventRecord(sent_, s));
  }
  void waitRecv() override { throw EnforceNotMet("waitRecv on a send buffer"); }
  void waitSend() override { GLOO_AMD_HIP_CHECK(hipEventSynchronize(sent_)); }

 private:
  static void checkRc(int rc, const char* what) {
    GLOO_AMD_ENFORCE(rc == GLOO_HIP_OK, what, ": ", gloo_hip_last_error());
  }

  // The peer's receive buffer of this slot (published when it was created).
  void resolve() {
    if (resolved_) return;
    Context& ctx = *dev_->context();
    const auto v = ctx.store().get(recordKey(dev_->instance(), ctx.rank, peer_, slot_), ctx.timeout());
    GLOO_AMD_ENFORCE(v.size() == sizeof(RecvRecord), "bad receive-buffer record from rank ", peer_);
    RecvRecord r;
    std::memcpy(&r, v.data(), sizeof(r));
    peerSize_ = r.size;
    channelIdx_ = r.channel;
    channel_ = &dev_->channel(ctx.rank, peer_, r.channel);
    sameGpu_ = r.device == ctx.device();
    if (r.size == 0) {
      remote_ = nullptr;  // a notification buffer: arrivals only
    } else if (r.pid == ctx.pid()) {
      remote_ = reinterpret_cast<char*>(r.ptr);
      dstDevice_ = !r.host;
      if (!r.host && r.device != ctx.device()) {
        hipError_t e = hipDeviceEnablePeerAccess(r.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) GLOO_AMD_HIP_CHECK(e);
        (void)hipGetLastError();
      }
    } else if (r.host) {
      // host memory of another process: its landing segment, registered for
      // the device's copies when this buffer's bytes are device memory
      r.landing[sizeof(r.landing) - 1] = 0;
      const int fd = ::shm_open(r.landing, O_RDWR, 0600);
      GLOO_AMD_ENFORCE(fd >= 0, "shm_open failed for rank ", peer_, "'s landing segment ", r.landing);
      void* m = ::mmap(nullptr, r.size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
      ::close(fd);
      GLOO_AMD_ENFORCE(m != MAP_FAILED, "mmap of rank ", peer_, "'s landing segment failed");
      landing_ = static_cast<char*>(m);
      viaLanding_ = true;
      if (srcDevice_) {
        // (pinned where the system allows: the copies go through the runtime's
        // staging otherwise)
        hipError_t e;
        {
          std::lock_guard<std::mutex> allocLock(HipShared::getMutex());
          e = hipHostRegister(landing_, r.size, hipHostRegisterPortable);
        }
        landingRegistered_ = e == hipSuccess;
        if (!landingRegistered_) (void)hipGetLastError();
      }
    } else if (r.exported) {
      // device memory of another process: its dma-buf range, mapped here
      // once per send buffer (eager copies only, never captured into a
      // graph), unmapped when the send buffer goes
      ipc::Remote rm;
      rm.pid = r.pid;
      rm.incarnation = r.incarnation;
      rm.id = r.exportId;
      imported_ = ipc::importRange(rm, r.exportOffset, r.size, ctx.device());
      remote_ = imported_.ptr;
      dstDevice_ = true;
    } else {
      // device memory the peer's runtime could not export: its landing slab
      GLOO_AMD_ENFORCE(r.deviceLanding, "rank ", peer_, "'s receive buffer (slot ", slot_,
                       ") is device memory with neither an export nor a landing slab");
      ipc::Remote rm;
      rm.pid = r.pid;
      rm.incarnation = r.incarnation;
      rm.id = r.landingSlab;
      landingImport_ = static_cast<char*>(ipc::import(rm, r.size, ctx.device()));
      remote_ = landingImport_;
      viaLanding_ = true;
      dstDevice_ = true;
    }
    if (srcDevice_ || dstDevice_) {
      channelDev_ = dev_->channelDevicePtr(ctx.rank, peer_, r.channel);
      if (channelDev_ && srcDevice_ && dstDevice_) {
        GLOO_AMD_HIP_ALLOC(hipMalloc(reinterpret_cast<void**>(&ticket_), sizeof(unsigned)));
        // zeroed on the transport's stream, ahead of the first copy kernel: a
        // plain hipMemset goes to the null stream, which a non-blocking
        // stream does not wait for (a late zero lost a ticket and the
        // arrival with it: transport_test device_ring_chunked/P5, r5b)
        GLOO_AMD_HIP_CHECK(hipMemsetAsync(ticket_, 0, sizeof(unsigned), dev_->stream()));
      }
    }
    resolved_ = true;
  }

  Device* dev_;
  int peer_;
  const bool srcDevice_;   // this buffer is device memory
  bool dstDevice_ = false; // the peer's buffer is device memory (its bytes move on the device)
  bool sameGpu_ = false;   // ... on this rank's own GPU
  bool resolved_ = false;
  char* remote_ = nullptr;
  char* landing_ = nullptr;         // a host buffer's landing segment (mapped here)
  bool landingRegistered_ = false;
  char* landingImport_ = nullptr;   // a device buffer's landing slab (imported)
  bool viaLanding_ = false;         // messages go through a landing area, with records
  ipc::RangeImport imported_;       // a device buffer of another process, mapped here
  size_t peerSize_ = 0;
  int channelIdx_ = -1;
  Device::Channel* channel_ = nullptr;
  uint64_t* channelDev_ = nullptr;
  unsigned* ticket_ = nullptr;
  hipEvent_t sent_ = nullptr;
};

class RecvBuffer : public Buffer {
 public:
  RecvBuffer(Device* dev, int peer, uint64_t slot, void* ptr, size_t size)
      : Buffer(slot, ptr, size), dev_(dev), peer_(peer) {
    Context& ctx = *dev_->context();
    dev_->claim(false, peer_, slot_);
    idx_ = dev_->allocChannel(peer_);
    channel_ = &dev_->channel(peer_, ctx.rank, idx_);
    // baseline before the record is published, i.e. before the peer's
    // first send can land (the sender resolves the record first)
    baseline_ = channel_->count.load(std::memory_order_acquire);
    channel_->sent.store(baseline_, std::memory_order_release);
    // message records an earlier buffer of this channel left unconsumed are
    // released, so the peer's sends here never wait for them
    for (int i = 0; i < kMsgRing; i++) {
      Device::MsgRecord& rec = dev_->msgRecord(peer_, ctx.rank, idx_, (uint64_t)i);
      rec.ack.store(rec.seq.load(std::memory_order_acquire), std::memory_order_release);
    }
    RecvRecord r;
    std::memset(&r, 0, sizeof(r));
    r.pid = ctx.pid();
    r.device = ctx.device();
    r.ptr = reinterpret_cast<uint64_t>(ptr_);
    r.size = ptr_ ? size_ : 0;
    r.channel = idx_;
    r.baseline = baseline_;
    if (ptr_ && size_) {
      r.incarnation = ipc::incarnation();
      if (isDevice(ptr_)) {
        ipc::RangeExport ex;
        if (ipc::exportRange(ptr_, size_, &ex)) {
          export_ = ex;
          r.exported = 1;
          r.exportId = ex.id;
          r.exportOffset = ex.offset;
        } else {
          deviceLanding_ = ipc::acquire(ctx.device(), size_, true);
          r.deviceLanding = 1;
          r.landingSlab = deviceLanding_->id;
        }
      } else {
        r.host = 1;
        host_ = true;
        // where a sender in another process writes (pages only once touched)
        landingName_ = strcat_("/glr_", ctx.pid(), "_", ++g_landing);
        landing_ = static_cast<char*>(createSegment(landingName_, size_));
        std::snprintf(r.landing, sizeof(r.landing), "%s", landingName_.c_str());
      }
      (void)hipGetLastError();
    }
    std::vector<char> blob(sizeof(r));
    std::memcpy(blob.data(), &r, sizeof(r));
    ctx.store().set(recordKey(dev_->instance(), peer_, ctx.rank, slot_), blob);
  }
  ~RecvBuffer() override {
    ipc::unexportRange(export_);
    if (deviceLanding_) ipc::release(deviceLanding_);
    if (landing_) {
      ::munmap(landing_, size_);
      ::shm_unlink(landingName_.c_str());
    }
    dev_->freeChannel(peer_, idx_);
    dev_->release(false, peer_, slot_);
  }

  void send(size_t, size_t, size_t) override { throw EnforceNotMet("send on a receive buffer"); }
  void waitSend() override {}
  void waitRecv() override {
    Context& ctx = *dev_->context();
    const uint64_t target = baseline_ + ++received_;
    pollUntil([&] { return (int64_t)(channel_->count.load(std::memory_order_acquire) - target) >= 0; }, nullptr,
              ctx.timeout(), strcat_("waiting for rank ", peer_, " (slot ", slot_, ") on rank ", ctx.rank));
    if (deviceLanding_) {
      // a sender in another process wrote into the landing slab and described
      // the message in the record of this arrival (one in this process wrote
      // in place: no record carries this arrival number then)
      Device::MsgRecord& rec = dev_->msgRecord(peer_, ctx.rank, idx_, target);
      if (rec.seq.load(std::memory_order_acquire) != target) return;
      const uint64_t off = rec.off, len = rec.len;
      GLOO_AMD_ENFORCE(off + len <= size_, "message of ", len, " B at ", off, " beyond the ", size_,
                       "-byte receive buffer");
      if (len) {
        GLOO_AMD_HIP_CHECK(hipSetDevice(ctx.device()));
        GLOO_AMD_HIP_CHECK(hipMemcpyAsync(ptr_ + off, deviceLanding_->ptr + off, len, hipMemcpyDeviceToDevice,
                                          dev_->stream()));
        GLOO_AMD_HIP_CHECK(hipStreamSynchronize(dev_->stream()));
      }
      rec.ack.store(target, std::memory_order_release);
      return;
    }
    if (!host_) return;  // device memory: always written in place
    // A host buffer's sender in another process wrote the bytes into the
    // landing segment and described them in the record of this arrival; one
    // in this process wrote them in place (no record carries this arrival
    // number then).
    Device::MsgRecord& rec = dev_->msgRecord(peer_, ctx.rank, idx_, target);
    if (rec.seq.load(std::memory_order_acquire) != target) return;
    const uint64_t off = rec.off, len = rec.len;
    GLOO_AMD_ENFORCE(off + len <= size_, "message of ", len, " B at ", off, " beyond the ", size_,
                     "-byte receive buffer");
    if (len) std::memcpy(ptr_ + off, landing_ + off, len);
    rec.ack.store(target, std::memory_order_release);
  }

 private:
  Device* dev_;
  int peer_;
  bool host_ = false;
  int idx_ = -1;
  Device::Channel* channel_ = nullptr;
  uint64_t baseline_ = 0, received_ = 0;
  std::string landingName_;
  char* landing_ = nullptr;
  ipc::Slab* deviceLanding_ = nullptr;  // device memory the runtime could not export: where peer processes write
  ipc::RangeExport export_;             // device memory: the dma-buf range peer processes map
};

}  // namespace

// ---- Device ------------------------------------------------------------

Device::Device(std::shared_ptr<Context> ctx, hipStream_t stream) : ctx_(std::move(ctx)) {
  GLOO_AMD_HIP_CHECK(hipSetDevice(ctx_->device()));
  inst_ = ctx_->acquireInstance();
  if (stream) {
    stream_ = stream;
  } else {
    GLOO_AMD_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    ownStream_ = true;
  }
  const size_t P = (size_t)ctx_->size;
  blockBytes_ = 4096 + P * P * kChannels * sizeof(Channel) + P * P * kAnnouncements * sizeof(Announcement) + P * 64 +
                P * P * kChannels * kMsgRing * sizeof(MsgRecord);
  blockBytes_ = (blockBytes_ + 4095) / 4096 * 4096;
  // Ranks of ONE process share a block of pinned host memory by its address
  // (hipHostMalloc: the GPU addresses it from the start).  Ranks of several
  // processes share a named segment, which channelDevicePtr registers with
  // HIP where the system can pin memory a process already has mapped.
  const int32_t pid = ctx_->pid();
  const char* pidBytes = reinterpret_cast<const char*>(&pid);
  const auto pids = ctx_->allgather(strcat_("tdev", inst_, "/pid"), std::vector<char>(pidBytes, pidBytes + sizeof(pid)));
  for (const auto& v : pids)
    if (v.size() != sizeof(pid) || std::memcmp(v.data(), &pid, sizeof(pid)) != 0) blockPinned_ = false;
  if (!blockPinned_) (void)ctx_->agreeOnSharing();  // before the first receive buffer's export or landing slab
  std::string name;
  if (ctx_->rank == 0 && blockPinned_) {
    void* m = nullptr;
    GLOO_AMD_HIP_ALLOC(hipHostMalloc(&m, blockBytes_, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
    std::memset(m, 0, blockBytes_);
    blockHold_ = std::shared_ptr<void>(m, [](void* q) { GLOO_AMD_HIP_RELEASE(hipHostFree(q)); });
    name = strcat_(reinterpret_cast<uintptr_t>(m));
    std::lock_guard<std::mutex> lk(g_pinnedMutex);
    g_pinnedBlocks[name] = blockHold_;
  } else if (ctx_->rank == 0) {
    std::random_device rd;
    name = strcat_("/gloo_amd_t_", ctx_->pid(), "_", rd(), rd());
    const int fd = ::shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    GLOO_AMD_ENFORCE(fd >= 0, "shm_open(create) failed for ", name);
    const bool ok = ::ftruncate(fd, (off_t)blockBytes_) == 0;  // zero-filled
    block_ = ok ? ::mmap(nullptr, blockBytes_, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
    ::close(fd);
    GLOO_AMD_ENFORCE(block_ != MAP_FAILED, "transport block: ftruncate/mmap failed");
  }
  const auto names = ctx_->allgather(strcat_("tdev", inst_, "/block"),
                                     ctx_->rank == 0 ? std::vector<char>(name.begin(), name.end())
                                                     : std::vector<char>{});
  if (blockPinned_) {
    name.assign(names[0].begin(), names[0].end());
    {
      std::lock_guard<std::mutex> lk(g_pinnedMutex);
      auto it = g_pinnedBlocks.find(name);
      if (it != g_pinnedBlocks.end()) blockHold_ = it->second;  // held until this rank's transport goes
    }
    GLOO_AMD_ENFORCE(blockHold_ != nullptr, "transport block: rank 0's pinned block is not in this process");
    block_ = blockHold_.get();
    GLOO_AMD_HIP_CHECK(hipHostGetDevicePointer(&blockDev_, block_, 0));
  } else if (ctx_->rank != 0) {
    name.assign(names[0].begin(), names[0].end());
    const int fd = ::shm_open(name.c_str(), O_RDWR, 0600);
    GLOO_AMD_ENFORCE(fd >= 0, "shm_open failed for ", name);
    block_ = ::mmap(nullptr, blockBytes_, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    GLOO_AMD_ENFORCE(block_ != MAP_FAILED, "transport block: mmap failed");
  }
  ctx_->barrier(strcat_("tdev", inst_, "/mapped"));
  if (ctx_->rank == 0 && blockPinned_) {
    std::lock_guard<std::mutex> lk(g_pinnedMutex);
    g_pinnedBlocks.erase(name);  // every rank holds it now
  } else if (ctx_->rank == 0) {
    ::shm_unlink(name.c_str());  // every rank has it mapped now
  }
  channelUsed_.assign(P, std::vector<bool>(kChannels, false));
}

Device::~Device() {
  pairs_.clear();
  if (stream_) (void)hipStreamSynchronize(stream_);
  if (ownStream_) (void)hipStreamDestroy(stream_);
  if (block_) {
    // staged messages nobody took: their segments go with the transport
    for (int dst = 0; dst < ctx_->size; dst++)
      for (int i = 0; i < kAnnouncements; i++) {
        Announcement& a = announcement(ctx_->rank, dst, i);
        uint32_t ready = 2;
        if (a.state.compare_exchange_strong(ready, 3) && a.name[0]) ::shm_unlink(a.name);
      }
    if (blockPinned_) {
      blockHold_.reset();  // freed with the last rank's transport
    } else {
      if (blockDev_) GLOO_AMD_HIP_RELEASE(hipHostUnregister(block_));
      ::munmap(block_, blockBytes_);
    }
  }
  ctx_->releaseInstance(inst_);
}

Pair& Device::getPair(int peer) {
  GLOO_AMD_ENFORCE(peer >= 0 && peer < ctx_->size && peer != ctx_->rank, "no pair to rank ", peer);
  std::lock_guard<std::mutex> lk(m_);
  auto& p = pairs_[peer];
  if (!p) p.reset(new Pair(this, peer));
  return *p;
}

void Device::claim(bool send, int peer, uint64_t slot) {
  std::lock_guard<std::mutex> lk(m_);
  GLOO_AMD_ENFORCE(live_.insert(std::make_tuple(send, peer, slot)).second, "slot ", slot, " already has a live ",
                   send ? "send" : "receive", " buffer to/from rank ", peer);
}

void Device::release(bool send, int peer, uint64_t slot) {
  std::lock_guard<std::mutex> lk(m_);
  live_.erase(std::make_tuple(send, peer, slot));
}

Device::Channel& Device::channel(int src, int dst, int idx) {
  const size_t P = (size_t)ctx_->size;
  GLOO_AMD_ENFORCE(idx >= 0 && idx < kChannels, "bad channel ", idx);
  auto* base = reinterpret_cast<Channel*>(static_cast<char*>(block_) + 4096);
  return base[((size_t)src * P + (size_t)dst) * kChannels + (size_t)idx];
}

Device::Announcement& Device::announcement(int src, int dst, int idx) {
  const size_t P = (size_t)ctx_->size;
  auto* base = reinterpret_cast<Announcement*>(static_cast<char*>(block_) + 4096 + P * P * kChannels * sizeof(Channel));
  return base[((size_t)src * P + (size_t)dst) * kAnnouncements + (size_t)idx];
}

std::atomic<uint64_t>& Device::orderCounter(int dst) {
  const size_t P = (size_t)ctx_->size;
  char* p = static_cast<char*>(block_) + 4096 + P * P * kChannels * sizeof(Channel) +
            P * P * kAnnouncements * sizeof(Announcement) + (size_t)dst * 64;
  return *reinterpret_cast<std::atomic<uint64_t>*>(p);
}

Device::MsgRecord& Device::msgRecord(int src, int dst, int idx, uint64_t k) {
  const size_t P = (size_t)ctx_->size;
  GLOO_AMD_ENFORCE(idx >= 0 && idx < kChannels, "bad channel ", idx);
  auto* base = reinterpret_cast<MsgRecord*>(static_cast<char*>(block_) + 4096 + P * P * kChannels * sizeof(Channel) +
                                            P * P * kAnnouncements * sizeof(Announcement) + P * 64);
  return base[(((size_t)src * P + (size_t)dst) * kChannels + (size_t)idx) * kMsgRing + (size_t)(k % kMsgRing)];
}

uint64_t* Device::channelDevicePtr(int src, int dst, int idx) {
  {
    std::lock_guard<std::mutex> lk(m_);
    if (blockUnpinnable_) return nullptr;
    if (!blockDev_) {
      hipError_t e;
      {
        std::lock_guard<std::mutex> allocLock(HipShared::getMutex());
        e = hipHostRegister(block_, blockBytes_, hipHostRegisterMapped | hipHostRegisterPortable);
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();  // (a failed registration otherwise shows up at the next launch)
        blockUnpinnable_ = true;
        return nullptr;
      }
      void* d = nullptr;
      GLOO_AMD_HIP_CHECK(hipHostGetDevicePointer(&d, block_, 0));
      blockDev_ = d;
    }
  }
  const size_t off = reinterpret_cast<char*>(&channel(src, dst, idx).count) - static_cast<char*>(block_);
  return reinterpret_cast<uint64_t*>(static_cast<char*>(blockDev_) + off);
}

int Device::allocChannel(int src) {
  std::lock_guard<std::mutex> lk(m_);
  auto& used = channelUsed_.at((size_t)src);
  for (int i = 0; i < kChannels; i++)
    if (!used[i]) {
      used[i] = true;
      return i;
    }
  GLOO_AMD_ENFORCE(false, "more than ", kChannels, " live receive buffers from rank ", src);
  return -1;
}

void Device::freeChannel(int src, int idx) {
  std::lock_guard<std::mutex> lk(m_);
  if (idx >= 0) channelUsed_.at((size_t)src)[(size_t)idx] = false;
}

void Device::announce(int dst, uint64_t slot, const void* ptr, size_t n) {
  GLOO_AMD_ENFORCE(dst >= 0 && dst < ctx_->size, "no rank ", dst);
  char name[32] = {0};
  if (n) {
    std::snprintf(name, sizeof(name), "/gla_%d_%llu", ctx_->pid(), (unsigned long long)++g_staged);
    const int fd = ::shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
    GLOO_AMD_ENFORCE(fd >= 0, "shm_open(create) failed for ", name);
    void* m = ::ftruncate(fd, (off_t)n) == 0 ? ::mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0)
                                             : MAP_FAILED;
    ::close(fd);
    if (m == MAP_FAILED) {
      ::shm_unlink(name);
      GLOO_AMD_ENFORCE(false, "staging ", n, " bytes failed");
    }
    if (isDevice(ptr)) {
      const hipError_t e = hipMemcpy(m, ptr, n, hipMemcpyDeviceToHost);
      if (e != hipSuccess) {
        ::munmap(m, n);
        ::shm_unlink(name);
        GLOO_AMD_HIP_CHECK(e);
      }
    } else {
      std::memcpy(m, ptr, n);
    }
    ::munmap(m, n);
  }
  // a free entry of the (me -> dst) queue (the receiver frees them as it takes)
  Announcement* a = nullptr;
  pollUntil(
      [&] {
        for (int i = 0; i < kAnnouncements; i++) {
          Announcement& x = announcement(ctx_->rank, dst, i);
          uint32_t fr = 0;
          if (x.state.load(std::memory_order_relaxed) == 0 && x.state.compare_exchange_strong(fr, 1)) {
            a = &x;
            return true;
          }
        }
        return false;
      },
      nullptr, ctx_->timeout(), strcat_("waiting for rank ", dst, " to take ", kAnnouncements, " messages"));
  a->slot = slot;
  a->nbytes = n;
  std::memcpy(a->name, name, sizeof(a->name));
  a->order = orderCounter(dst).fetch_add(1, std::memory_order_acq_rel);
  a->state.store(2, std::memory_order_release);
}

bool Device::take(const std::vector<int>& srcs, uint64_t slot, void* dst, size_t n, int* src) {
  const int me = ctx_->rank;
  for (;;) {
    Announcement* best = nullptr;
    int bestSrc = -1;
    for (int s : srcs) {
      GLOO_AMD_ENFORCE(s >= 0 && s < ctx_->size && s != me, "bad source rank ", s);
      for (int i = 0; i < kAnnouncements; i++) {
        Announcement& a = announcement(s, me, i);
        if (a.state.load(std::memory_order_acquire) != 2 || a.slot != slot) continue;
        if (!best || a.order < best->order) {
          best = &a;
          bestSrc = s;
        }
      }
    }
    if (!best) return false;
    uint32_t ready = 2;
    if (!best->state.compare_exchange_strong(ready, 3)) continue;  // another thread of this rank took it
    const size_t nbytes = best->nbytes;
    char name[32];
    std::memcpy(name, best->name, sizeof(name));
    if (nbytes != n) {
      best->state.store(2, std::memory_order_release);  // leave it for a receive of the right size
      GLOO_AMD_ENFORCE(false, "rank ", bestSrc, " sent ", nbytes, " bytes on slot ", slot, " to a ", n,
                       "-byte receive");
    }
    if (nbytes) {
      const int fd = ::shm_open(name, O_RDONLY, 0600);
      GLOO_AMD_ENFORCE(fd >= 0, "shm_open failed for ", name);
      void* m = ::mmap(nullptr, nbytes, PROT_READ, MAP_SHARED, fd, 0);
      ::close(fd);
      GLOO_AMD_ENFORCE(m != MAP_FAILED, "mmap of a staged message failed");
      hipError_t e = hipSuccess;
      if (isDevice(dst)) {
        e = hipMemcpy(dst, m, nbytes, hipMemcpyHostToDevice);
      } else {
        std::memcpy(dst, m, nbytes);
      }
      ::munmap(m, nbytes);
      ::shm_unlink(name);
      GLOO_AMD_HIP_CHECK(e);
    }
    best->state.store(0, std::memory_order_release);
    *src = bestSrc;
    return true;
  }
}

// ---- Pair / UnboundBuffer ----------------------------------------------

std::unique_ptr<Buffer> Pair::createSendBuffer(uint64_t slot, void* ptr, size_t size) {
  return std::unique_ptr<Buffer>(new SendBuffer(dev_, peer_, slot, ptr, size));
}

std::unique_ptr<Buffer> Pair::createRecvBuffer(uint64_t slot, void* ptr, size_t size) {
  return std::unique_ptr<Buffer>(new RecvBuffer(dev_, peer_, slot, ptr, size));
}

void UnboundBuffer::send(int dst, uint64_t slot, size_t offset, size_t nbytes) {
  if (nbytes == std::numeric_limits<size_t>::max()) nbytes = offset <= size_ ? size_ - offset : 0;
  // an empty message may name any offset (BCUBE sends empty chunks past the
  // end of short buffers, gloo/allreduce.cc:466-503)
  GLOO_AMD_ENFORCE(nbytes == 0 || offset + nbytes <= size_, "send of [", offset, ", +", nbytes, ") beyond a ",
                   size_, "-byte buffer");
  GLOO_AMD_ENFORCE(dst != dev_->context()->rank, "send to self");
  dev_->announce(dst, slot, ptr_ + offset, nbytes);
  sent_.push_back(dst);
}

void UnboundBuffer::recv(const std::vector<int>& srcs, uint64_t slot, size_t offset, size_t nbytes) {
  if (nbytes == std::numeric_limits<size_t>::max()) nbytes = offset <= size_ ? size_ - offset : 0;
  GLOO_AMD_ENFORCE(nbytes == 0 || offset + nbytes <= size_, "recv of [", offset, ", +", nbytes, ") beyond a ",
                   size_, "-byte buffer");
  GLOO_AMD_ENFORCE(!srcs.empty(), "recv from no rank");
  recvs_.push_back({srcs, slot, offset, nbytes});
}

bool UnboundBuffer::waitRecv(int* rank, std::chrono::milliseconds timeout) {
  Context& ctx = *dev_->context();
  GLOO_AMD_ENFORCE(!recvs_.empty(), "waitRecv without a pending recv");
  if (timeout.count() < 0) timeout = ctx.timeout();
  int src = -1;
  // Receives on one slot from overlapping sources complete in the order they
  // were posted: a receive is tried only when no earlier pending receive
  // could take the same message (else a message arriving between two tries
  // would land in the later receive's place).
  auto blocked = [&](std::deque<PendingRecv>::iterator it) {
    for (auto e = recvs_.begin(); e != it; ++e) {
      if (e->slot != it->slot) continue;
      for (int a : e->srcs)
        for (int b : it->srcs)
          if (a == b) return true;
    }
    return false;
  };
  const bool done = pollUntil(
      [&] {
        for (auto it = recvs_.begin(); it != recvs_.end(); ++it)
          if (!blocked(it) && dev_->take(it->srcs, it->slot, ptr_ + it->offset, it->nbytes, &src)) {
            recvs_.erase(it);
            return true;
          }
        return false;
      },
      &abortRecv_, timeout, strcat_("waiting for a message on rank ", ctx.rank));
  if (!done) {
    abortRecv_ = false;
    return false;
  }
  if (rank) *rank = src;
  return true;
}

bool UnboundBuffer::waitSend(int* rank, std::chrono::milliseconds) {
  // sends are eager: each completed when send() returned
  if (abortSend_.exchange(false)) return false;
  GLOO_AMD_ENFORCE(!sent_.empty(), "waitSend without a pending send");
  if (rank) *rank = sent_.front();
  sent_.pop_front();
  return true;
}

}  // namespace transport
}  // namespace gloo_amd
