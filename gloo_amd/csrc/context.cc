// context.cc — see context.h.
#include "gloo_amd/context.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <random>

#include "gloo_amd.h"
#include "gloo_amd/common.h"
#include "gloo_amd/ipc.h"

#include <hip/hip_runtime_api.h>

namespace gloo_amd {

namespace {
struct ShmHeader {
  uint64_t magic;
  uint64_t size;
  uint64_t slots;
  uint64_t pad;
};
constexpr uint64_t kMagic = 0x676c6f6f5f616d64ull;  // "gloo_amd"

std::vector<char> bytes(const std::string& s) { return std::vector<char>(s.begin(), s.end()); }
}  // namespace

Context::Context(int r, int s, std::chrono::milliseconds timeout)
    : rank(r), size(s), timeout_(timeout), pid_((int)::getpid()) {
  GLOO_AMD_ENFORCE(size >= 1 && rank >= 0 && rank < size, "bad rank ", rank, " / size ", size);
}

Context::~Context() {
  if (shmDev_) GLOO_AMD_HIP_RELEASE(hipHostUnregister(shm_));
  if (shm_) ::munmap(shm_, shmBytes_);
  if (errorWords_.load()) GLOO_AMD_HIP_RELEASE(hipHostFree(errorWords_.load()));
}

void Context::connect(std::shared_ptr<Store> store, int device) {
  store_ = std::move(store);
  device_ = device;
  countersBytes_ = kMaxLiveInstances * (size_t)size * size * GLOO_HIP_NUM_SLOTS * sizeof(uint64_t);
  shmBytes_ = sizeof(ShmHeader) + countersBytes_;
  shmBytes_ = (shmBytes_ + 4095) / 4096 * 4096;
  if (rank == 0) {
    std::random_device rd;
    shmName_ = strcat_("/gloo_amd_", pid_, "_", rd(), rd());
    int fd = ::shm_open(shmName_.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    GLOO_AMD_ENFORCE(fd >= 0, "shm_open(create) failed for ", shmName_);
    GLOO_AMD_ENFORCE(::ftruncate(fd, (off_t)shmBytes_) == 0, "ftruncate failed");
    shm_ = ::mmap(nullptr, shmBytes_, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    GLOO_AMD_ENFORCE(shm_ != MAP_FAILED, "mmap failed");
    auto* h = static_cast<ShmHeader*>(shm_);
    h->size = size;
    h->slots = GLOO_HIP_NUM_SLOTS;
    std::atomic_thread_fence(std::memory_order_release);
    h->magic = kMagic;
  }
  // rank 0 publishes the control block's name
  const auto names = allgather("shm", rank == 0 ? bytes(shmName_) : std::vector<char>{});
  if (rank != 0) {
    shmName_.assign(names[0].begin(), names[0].end());
    int fd = ::shm_open(shmName_.c_str(), O_RDWR, 0600);
    GLOO_AMD_ENFORCE(fd >= 0, "shm_open failed for ", shmName_);
    shm_ = ::mmap(nullptr, shmBytes_, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    GLOO_AMD_ENFORCE(shm_ != MAP_FAILED, "mmap failed");
    auto* h = static_cast<ShmHeader*>(shm_);
    GLOO_AMD_ENFORCE(h->magic == kMagic && (int)h->size == size, "control block mismatch");
  }
  barrier("connect");
  if (rank == 0) ::shm_unlink(shmName_.c_str());  // every rank has it mapped now
}

std::atomic<uint64_t>& Context::counter(uint64_t inst, int src, int dst, int slot) {
  GLOO_AMD_ENFORCE(shm_ != nullptr, "context not connected");
  auto* base = reinterpret_cast<std::atomic<uint64_t>*>(static_cast<char*>(shm_) + sizeof(ShmHeader));
  const size_t i = (((inst % kMaxLiveInstances) * size + src) * size + dst) * GLOO_HIP_NUM_SLOTS + slot;
  return base[i];
}

void Context::ensureDeviceMapped() {
  std::lock_guard<std::mutex> lk(mapMutex_);
  if (shmDev_) return;
  // The control block is memory this process already has mapped, which not
  // every system lets HIP pin (virtual machines refuse it).  Only a device
  // signal to or from a rank without a device mailbox needs it (executor.h).
  hipError_t e;
  {
    std::lock_guard<std::mutex> allocLock(HipShared::getMutex());
    e = hipHostRegister(shm_, shmBytes_, hipHostRegisterMapped | hipHostRegisterPortable);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();  // (a failed registration otherwise shows up at the next launch)
    throw EnforceNotMet(strcat_("rank ", rank, ": this system cannot pin the node's shared control block for the GPU "
                                "(hipHostRegister: ", hipGetErrorString(e), "), which device-side signalling between "
                                "a rank that waits on the host and a rank that waits on the device needs"));
  }
  void* d = nullptr;
  GLOO_AMD_HIP_CHECK(hipHostGetDevicePointer(&d, shm_, 0));
  shmDev_ = d;
}

uint64_t* Context::counterDevicePtr(uint64_t inst, int src, int dst, int slot) {
  ensureDeviceMapped();
  const size_t off = reinterpret_cast<char*>(&counter(inst, src, dst, slot)) - static_cast<char*>(shm_);
  return reinterpret_cast<uint64_t*>(static_cast<char*>(shmDev_) + off);
}

// The error words are this rank's own: its device-side waits write them and
// its host reads them, so they live in pinned memory of this process.
void Context::ensureErrorWords() {
  if (errorWords_.load(std::memory_order_acquire)) return;  // (every call after the first: no lock)
  std::lock_guard<std::mutex> lk(mapMutex_);
  if (errorWords_.load(std::memory_order_relaxed)) return;
  const size_t bytes = ((size_t)size * sizeof(uint32_t) + 63) / 64 * 64;
  void* h = nullptr;
  GLOO_AMD_HIP_ALLOC(hipHostMalloc(&h, bytes, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
  std::memset(h, 0, bytes);
  void* d = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    GLOO_AMD_HIP_RELEASE(hipHostFree(h));
    GLOO_AMD_HIP_CHECK(e);
  }
  errorWordsDev_ = d;
  errorWords_.store(h, std::memory_order_release);
}

std::atomic<uint32_t>& Context::errorWord(int r) {
  GLOO_AMD_ENFORCE(r >= 0 && r < size, "no rank ", r);
  ensureErrorWords();
  return static_cast<std::atomic<uint32_t>*>(errorWords_.load(std::memory_order_relaxed))[r];
}

uint32_t* Context::errorWordDevicePtr(int r) {
  GLOO_AMD_ENFORCE(r >= 0 && r < size, "no rank ", r);
  ensureErrorWords();
  return static_cast<uint32_t*>(errorWordsDev_) + r;
}

uint64_t Context::acquireInstance() {
  const uint64_t inst = nextInstance();
  std::lock_guard<std::mutex> lk(liveMutex_);
  GLOO_AMD_ENFORCE(live_.insert(inst % kMaxLiveInstances).second, "more than ", kMaxLiveInstances,
                   " live algorithm instances on one context");
  return inst;
}

void Context::releaseInstance(uint64_t inst) {
  std::lock_guard<std::mutex> lk(liveMutex_);
  live_.erase(inst % kMaxLiveInstances);
}

bool Context::agreeOnSharing() {
  if (sharing_ < 0)
    sharing_ = ipc::agreeOnSharing(rank, size, device_, [this](const std::string& tag, const std::vector<char>& mine) {
      return allgather("sharing/" + tag, mine);
    }) ? 1 : 0;
  return sharing_ == 1;
}

void Context::barrier(const std::string& tag) { (void)allgather("barrier/" + tag, {}); }

std::vector<std::vector<char>> Context::allgather(const std::string& tag, const std::vector<char>& mine) {
  const uint64_t gen = barrierGen_++;
  return store_->allgather(strcat_("gloo_amd/ag/", gen, "/", tag), rank, size, mine, timeout_);
}

}  // namespace gloo_amd
