// hd_pipelined_test.cc — a Gloo program that runs the pipelined
// halving-doubling through Gloo's own surface (gloo_amd/include/gloo_amd/gloo_bridge.h):
// gloo::HipAllreduceHalvingDoublingPipelined and
// gloo::HipAllreduceHalvingDoubling(..., pipelineBroadcastAndReduce) built from
// a gloo::Context of the reference (ranks as threads over its TCP transport),
// checked against the closed form of gloo/test/base_test.h:184-236.  Each
// case also checks WHICH algorithm the bridge constructor selected
// (HipPlanAlgorithm::algorithm()): the flag and the Pipelined twin select
// GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED, false and the default the plain
// one.  Built by oracle/hd_pipelined.mk into oracle/_ref/hd_pipelined_test;
// run by tests/test_hd_pipelined_bridge.py.  Prints "ok <case>" or
// "FAIL <case>: why" per case; exit status 0 when all pass.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "gloo/rendezvous/context.h"
#include "gloo/rendezvous/hash_store.h"
#include "gloo/transport/tcp/device.h"
#include "gloo_amd/gloo_bridge.h"

namespace {

#define HIPOK(x)                                                                                      \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

using Make = std::function<std::unique_ptr<gloo::HipPlanAlgorithm<float, GLOO_HIP_ALGO_HALVING_DOUBLING,
                                                                  gloo::HipDeviceWorkspace<float>>>(
    std::shared_ptr<gloo::Context>&, std::vector<float*>&, int)>;

// Fixture<T>::assignValues / checkAllreduceResult: element j of pointer i on
// rank r holds j * P * k + r * k + i, so every output element j is
// j * (P k)^2 + (P k)(P k - 1) / 2.  Runs twice with the inputs reloaded.
std::string run(int P, int k, int count, int wantAlgo, const Make& make) {
  auto store = std::make_shared<gloo::rendezvous::HashStore>();
  std::vector<std::thread> ts;
  std::mutex em;
  std::string err;
  for (int rank = 0; rank < P; rank++) {
    ts.emplace_back([&, rank] {
      try {
        HIPOK(hipSetDevice(0));
        auto rctx = std::make_shared<gloo::rendezvous::Context>(rank, P);
        rctx->setTimeout(std::chrono::milliseconds(30000));
        gloo::transport::tcp::attr attr("localhost");
        auto dev = gloo::transport::tcp::CreateDevice(attr);
        rctx->connectFullMesh(store, dev);
        std::shared_ptr<gloo::Context> ctx = rctx;
        const size_t stride = (size_t)P * k;
        std::vector<float*> ptrs(k);
        std::vector<float> host(count);
        for (int i = 0; i < k; i++) HIPOK(hipMalloc(reinterpret_cast<void**>(&ptrs[i]), count * sizeof(float)));
        {
          auto a = make(ctx, ptrs, count);
          if (a->algorithm() != wantAlgo)
            throw std::runtime_error("the bridge selected algorithm " + std::to_string(a->algorithm()) + ", not " +
                                     std::to_string(wantAlgo));
          for (int r = 0; r < 2; r++) {
            for (int i = 0; i < k; i++) {
              for (int j = 0; j < count; j++) host[j] = (float)(j * stride + (size_t)rank * k + i);
              HIPOK(hipMemcpy(ptrs[i], host.data(), count * sizeof(float), hipMemcpyHostToDevice));
            }
            a->run();
            for (int i = 0; i < k; i++) {
              HIPOK(hipMemcpy(host.data(), ptrs[i], count * sizeof(float), hipMemcpyDeviceToHost));
              for (int j = 0; j < count; j++) {
                const float want = (float)((double)j * stride * stride + stride * (stride - 1) / 2.0);
                if (host[j] != want)
                  throw std::runtime_error("mismatch in ptr " + std::to_string(i) + " element " + std::to_string(j) +
                                           " run " + std::to_string(r) + ": " + std::to_string(host[j]) +
                                           " != " + std::to_string(want));
              }
            }
          }
        }
        for (float* p : ptrs) HIPOK(hipFree(p));
      } catch (const std::exception& e) {
        std::lock_guard<std::mutex> lk(em);
        if (err.empty()) err = "rank " + std::to_string(rank) + ": " + e.what();
      }
    });
  }
  for (auto& t : ts) t.join();
  return err;
}

}  // namespace

int main() {
  using HD = gloo::HipAllreduceHalvingDoubling<float>;
  using HDP = gloo::HipAllreduceHalvingDoublingPipelined<float>;
  using Base = gloo::HipPlanAlgorithm<float, GLOO_HIP_ALGO_HALVING_DOUBLING, gloo::HipDeviceWorkspace<float>>;
  struct Case {
    const char* name;
    int P, k, n, algo;
    Make make;
  };
  auto flag = [](bool on) {
    return [on](std::shared_ptr<gloo::Context>& c, std::vector<float*>& p, int n) {
      return std::unique_ptr<Base>(new HD(c, p, n, std::vector<hipStream_t>(), on));
    };
  };
  const Make twin = [](std::shared_ptr<gloo::Context>& c, std::vector<float*>& p, int n) {
    return std::unique_ptr<Base>(new HDP(c, p, n));
  };
  const Make plain = [](std::shared_ptr<gloo::Context>& c, std::vector<float*>& p, int n) {
    return std::unique_ptr<Base>(new HD(c, p, n));
  };
  const std::vector<Case> cases = {
      {"HalvingDoublingPipelined/P2/k2/n1000", 2, 2, 1000, GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED, twin},
      {"HalvingDoubling(flag=true)/P2/k2/n1000", 2, 2, 1000, GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED, flag(true)},
      {"HalvingDoubling(flag=false)/P2/k2/n1000", 2, 2, 1000, GLOO_HIP_ALGO_HALVING_DOUBLING, flag(false)},
      {"HalvingDoubling(default)/P2/k2/n1000", 2, 2, 1000, GLOO_HIP_ALGO_HALVING_DOUBLING, plain},
      {"HalvingDoublingPipelined/P3/k3/n1001", 3, 3, 1001, GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED, twin},
  };
  int bad = 0;
  for (const Case& c : cases) {
    const std::string err = run(c.P, c.k, c.n, c.algo, c.make);
    if (err.empty()) {
      std::printf("ok   %s\n", c.name);
    } else {
      std::printf("FAIL %s: %s\n", c.name, err.c_str());
      bad++;
    }
    std::fflush(stdout);
  }
  return bad ? 1 : 0;
}
