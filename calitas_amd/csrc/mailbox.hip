// mailbox.hip -- the mailbox of mailbox.hpp: the one-thread kernel that posts and the host side that opens, posts and waits.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "mailbox.hpp"

namespace calitas {

__global__ void mailbox_kernel(const uint32_t* src, int n, uint32_t* box, uint32_t seq) {
  CALITAS_TAIL_PRIO();
  for (int i = 0; i < n; i++) box[1 + i] = src[i];
  __threadfence_system();
  __hip_atomic_store(box, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t mailbox_open(Mailbox& mb) {
  if (mb.host) return hipSuccess;
  void* h = nullptr;
  hipError_t e = hipHostMalloc(&h, (MAILBOX_WORDS + 1) * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return e;
  void* d = nullptr;
  e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) { (void)hipHostFree(h); return e; }
  mb.host = (volatile uint32_t*)h; mb.dev = (uint32_t*)d; mb.seq = 0;
  mb.host[0] = 0;
  return hipSuccess;
}

void mailbox_close(Mailbox& mb) {
  if (mb.host) (void)hipHostFree((void*)mb.host);
  mb.host = nullptr; mb.dev = nullptr;
}

hipError_t mailbox_post(Mailbox& mb, const uint32_t* src, int n, hipStream_t stream) {
  hipError_t e = mailbox_open(mb);
  if (e != hipSuccess) return e;
  if (n > MAILBOX_WORDS) return hipErrorInvalidValue;
  mb.seq++;
  hipLaunchKernelGGL(mailbox_kernel, dim3(1), dim3(1), 0, stream, src, n, mb.dev, mb.seq);
  return hipGetLastError();
}

hipError_t mailbox_wait(Mailbox& mb, hipStream_t stream) {
  // Bounded: a kernel that never finishes would otherwise leave the caller (and every lane thread) spinning for good.  The limit is far
  // beyond any legitimate wait (the longest device stage of a PAM-less whole-genome pass is under a second).
  constexpr double kDeadlineSeconds = 120.0;
  Backoff wait;
  long long next_check_us = 200;               // now and then: is the stream still alive?
  while (mb.host[0] != mb.seq) {
    wait.pause();
    if (wait.spins >= 256 && wait.waited_us() >= next_check_us) {
      next_check_us = wait.waited_us() + 200;
      const hipError_t e = hipStreamQuery(stream);
      if (e != hipSuccess && e != hipErrorNotReady) return e;
      if (e == hipSuccess && mb.host[0] != mb.seq) {      // everything queued has run, yet nothing arrived
        if (mb.host[0] == mb.seq) break;
        return hipErrorUnknown;
      }
      if ((double)wait.waited_us() * 1e-6 > kDeadlineSeconds) return hipErrorLaunchTimeOut;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return hipSuccess;
}

}  // namespace calitas
