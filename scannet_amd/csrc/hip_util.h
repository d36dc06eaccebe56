// hip_util.h -- small RAII helpers shared by the mesh filters that run on the GPU (simplify_gpu.hip, clean_gpu.hip) and by the work sets of the tracker
// and the aligner (track.hip, align.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace sf {

template <bool HOST>
struct Buf {   // one hipMalloc'ed (DevBuf) or page-locked hipHostMalloc'ed (HostBuf) buffer, freed with its scope
  void* p = nullptr;
  size_t cap = 0;   // the bytes asked for; 0 while p is null
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  void release() {
    if (p) (void)(HOST ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  hipError_t alloc(size_t bytes) {   // null on failure
    release();
    const size_t n = bytes ? bytes : 16;
    const hipError_t e = HOST ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
    if (e != hipSuccess) p = nullptr;
    else cap = bytes;
    return e;
  }
  hipError_t reserve(size_t bytes) { return bytes <= cap ? hipSuccess : alloc(bytes); }   // grow only
  template <typename T> T* as() const { return (T*)p; }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;

struct StreamGuard {   // a stream of the call's own: host threads finishing several meshes, and the fuser of the next scan, share the device
  hipStream_t s = nullptr;
  StreamGuard() = default;
  StreamGuard(const StreamGuard&) = delete;
  StreamGuard& operator=(const StreamGuard&) = delete;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};

}  // namespace sf
