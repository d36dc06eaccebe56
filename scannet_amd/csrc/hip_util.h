// hip_util.h -- the host-side device plumbing of every .hip translation unit: scope-owned device and pinned buffers, streams and event pairs, opening a
// device by index, telling device memory from host memory, and the device scope of the _device entry points.  Nothing here runs on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "common.h"

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

struct EventSpan {   // two events on a stream; us() after the stream has been synchronised
  hipEvent_t a = nullptr, b = nullptr;
  EventSpan() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
  EventSpan(const EventSpan&) = delete;
  EventSpan& operator=(const EventSpan&) = delete;
  ~EventSpan() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  void begin(hipStream_t s) { if (a) (void)hipEventRecord(a, s); }
  void end(hipStream_t s) { if (b) (void)hipEventRecord(b, s); }
  float us() const {
    float ms = 0.0f;
    if (!a || !b || hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0.0f; }
    return ms * 1000.0f;
  }
};

// Makes `device` the calling thread's current device.  Without a runtime or without any device: SF_ERR_DEVICE and "no HIP device: " followed by the site's
// own sentence (who needs the device, what the alternative is), with the runtime's sticky error cleared.  An index outside [0, count): `range_code`, the
// code the site answers for it (SF_ERR_INVALID_ARG where the index is an argument like any other, SF_ERR_DEVICE where the device is one of two paths).
__attribute__((format(printf, 3, 4))) inline int open_device(int device, int range_code, const char* sentence, ...) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    char buf[512];
    va_list ap;
    va_start(ap, sentence);
    vsnprintf(buf, sizeof(buf), sentence, ap);
    va_end(ap);
    return fail(SF_ERR_DEVICE, "no HIP device: %s", buf);
  }
  if (device < 0 || device >= ndev) return fail(range_code, "device %d out of range (%d devices)", device, ndev);
  SF_HIP_CHECK(hipSetDevice(device));
  return SF_OK;
}

// is p device memory (and of which device)?  hipPointerGetAttributes is a query on the host that waits for nothing on the device
inline bool on_device(const void* p, int* device = nullptr) {
  if (!p) return false;
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (device) *device = a.device;
  return a.type == hipMemoryTypeDevice;
}

// a result leaves device memory: dst may be host or device memory
inline hipError_t deliver(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return hipSuccess;
  return hipMemcpyAsync(dst, src, bytes, on_device(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s);
}

// the device of a _device call is current for the launch only: the caller's current device is put back when the call returns
struct DeviceScope {
  int old = -1;
  bool changed = false;
  DeviceScope() = default;
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  ~DeviceScope() { if (changed) (void)hipSetDevice(old); }
  hipError_t enter(int dev) {
    hipError_t e = hipGetDevice(&old);
    if (e != hipSuccess || old == dev) return e;
    e = hipSetDevice(dev);
    changed = e == hipSuccess;
    return e;
  }
};

// every pointer of a _device call must be device memory, all on one device: that device is made current for the life of `scope`
inline int same_device(const void* const* ptrs, int count, const char* who, DeviceScope& scope) {
  int dev = -1;
  for (int i = 0; i < count; i++) {
    if (!ptrs[i]) continue;
    int d = -1;
    if (!on_device(ptrs[i], &d)) return fail(SF_ERR_INVALID_ARG, "%s: argument %d is not device memory", who, i);
    if (dev >= 0 && d != dev) return fail(SF_ERR_INVALID_ARG, "%s: arguments on devices %d and %d", who, dev, d);
    dev = d;
  }
  if (dev >= 0) SF_HIP_CHECK(scope.enter(dev));
  return SF_OK;
}

}  // namespace sf
