// device_owned.h — the owners of a context's HIP resources (host only).
//
// Every device buffer, event, stream and pinned host block of rt_api.hip is a member of one of these types and is released
// when its owner goes: destroying a context is `delete`, and a new family of calls adds members and nothing else.  Members go
// in reverse order of declaration, so the streams, declared first, outlive every buffer and event.
//
// No HIP header is included here: include this one after <hip/hip_runtime.h>, or after stand-ins for the few names it uses
// (tests/model/owned_check.cpp).
#pragma once

#include <cstddef>
#include <memory>
#include <utility>

namespace owned {

// A handle released by `Release`.  Movable, not copyable (the move operations suppress the copies).  Converts to the handle
// for the calls that use it; `&owner` is the address of the handle, for the call that creates it into an empty owner:
// hipEventCreate(&ev), hipHostMalloc(&block, ...).
template <class T, hipError_t (*Release)(T)>
struct Handle {
  T h = nullptr;

  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != std::addressof(o)) {
      (void)reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Handle() { (void)reset(); }

  // release and clear; nothing to do on an empty owner
  hipError_t reset() {
    const hipError_t e = h ? Release(h) : hipSuccess;
    h = nullptr;
    return e;
  }
  operator T() const { return h; }
  T* operator&() { return &h; }
};

using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Pinned = Handle<void*, hipHostFree>;   // hipHostMalloc

struct EventPair {
  Event a, b;
};

// Device memory with the sizes rt_api.hip keeps beside it (ensure_buffer, upload).  Movable, not copyable.
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t capacity = 0;  // bytes allocated
  size_t size = 0;      // bytes in use

  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept { *this = std::move(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      ptr = std::exchange(o.ptr, nullptr);
      capacity = std::exchange(o.capacity, 0);
      size = std::exchange(o.size, 0);
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  // free and clear; nothing to do on an empty buffer
  void reset() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    capacity = size = 0;
  }
};

}  // namespace owned
