// snf_devmem.h - host side of the extraction and container handles (snf_extract.hip, snf_container.h): device memory that is
// released with its owner, and the C boundary every `extern "C"` entry point of the two goes through.
#pragma once
#include "snf_rt.h"
#include <exception>

#pragma GCC visibility push(hidden)      // helpers, not part of what the library exports
namespace snf {

// One grow-only device allocation carved into arrays.  (A run made some forty hipMalloc / hipFree calls - 0.5 ms of a 1.4-ms run;
// repeated runs over tables of similar size now allocate nothing.)
struct XSlab {
  uint8_t* base = nullptr; size_t cap = 0, used = 0; bool measuring = false;
  void measure() { measuring = true; used = 0; }
  void reserve() {      // after a measuring pass: room for what it added up
    const size_t need = used + 256;
    if (need > cap) {
      if (base) (void)hipFree(base);
      base = nullptr; cap = 0;
      const size_t want = need + need / 4;
      void* p = nullptr;
      if (hipMalloc(&p, want) != hipSuccess) snf::fail("hipMalloc failed (" + std::to_string(want) + " bytes)");
      base = (uint8_t*)p; cap = want;
    }
    measuring = false; used = 0;
  }
  template <class T> T* take(size_t n, size_t pad_bytes = 0) {
    used = (used + 255) & ~(size_t)255;
    T* p = measuring ? nullptr : (T*)(base + used);
    used += (n ? n : 1) * sizeof(T) + pad_bytes;
    return p;
  }
  void release() { if (base) (void)hipFree(base); base = nullptr; cap = 0; used = 0; }
};

inline void x_free(void* p) {
  (void)hipFree(p);
}
template <class T> T* x_alloc(std::vector<void*>& pool, size_t n, size_t pad_bytes = 0) {
  void* p = nullptr;
  const size_t bytes = (n ? n : 1) * sizeof(T) + pad_bytes;
  if (hipMalloc(&p, bytes) != hipSuccess) snf::fail("hipMalloc failed (" + std::to_string(bytes) + " bytes)");
  pool.push_back(p);
  return (T*)p;
}
inline void x_h2d(void* d, const void* h, size_t bytes) {
  if (!bytes) return;
  SNF_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
}
inline void x_d2h(void* h, const void* d, size_t bytes) {
  if (!bytes) return;
  SNF_HIP(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
}
template <class T> T* x_up(std::vector<void*>& pool, const T* h, size_t n, size_t pad_bytes = 0) {
  T* d = x_alloc<T>(pool, n, pad_bytes);
  x_h2d(d, h, n * sizeof(T));
  return d;
}
inline void x_release(std::vector<void*>& pool) { for (void* p : pool) x_free(p); pool.clear(); }

// ---- the C boundary ---------------------------------------------------------------------------------------------
// An entry point of a handle: select the handle's device, run `body`, leave what it throws in `err` (the thread-local string behind
// the family's snf_*_last_error).  0, or 1 with the message.  What an entry checks before it touches the device stands in front.
template <class F> int c_entry(std::string& err, int device, F&& body) {
  if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return 1; }
  try { body(); }
  catch (const snf::Error& e) { err = e.msg; return 1; }
  catch (const std::exception& e) { err = e.what(); return 1; }
  return 0;
}
// What every snf_*_create does before it makes its handle; `noun` names the family's kernels in the message.
inline int c_create(std::string& err, int device, const char* noun) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { err = std::string("no HIP device: the ") + noun + " kernels need a gfx950 GPU (there is no CPU fallback)"; return 1; }
  if (device < 0 || device >= nd) { err = "device index out of range"; return 1; }
  if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return 1; }
  return 0;
}
}  // namespace snf
#pragma GCC visibility pop
