// Shared host-side plumbing of libmimi_hip: error reporting and the guard of the C entries, the stream-owning base of
// the handles, device buffers, pointer classification.  No kernels here.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mimi_hip.h"

namespace mimi_hip {

// utils/print.hpp:47-56 PrintAndThrowError -> std::runtime_error; the C ABI catches it,
// stores the text for mimi_hip_last_error() and returns non-zero.
struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

[[noreturn]] inline void fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw Error(buf);
}

#define MH_HIP(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      ::mimi_hip::fail("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__, __LINE__, \
                       hipGetErrorString(e_));                                             \
  } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device) instead of once per launch (it costs microseconds,
// which the small meshes of the reference's examples notice)
inline void ensure_dynamic_lds(const void* kernel, int bytes) {
  static std::mutex guard;
  static std::map<std::pair<const void*, int>, int> granted;
  int device = 0;
  MH_HIP(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(guard);
  int& have = granted[std::make_pair(kernel, device)];
  if (bytes > have) {
    MH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
  }
}

// Every kernel launch of the converted sources: above the 64 KB every kernel may use unasked, the dynamic-LDS limit is raised
// first (the nine-block and symmetric-half kernels ask for 69-76 KB, so this is the rule their launchers applied
// unconditionally); kernels under the limit get no attribute call.
template<typename... Params, typename... Args>
void launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  if (lds_bytes > 64 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds_bytes);
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
  MH_HIP(hipGetLastError());
}

// The environment switches of the library: the only getenv of csrc, one accessor per switch.
// WHEN a switch is read is part of its behaviour -- the tests flip the per-create and per-launch ones inside one process.
inline const char* env_text(const char* name) { return getenv(name); }
inline bool env_starts(const char* name, char c) {
  const char* v = env_text(name);
  return v && v[0] == c;
}
// once per process, at first use
inline bool env_general_no_wpe() { static const bool on = env_starts("MIMI_HIP_GENERAL_NO_WPE", '1'); return on; }
inline bool env_general_no_mfma() { static const bool on = env_starts("MIMI_HIP_GENERAL_NO_MFMA", '1'); return on; }
// at every create
inline bool env_force_general() { return env_starts("MIMI_HIP_FORCE_GENERAL", '1'); }
inline bool env_keep_general() { return env_starts("MIMI_HIP_KEEP_GENERAL", '1'); }
inline bool env_no_structured() { return env_starts("MIMI_HIP_NO_STRUCTURED", '1'); }
// what the handle's general_two_phase_failed starts from (domain_dispatch.hpp: the atomics instead of store + row gather)
inline bool env_general_no_two_phase() { return env_starts("MIMI_HIP_GENERAL_NO_TWO_PHASE", '1'); }
// a test seam: what stands in for WGSYM_MIN_WGS on the handle (wgsym_geometry.hpp); 0 when unset
inline int env_wgsym_min_wgs() {
  const char* v = env_text("MIMI_HIP_WGSYM_MIN_WGS");
  if (!v) return 0;
  char* end = nullptr;
  const long n = strtol(v, &end, 10);
  if (end == v || *end != '\0' || n < 1 || n > INT32_MAX) fail("MIMI_HIP_WGSYM_MIN_WGS must be a positive integer, got \"%s\"", v);
  return (int)n;
}
// at every launch of the degree-3 contraction
inline bool env_p3_contract_cxx() {
  const char* v = env_text("MIMI_HIP_P3_CONTRACT");
  return v && !strcmp(v, "cxx");
}

void set_last_error(const std::string& s);

// Every entry of the C ABI runs its body through this: an exception becomes the text of mimi_hip_last_error() and a
// non-zero return.
template<typename F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return 1;
  } catch (...) {
    set_last_error("unknown error");
    return 1;
  }
}

// the stream argument of the C ABI: MIMI_HIP_STREAM_NULL = the device's null stream, NULL = `fallback`
inline hipStream_t pick_stream(void* stream, hipStream_t fallback) {
  return stream == MIMI_HIP_STREAM_NULL ? nullptr : (stream ? reinterpret_cast<hipStream_t>(stream) : fallback);
}

// What every handle of the library starts with: its device, a non-blocking stream of its own and the stream it launches
// on.  The handle structs derive from it; handle_set_stream / _synchronize / _destroy below are their C entries.
struct StreamHandle {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  StreamHandle() = default;
  StreamHandle(const StreamHandle&) = delete;
  StreamHandle& operator=(const StreamHandle&) = delete;
  ~StreamHandle() {
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
  void open(int dev) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
      fail("libmimi_hip: no HIP device visible -- this library has no CPU fallback");
    if (dev < 0 || dev >= count) fail("device %d out of range (%d visible)", dev, count);
    device = dev;
    MH_HIP(hipSetDevice(dev));
    MH_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    stream = own_stream;
  }
  void set_stream(void* s) { stream = pick_stream(s, own_stream); }
  void synchronize() {
    MH_HIP(hipSetDevice(device));
    MH_HIP(hipStreamSynchronize(stream));
  }
};

template<typename H>
int handle_set_stream(H* h, void* stream) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->set_stream(stream);
  });
}

template<typename H>
int handle_synchronize(H* h) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->synchronize();
  });
}

template<typename H>
int handle_destroy(H* h) {
  return guarded([&] {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
  });
}

// true when p points to device memory of any kind
inline bool is_device_pointer(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // plain malloc'd host memory: not an error for us
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// a host copy of n elements of a host or device source
template<typename T>
std::vector<T> to_host(const T* p, size_t n) {
  std::vector<T> out(n);
  if (n == 0) return out;
  if (is_device_pointer(p)) MH_HIP(hipMemcpy(out.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
  else std::copy(p, p + n, out.begin());
  return out;
}

template<typename T>
struct DeviceBuffer {
  T* ptr = nullptr;
  size_t count = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  void resize(size_t n) {
    if (n <= count) return;
    release();
    MH_HIP(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
    count = n;
  }
  // copy n elements from a host or device source
  void assign(const T* src, size_t n, hipStream_t s) {
    resize(n);
    if (n == 0) return;
    MH_HIP(hipMemcpyAsync(ptr, src, n * sizeof(T),
                          is_device_pointer(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (!is_device_pointer(src)) MH_HIP(hipStreamSynchronize(s));
  }
};

// A caller-provided array that may live on the host (then mirrored in `stage`) or on the
// device (used in place).
template<typename T>
struct Mirror {
  T* dev = nullptr;      // what kernels use
  T* host = nullptr;     // non-null when the caller's buffer is on the host
  size_t count = 0;
  DeviceBuffer<T>* stage = nullptr;

  static Mirror in(const T* p, size_t n, DeviceBuffer<T>& stage, hipStream_t s) {
    Mirror m;
    m.count = n;
    if (is_device_pointer(p)) {
      m.dev = const_cast<T*>(p);
    } else {
      stage.resize(n);
      MH_HIP(hipMemcpyAsync(stage.ptr, p, n * sizeof(T), hipMemcpyHostToDevice, s));
      m.dev = stage.ptr;
      m.host = const_cast<T*>(p);
      m.stage = &stage;
    }
    return m;
  }
  // for += outputs: host contents are uploaded first, downloaded by finish()
  static Mirror inout(T* p, size_t n, DeviceBuffer<T>& stage, hipStream_t s) { return in(p, n, stage, s); }
  void finish(hipStream_t s) {
    if (host) MH_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s));
  }
};

struct MaterialDev {
  mimi_hip_material m;
  double const_temperature_contribution;  // material_hardening.hpp:310-318
  double sigma_y_ref;                     // HardeningBase::SigmaY()
};

// What the kernels read next to the C struct, with the reference's checks; needs no HIP runtime, so the host build of the
// device routines (tests/host_materials.hip) calls the same function as the library.
inline MaterialDev make_material_dev(const mimi_hip_material& m) {
  MaterialDev d{};
  d.m = m;
  d.const_temperature_contribution = 1.0;
  if (m.kind == MIMI_HIP_MAT_J2 || m.kind == MIMI_HIP_MAT_J2SIMO || m.kind == MIMI_HIP_MAT_J2LOG) {
    if (m.hardening < MIMI_HIP_HARD_POWERLAW || m.hardening > MIMI_HIP_HARD_JC_CONST_TEMP)
      fail("hardening missing for J2 / J2Simo / J2Log");  // materials.cpp:139-148,177-183,217-223
    d.sigma_y_ref = (m.hardening == MIMI_HIP_HARD_POWERLAW || m.hardening == MIMI_HIP_HARD_VOCE) ? m.sigma_y : m.A;
    if (m.hardening >= MIMI_HIP_HARD_JC_TEMP_RATE && m.reference_temperature > m.melting_temperature)
      fail("reference temperature, %g ,can't be bigger than melting temperature, %g .",
           m.reference_temperature, m.melting_temperature);  // material_hardening.hpp:228-238
    if (m.hardening == MIMI_HIP_HARD_JC_CONST_TEMP) {
      d.const_temperature_contribution =
          1.0 - std::pow((m.initial_temperature - m.reference_temperature)
                             / (m.melting_temperature - m.reference_temperature), m.m);
      if (d.const_temperature_contribution <= 0.0)
        fail("Invalid temperature contribution %g", d.const_temperature_contribution);
    }
  } else if (m.kind == MIMI_HIP_MAT_J2LINEAR) {
    d.sigma_y_ref = m.sigma_y;
  } else if (m.kind != MIMI_HIP_MAT_NEOHOOKEAN && m.kind != MIMI_HIP_MAT_STVK) {
    fail("unknown material kind %d", m.kind);
  }
  return d;
}

}  // namespace mimi_hip
