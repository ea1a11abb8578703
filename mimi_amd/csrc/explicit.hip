// C ABI + kernels of the explicit central-difference step with a lumped mass: stands in for the reference's
// CentralDifference = Newmark(beta = 0, gamma = 1/2) (solvers/ode.hpp:257, ode.cpp:229-250), which solves with the consistent
// mass in every step; here the mass is a vector and a step is two streaming kernels around one residual assembly.
//
// Per dof, with the masks F (fixed: v = 0, x kept) and P (constant velocity: v = vbar, a = 0; P wins where both are set):
//   predict   v <- v + dt/2 a;  x <- x + dt v                                  (v is now v_{n+1/2})
//   correct   a <- ((f - r) - d) / m on free dofs, 0 elsewhere;  v <- v + dt/2 a
// r is the RAW internal force of all integrators at the new x (not eliminated: the ledger needs the reactions at P dofs),
// d = eta C v_{n+1/2} the damping force at the predictor velocity, f the load vector.  The reference's predictor for the
// damping is the same v + (1 - gamma) dt a; its gamma dt a correction would need a solve and is left out.
//
// The energy ledger is accumulated in the pass of `correct`, by the trapezoid rule with dx = dt v_{n+1/2}:
//   W_int  += 1/2 (r_n + r_{n+1}) . dx   over all dofs      W_damp += 1/2 (d_n + d_{n+1}) . dx   over free dofs
//   W_ext  += f . dx over free dofs + 1/2 (r_n + r_{n+1}) . dx over P dofs (the work of the reactions)
//   KE = 1/2 sum m v^2,  Q = dt^2/8 sum m a^2,  E* = KE - Q + W_int + W_damp - W_ext   -- E* is conserved by the scheme
// in exact arithmetic for any r (plastic, contact), with the lagged damping and with prescribed dofs, while f stays put.
//
// The sums give equal bytes from equal inputs: the grid depends on n alone, every thread adds its dofs in ascending order,
// the workgroup adds by a fixed tree, and the workgroup that finishes last adds the per-workgroup partials in index order
// (EXPLICIT_FINAL_RUN consecutive ones per thread, then the same tree).  No atomic takes part in a sum: the one atomic is
// the ticket that tells a workgroup it is the last.  Contraction to fused multiply-adds is off in the kernels, so an
// update is the two roundings a host loop makes.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "common.hpp"

namespace mimi_hip {

constexpr int EXPLICIT_BLOCK = 256;        // threads of a workgroup: a tree of 8 levels
constexpr int EXPLICIT_GRID_CAP = 1024;    // workgroups at most: beyond EXPLICIT_BLOCK * EXPLICIT_GRID_CAP dofs a thread takes several
constexpr int EXPLICIT_FINAL_RUN = EXPLICIT_GRID_CAP / EXPLICIT_BLOCK;   // partials a thread of the last workgroup adds
constexpr int EXPLICIT_TREE_DEPTH = 16;    // levels of the two trees a term passes through
constexpr int EXPLICIT_N_SUMS = 6;
constexpr unsigned char kFixed = 1, kPrescribed = 2;

enum { SUM_MV2 = 0, SUM_INT = 1, SUM_DAMP = 2, SUM_LOAD = 3, SUM_REACT = 4, SUM_MA2 = 5 };
// the running values (device): sum m v^2, W_int, W_ext, W_damp, sum m a^2; behind them what the additions into the three
// works have lost so far (compensated summation: over many steps a work keeps the accuracy of its increments)
enum { RUN_MV2 = 0, RUN_WINT = 1, RUN_WEXT = 2, RUN_WDAMP = 3, RUN_MA2 = 4, N_RUN = 5, RUN_LOST = 5, N_RUN_ALL = 9 };

inline unsigned explicit_grid(int64_t n) {
  return (unsigned)std::min<int64_t>((n + EXPLICIT_BLOCK - 1) / EXPLICIT_BLOCK, EXPLICIT_GRID_CAP);
}

__global__ __launch_bounds__(EXPLICIT_BLOCK) void explicit_mask_kernel(int64_t n, const unsigned char* __restrict__ fixed,
                                                                       const unsigned char* __restrict__ prescribed,
                                                                       unsigned char* __restrict__ mask) {
  for (int64_t i = (int64_t)blockIdx.x * EXPLICIT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXPLICIT_BLOCK)
    mask[i] = (unsigned char)(((fixed && fixed[i]) ? kFixed : 0) | ((prescribed && prescribed[i]) ? kPrescribed : 0));
}

// a non-positive (or NaN) mass on a dof that moves -- free, or prescribed (its mass enters KE): a plain store, every such
// thread stores the same value
__global__ __launch_bounds__(EXPLICIT_BLOCK) void explicit_mass_check_kernel(int64_t n, const unsigned char* __restrict__ mask,
                                                                             const double* __restrict__ m, int* status) {
  for (int64_t i = (int64_t)blockIdx.x * EXPLICIT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXPLICIT_BLOCK) {
    const unsigned char k = mask[i];
    if ((!k || (k & kPrescribed)) && !(m[i] > 0.0)) *status = 1;
  }
}

__global__ __launch_bounds__(EXPLICIT_BLOCK) void explicit_predict_kernel(int64_t n, double dt, const unsigned char* __restrict__ mask,
                                                                          const double* __restrict__ vbar, const double* __restrict__ a,
                                                                          double* __restrict__ x, double* __restrict__ v) {
#pragma clang fp contract(off)
  const double hdt = 0.5 * dt;
  for (int64_t i = (int64_t)blockIdx.x * EXPLICIT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXPLICIT_BLOCK) {
    const unsigned char k = mask[i];
    if (k & kPrescribed) {
      const double vb = vbar[i];
      v[i] = vb;
      x[i] = x[i] + dt * vb;
    } else if (k & kFixed) {
      v[i] = 0.0;
    } else {
      const double vh = v[i] + hdt * a[i];
      v[i] = vh;
      x[i] = x[i] + dt * vh;
    }
  }
}

struct ExplicitArgs {
  int64_t n;
  double dt;
  const unsigned char* mask;
  const double* vbar;
  const double* m;
  const double* f;        // may be nullptr: no load
  const double* r;
  const double* r_prev;   // START: unused
  const double* d;        // may be nullptr: no damping (then d_prev is nullptr too)
  const double* d_prev;
  double* a;
  double* v;
  double* partials;       // [EXPLICIT_N_SUMS][EXPLICIT_GRID_CAP]
  double* run;            // [N_RUN_ALL]
  unsigned* ticket;
};

// work += inc, with the rounding error of the addition carried in `lost` (Kahan)
__device__ inline void explicit_accumulate(double* work, double* lost, double inc) {
#pragma clang fp contract(off)
  const double y = inc - *lost, t = *work + y;
  *lost = (t - *work) - y;
  *work = t;
}

// the fixed tree over the workgroup's EXPLICIT_BLOCK threads, all sums at once; the result in part[0][*]
__device__ inline void explicit_tree(double (*part)[EXPLICIT_N_SUMS], const double* acc) {
  const int t = threadIdx.x;
  for (int k = 0; k < EXPLICIT_N_SUMS; ++k) part[t][k] = acc[k];
  __syncthreads();
  for (int w = EXPLICIT_BLOCK / 2; w >= 1; w >>= 1) {
    if (t < w)
      for (int k = 0; k < EXPLICIT_N_SUMS; ++k) part[t][k] += part[t + w][k];
    __syncthreads();
  }
}

// START: a_0 from the forces at the initial state, the masks applied to v, the works zeroed; else the corrector with the
// ledger.  A dof's values stay in registers between the update and the sums.
template<int START>
__global__ __launch_bounds__(EXPLICIT_BLOCK) void explicit_correct_kernel(ExplicitArgs g) {
#pragma clang fp contract(off)
  __shared__ double part[EXPLICIT_BLOCK][EXPLICIT_N_SUMS];
  __shared__ bool last;
  const double hdt = 0.5 * g.dt;
  double acc[EXPLICIT_N_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * EXPLICIT_BLOCK + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * EXPLICIT_BLOCK) {
    const unsigned char k = g.mask[i];
    const double mi = g.m[i];
    if (k & kPrescribed) {
      const double vb = g.vbar[i];
      g.a[i] = 0.0;
      g.v[i] = vb;
      acc[SUM_MV2] += (mi * vb) * vb;
      if constexpr (!START) {
        const double t = (g.r_prev[i] + g.r[i]) * vb;
        acc[SUM_INT] += t;
        acc[SUM_REACT] += t;
      }
    } else if (k & kFixed) {
      g.a[i] = 0.0;
      g.v[i] = 0.0;
    } else {
      const double fi = g.f ? g.f[i] : 0.0;
      const double r1 = g.r[i];
      const double d1 = g.d ? g.d[i] : 0.0;
      const double an = ((fi - r1) - d1) / mi;
      const double vh = g.v[i];
      g.a[i] = an;
      double vn = vh;
      if constexpr (!START) {
        vn = vh + hdt * an;
        g.v[i] = vn;
        acc[SUM_INT] += (g.r_prev[i] + r1) * vh;
        if (g.d) acc[SUM_DAMP] += (g.d_prev[i] + d1) * vh;
        acc[SUM_LOAD] += fi * vh;
      }
      acc[SUM_MV2] += (mi * vn) * vn;
      acc[SUM_MA2] += (mi * an) * an;
    }
  }
  explicit_tree(part, acc);
  if (threadIdx.x < EXPLICIT_N_SUMS) g.partials[threadIdx.x * EXPLICIT_GRID_CAP + blockIdx.x] = part[0][threadIdx.x];
  // the workgroup that takes the last ticket adds the partials; the fences order the partials before the ticket and the
  // reads behind it
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(g.ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  const volatile double* p = g.partials;
  for (int k = 0; k < EXPLICIT_N_SUMS; ++k) {
    double s = 0.0;
    for (int j = 0; j < EXPLICIT_FINAL_RUN; ++j) {
      const int b = threadIdx.x * EXPLICIT_FINAL_RUN + j;
      if (b < (int)gridDim.x) s += p[k * EXPLICIT_GRID_CAP + b];
    }
    acc[k] = s;
  }
  explicit_tree(part, acc);
  if (threadIdx.x == 0) {
    g.run[RUN_MV2] = part[0][SUM_MV2];
    g.run[RUN_MA2] = part[0][SUM_MA2];
    if constexpr (START) {
      for (int k = RUN_WINT; k <= RUN_WDAMP; ++k) g.run[k] = g.run[RUN_LOST + k] = 0.0;
    } else {
      explicit_accumulate(g.run + RUN_WINT, g.run + RUN_LOST + RUN_WINT, hdt * part[0][SUM_INT]);
      explicit_accumulate(g.run + RUN_WDAMP, g.run + RUN_LOST + RUN_WDAMP, hdt * part[0][SUM_DAMP]);
      explicit_accumulate(g.run + RUN_WEXT, g.run + RUN_LOST + RUN_WEXT, g.dt * part[0][SUM_LOAD] + hdt * part[0][SUM_REACT]);
    }
    *g.ticket = 0u;      // for the next launch on the stream
  }
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_explicit_s : StreamHandle {
  int64_t n = 0, steps = 0;
  bool has_mass = false, started = false;
  DeviceBuffer<unsigned char> mask;
  DeviceBuffer<double> vbar, m, a, partials, run;
  DeviceBuffer<unsigned> ticket;
  DeviceBuffer<int> status;
  const double* r_prev = nullptr;   // the caller's buffers of the previous step: kept by pointer, never copied
  const double* d_prev = nullptr;
  double* run_host = nullptr;       // pinned
  int* status_host = nullptr;       // pinned
  ~mimi_hip_explicit_s() {
    if (run_host) (void)hipHostFree(run_host);
    if (status_host) (void)hipHostFree(status_host);
  }
};

namespace {

void device_only(const void* p, const char* entry, const char* name) {
  if (p && !is_device_pointer(p))
    fail("%s: %s is a host pointer; the explicit step takes device-resident vectors only (a staged copy per step would "
         "defeat it)", entry, name);
}

void explicit_check_status(mimi_hip_explicit_s* h) {
  MH_HIP(hipMemcpyAsync(h->status_host, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  if (*h->status_host) {
    MH_HIP(hipMemsetAsync(h->status.ptr, 0, sizeof(int), h->stream));
    fail("explicit step: the lumped mass is not positive on a free or constant-velocity dof");
  }
}

void explicit_launch(mimi_hip_explicit_s* h, bool start, double dt, const double* f, const double* r, const double* d, double* v) {
  ExplicitArgs g{};
  g.n = h->n;
  g.dt = dt;
  g.mask = h->mask.ptr;
  g.vbar = h->vbar.ptr;
  g.m = h->m.ptr;
  g.f = f;
  g.r = r;
  g.r_prev = h->r_prev;
  g.d = d;
  g.d_prev = h->d_prev;
  g.a = h->a.ptr;
  g.v = v;
  g.partials = h->partials.ptr;
  g.run = h->run.ptr;
  g.ticket = h->ticket.ptr;
  if (start) hipLaunchKernelGGL(explicit_correct_kernel<1>, dim3(explicit_grid(h->n)), dim3(EXPLICIT_BLOCK), 0, h->stream, g);
  else hipLaunchKernelGGL(explicit_correct_kernel<0>, dim3(explicit_grid(h->n)), dim3(EXPLICIT_BLOCK), 0, h->stream, g);
  MH_HIP(hipGetLastError());
  // the swap: this step's buffers are the next step's previous ones
  h->r_prev = r;
  h->d_prev = d;
}

}  // namespace

extern "C" {

int mimi_hip_explicit_create(int64_t n, const unsigned char* fixed, const unsigned char* prescribed, const double* prescribed_velocity,
                             int device, mimi_hip_explicit_t* out) {
  return guarded([&] {
    if (!out) fail("null argument");
    if (n < 1) fail("n %lld out of range", (long long)n);
    if (prescribed && !prescribed_velocity) fail("a constant-velocity mask needs the prescribed velocities");
    auto h = std::make_unique<mimi_hip_explicit_s>();
    h->open(device);
    h->n = n;
    DeviceBuffer<unsigned char> d_fixed, d_pres;
    if (fixed) d_fixed.assign(fixed, (size_t)n, h->stream);
    if (prescribed) d_pres.assign(prescribed, (size_t)n, h->stream);
    h->mask.resize((size_t)n);
    hipLaunchKernelGGL(explicit_mask_kernel, dim3(explicit_grid(n)), dim3(EXPLICIT_BLOCK), 0, h->stream, n, d_fixed.ptr, d_pres.ptr,
                       h->mask.ptr);
    MH_HIP(hipGetLastError());
    h->vbar.resize((size_t)n);
    if (prescribed) h->vbar.assign(prescribed_velocity, (size_t)n, h->stream);
    else MH_HIP(hipMemsetAsync(h->vbar.ptr, 0, (size_t)n * sizeof(double), h->stream));
    h->m.resize((size_t)n);
    h->a.resize((size_t)n);
    MH_HIP(hipMemsetAsync(h->a.ptr, 0, (size_t)n * sizeof(double), h->stream));
    h->partials.resize((size_t)EXPLICIT_N_SUMS * EXPLICIT_GRID_CAP);
    h->run.resize(N_RUN_ALL);
    MH_HIP(hipMemsetAsync(h->run.ptr, 0, N_RUN_ALL * sizeof(double), h->stream));
    h->ticket.resize(1);
    MH_HIP(hipMemsetAsync(h->ticket.ptr, 0, sizeof(unsigned), h->stream));
    h->status.resize(1);
    MH_HIP(hipMemsetAsync(h->status.ptr, 0, sizeof(int), h->stream));
    MH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->run_host), N_RUN * sizeof(double), hipHostMallocDefault));
    MH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->status_host), sizeof(int), hipHostMallocDefault));
    *h->status_host = 0;
    MH_HIP(hipStreamSynchronize(h->stream));   // (the temporaries of the masks go out of scope)
    *out = h.release();
  });
}

int64_t mimi_hip_explicit_info(mimi_hip_explicit_t h, int what) {
  switch (what) {          // the shape of the sums: no handle needed
    case MIMI_HIP_EXPLICIT_INFO_SUM_BLOCK: return EXPLICIT_BLOCK;
    case MIMI_HIP_EXPLICIT_INFO_SUM_GRID_CAP: return EXPLICIT_GRID_CAP;
    case MIMI_HIP_EXPLICIT_INFO_SUM_FINAL_RUN: return EXPLICIT_FINAL_RUN;
    case MIMI_HIP_EXPLICIT_INFO_SUM_TREE_DEPTH: return EXPLICIT_TREE_DEPTH;
    default: break;
  }
  if (!h) return -1;
  switch (what) {
    case MIMI_HIP_EXPLICIT_INFO_N: return h->n;
    case MIMI_HIP_EXPLICIT_INFO_R_PREV: return (int64_t)(intptr_t)h->r_prev;
    case MIMI_HIP_EXPLICIT_INFO_D_PREV: return (int64_t)(intptr_t)h->d_prev;
    case MIMI_HIP_EXPLICIT_INFO_STEPS: return h->steps;
    case MIMI_HIP_EXPLICIT_INFO_GRID: return explicit_grid(h->n);
    default: return -1;
  }
}

int mimi_hip_explicit_set_stream(mimi_hip_explicit_t h, void* stream) { return handle_set_stream(h, stream); }
int mimi_hip_explicit_destroy(mimi_hip_explicit_t h) { return handle_destroy(h); }

int mimi_hip_explicit_synchronize(mimi_hip_explicit_t h) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    explicit_check_status(h);
  });
}

int mimi_hip_explicit_set_mass(mimi_hip_explicit_t h, const double* m) {
  return guarded([&] {
    if (!h || !m) fail("null argument");
    device_only(m, "set_mass", "m");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(h->m.ptr, m, (size_t)h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(explicit_mass_check_kernel, dim3(explicit_grid(h->n)), dim3(EXPLICIT_BLOCK), 0, h->stream, h->n, h->mask.ptr,
                       h->m.ptr, h->status.ptr);
    MH_HIP(hipGetLastError());
    h->has_mass = true;
    h->started = false;
  });
}

int mimi_hip_explicit_start(mimi_hip_explicit_t h, double* v, const double* f, const double* r, const double* d) {
  return guarded([&] {
    if (!h || !v || !r) fail("null argument");
    if (!h->has_mass) fail("start before set_mass");
    device_only(v, "start", "v");
    device_only(f, "start", "f");
    device_only(r, "start", "r");
    device_only(d, "start", "d");
    MH_HIP(hipSetDevice(h->device));
    explicit_launch(h, true, 0.0, f, r, d, v);
    h->started = true;
    h->steps = 0;
  });
}

int mimi_hip_explicit_predict(mimi_hip_explicit_t h, double dt, double* x, double* v) {
  return guarded([&] {
    if (!h || !x || !v) fail("null argument");
    if (!h->started) fail("predict before start");
    device_only(x, "predict", "x");
    device_only(v, "predict", "v");
    MH_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(explicit_predict_kernel, dim3(explicit_grid(h->n)), dim3(EXPLICIT_BLOCK), 0, h->stream, h->n, dt, h->mask.ptr,
                       h->vbar.ptr, h->a.ptr, x, v);
    MH_HIP(hipGetLastError());
  });
}

int mimi_hip_explicit_correct(mimi_hip_explicit_t h, double dt, const double* f, const double* r, const double* d, double* v) {
  return guarded([&] {
    if (!h || !v || !r) fail("null argument");
    if (!h->started) fail("correct before start");
    device_only(f, "correct", "f");
    device_only(r, "correct", "r");
    device_only(d, "correct", "d");
    device_only(v, "correct", "v");
    if (r == h->r_prev || (d && d == h->d_prev))
      fail("correct: r / d is the buffer of the previous step, which the ledger still reads: alternate two buffers");
    if (!d != !h->d_prev) fail("correct: the damping force must be given in every call since start, or in none");
    MH_HIP(hipSetDevice(h->device));
    explicit_launch(h, false, dt, f, r, d, v);
    ++h->steps;
  });
}

int mimi_hip_explicit_acceleration(mimi_hip_explicit_t h, double* a) {
  return guarded([&] {
    if (!h || !a) fail("null argument");
    device_only(a, "acceleration", "a");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(a, h->a.ptr, (size_t)h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  });
}

int mimi_hip_explicit_energies(mimi_hip_explicit_t h, double dt, double* out6) {
  return guarded([&] {
    if (!h || !out6) fail("null argument");
    if (!h->started) fail("energies before start");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(h->run_host, h->run.ptr, N_RUN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    explicit_check_status(h);      // (synchronises)
    const double* s = h->run_host;
    const double ke = 0.5 * s[RUN_MV2], q = (dt * dt * 0.125) * s[RUN_MA2];
    out6[0] = ke;
    out6[1] = s[RUN_WINT];
    out6[2] = s[RUN_WEXT];
    out6[3] = s[RUN_WDAMP];
    out6[4] = q;
    out6[5] = ke - q + s[RUN_WINT] + s[RUN_WDAMP] - s[RUN_WEXT];
  });
}

}  // extern "C"
