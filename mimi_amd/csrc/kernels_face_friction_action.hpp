// Coulomb friction on the matrix-free route: the tangent of contact_friction_tangent_kernel (kernels_face_friction.hpp)
// applied to a vector, on top of the frozen-pressure action (kernels_face_action.hpp) or the consistent one
// (kernels_face_consistent.hpp), whichever the record holds.  With tau the traction of a face point (t = mu p_N s / |s| in
// slip, eps_T s in stick; the letter t is the surface tangents' in the action kernels), for a direction v:
//   dx_q = sum_b N_b v_b,   nD = n.dm = d|m|,   dn = (dm - n nD) / |m|,
//   ds   = (I - n n^T) dx_q - dn (n.a) - n (dn.a),
//   dtau = coef (ds - [slip] sh (sh.ds)),   coef = eps_T (stick), mu p_N / |s| (slip),   sh = s / |s|,
//   consistent record, slip:  dtau -= mu dp_q sh   (p_N = -p_q; the frozen friction tangent drops this first-order term of
//                                                    the friction residual itself),
//   g_i += w (tau_i nD + |m| dtau_i),   tau = coef s in both branches
// and (K v)(a, i) = sum_q g_i(q) N_q[a] as ever.
//   record   on top of coef / tang / active and, when set, the consistent record: per face point a_q = xi + x_q - xbar - d
//            (dim doubles), coef_q (one double; 0 where the point carries no traction) and the branch (one byte: 0 none,
//            1 stick, 2 slip); per record mu.  n and |m| come from the recorded tangents, s, sh and tau from a and n.
//              bytes = n_faces n_q (8 (dim + 1) + 1) + 8
//            Written by friction_point with store = false on the COMMITTED state, d, mu, eps_T of that moment and the nodal
//            pressure the linearisation has just formed: the trial state, face_fr and the history scalars are not touched,
//            nothing of u is kept.
//   action   ONE face kernel in the place of boundary_action_kernel (frozen record) or contact_consistent_action_kernel
//            (consistent record): friction adds no launch to a product.  Stage 1, lane = point, forms g with the friction
//            terms; stage 2, lane = (i, a), and the node sum are those of the frictionless actions.  A point with branch 0
//            adds nothing.
// One wave per face, four faces per workgroup, registers only: no LDS, no atomics, a fixed summation order -- equal inputs
// give equal bytes.  A record without friction (the action off, or mu = 0 at the linearize) launches what it always did.
// The record kernel stands on face_wave.hpp's stages; the action kernel has them in its own text (see there) and shares
// face_normal_rate.
// Only contact.hip includes this header.
#pragma once

#include "kernels_face_consistent.hpp"
#include "kernels_face_friction.hpp"

namespace mimi_hip {
namespace {

struct FrictionRecordArgs {
  double* a;                 // [n_faces][n_q][dim]
  double* coef;              // [n_faces][n_q]
  unsigned char* br;         // [n_faces][n_q]
};

// every face, active or not: a face without pressure gets branch 0 at all its points
template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_friction_record_kernel(FrictionArgs fr, FrictionRecordArgs rec) {
  int lane, f;
  if (!face_wave_index(fr.v, lane, f)) return;
  double pc, xc[DIM];
  friction_face_nodes<DIM>(fr, f, lane, pc, xc);
  const FrictionPoint<DIM> P = friction_point<DIM>(fr, f, lane, pc, xc, false);
  if (lane < fr.v.n_q) {   // (a contact face holds at most a wave's 64 points: checked at create)
    const int64_t pt = (int64_t)f * fr.v.n_q + lane;
#pragma unroll
    for (int i = 0; i < DIM; ++i) rec.a[pt * DIM + i] = P.a[i];
    rec.coef[pt] = P.coef;
    rec.br[pt] = (unsigned char)P.br;
  }
}

struct FrictionActionArgs {
  FaceView v;
  const double* coef;        // the frozen record
  const double* tang;
  const unsigned char* active;
  const double* fa;          // the friction record
  const double* fcoef;
  const unsigned char* fbr;
  double mu;
  const double* dp;          // [n_marked] of this product (CONSISTENT only)
  double factor;
  const double* x;
  double* face_y;            // [n_faces][dim][n_dof]
};

// (The kernel keeps its own stage text, the trips over the points included, although a face holds at most 64: written on
// face_wave.hpp's stages without the loop it was 9 .. 14 % faster where few faces are active and 0.3 % slower, in every set of
// runs, where all are -- profiles/face_wave_refactor.txt, section 6 -- and its times are to stay the parent's.)
template<int DIM, bool CONSISTENT>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_friction_action_kernel(FrictionActionArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.v.n_faces) return;
  if (!p.active[f]) return;   // (wave-uniform; the node sum skips the face, and a face without pressure has no friction point)
  const int n_dof = p.v.n_dof, n_q = p.v.n_q, NT = n_dof * DIM;
  double dpc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    if constexpr (CONSISTENT) dpc = p.dp[p.v.local[(int64_t)f * n_dof + lane]];
    const int64_t node = p.v.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.x[node * DIM + i];
  }
  const int k = lane < NT ? lane : 0, ki = k / n_dof, ka = k % n_dof;
  double Y = 0.0;
  for (int q0 = 0; q0 < n_q; q0 += 64) {
    // stage 1, lane = point q0 + lane: g = c_q dm [- w dp_q m] + w (tau nD + |m| dtau)
    double g[DIM];
    {
      const bool on = q0 + lane < n_q;
      const int64_t pt = (int64_t)f * n_q + (on ? q0 + lane : 0);
      const double* N = p.v.N + pt * n_dof;
      const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
      double dpq = 0.0, dx[DIM], dt[(DIM - 1) * DIM], t[(DIM - 1) * DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) dx[i] = 0.0;
#pragma unroll
      for (int kk = 0; kk < (DIM - 1) * DIM; ++kk) {
        dt[kk] = 0.0;
        t[kk] = p.tang[pt * ((DIM - 1) * DIM) + kk];
      }
      for (int c = 0; c < n_dof; ++c) {
        if constexpr (CONSISTENT) dpq = __builtin_fma(N[c], face_lane_read(dpc, c), dpq);
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double x = face_lane_read(xc[i], c);
          dx[i] = __builtin_fma(x, N[c], dx[i]);
#pragma unroll
          for (int kk = 0; kk < DIM - 1; ++kk) dt[kk * DIM + i] = __builtin_fma(x, dN[kk * n_dof + c], dt[kk * DIM + i]);
        }
      }
      double m[DIM], dm[DIM];
      face_normal_rate<DIM>(t, dt, m, dm);
      const double cq = on ? p.coef[pt] : 0.0, w = on ? p.v.weight[pt] : 0.0;
      if constexpr (CONSISTENT) {
        const double wdp = w * dpq;
#pragma unroll
        for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i] - wdp * m[i];
      } else {
#pragma unroll
        for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i];
      }
      const int br = on ? p.fbr[pt] : 0;
      if (br != 0) {
        double mm = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) mm += m[i] * m[i];
        const double len = sqrt(mm), coef = p.fcoef[pt];
        double n[DIM], a[DIM], na = 0.0, nD = 0.0, ndx = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          n[i] = m[i] / len;
          a[i] = p.fa[pt * DIM + i];
          na += n[i] * a[i];
          nD += n[i] * dm[i];
          ndx += n[i] * dx[i];
        }
        double s[DIM], dn[DIM], ss = 0.0, dna = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          s[i] = a[i] - n[i] * na;
          ss += s[i] * s[i];
          dn[i] = (dm[i] - n[i] * nD) / len;
          dna += dn[i] * a[i];
        }
        const bool slip = br == 2;
        const double inv = slip ? 1.0 / sqrt(ss) : 0.0;   // (slip: eps_T |s| > mu p_N >= 0)
        double ds[DIM], shds = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          ds[i] = (dx[i] - n[i] * ndx) - dn[i] * na - n[i] * dna;
          shds += (s[i] * inv) * ds[i];
        }
        const double along = (CONSISTENT && slip) ? p.mu * dpq : 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double sh = s[i] * inv;
          double dtau = coef * (ds[i] - sh * shds);
          if constexpr (CONSISTENT) dtau -= along * sh;
          g[i] += w * ((coef * s[i]) * nD + len * dtau);
        }
      }
    }
    // stage 2, lane = (i, a): the trip's points in ascending order
    const int n_trip = n_q - q0 < 64 ? n_q - q0 : 64;
    for (int q = 0; q < n_trip; ++q) {
      double gi = face_lane_read(g[0], q);
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double v = face_lane_read(g[ii], q);
        gi = ki == ii ? v : gi;
      }
      Y = __builtin_fma(gi, p.v.N[((int64_t)f * n_q + q0 + q) * n_dof + ka], Y);
    }
  }
  if (lane < NT) p.face_y[(int64_t)f * NT + lane] = p.factor * Y;   // [i][a]
}

// The record of a contact handle with the friction action on: ContactAction's, and on top of it the friction part when the
// linearisation that made it saw mu > 0.  `friction` is the record's own flag, like `consistent`: what the handle is set to
// reaches it at the next linearize only.  With the flag off none of the buffers below exists and add is ContactAction's.
struct FrictionContactAction : ContactAction {
  bool friction = false;
  double mu = 0.0;                       // of the linearisation
  DeviceBuffer<double> fa, fcoef;
  DeviceBuffer<unsigned char> fbr;

  int64_t bytes(const FaceSet& h) const {
    int64_t n = ContactAction::bytes(h);
    if (linearized && friction) n += (int64_t)h.n_faces * h.n_q * (8 * (h.dim + 1) + 1) + 8;
    return n;
  }

  // fr: the friction arguments at u_dev with the pressure of this linearisation, or nullptr (no friction part).  The friction
  // part goes first: ContactAction::linearize records the event that then stands behind everything
  template<class Body>
  void linearize(FaceSet& h, const double* u_dev, const double* area_now, const double* pressure_now, double penalty_now,
                 bool consistent_on, const Body& body, const FrictionArgs* fr, const double* gap_now = nullptr) {
    if (fr) {
      const size_t npts = (size_t)h.n_faces * h.n_q;
      fa.resize(npts * h.dim);
      fcoef.resize(npts);
      fbr.resize(npts);
      const FrictionRecordArgs rec{fa.ptr, fcoef.ptr, fbr.ptr};
      face_dispatch_dim(h.dim, [&](auto D) {
        launch(contact_friction_record_kernel<decltype(D)::value>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, h.stream, *fr, rec);
      });
      mu = fr->mu;
    }
    friction = fr != nullptr;
    ContactAction::linearize(h, u_dev, area_now, pressure_now, penalty_now, consistent_on, body, gap_now);
  }

  void add(FaceAssembly& h, double factor, const double* x, double* y, hipStream_t s) {
    if (!friction) {
      ContactAction::add(h, factor, x, y, s);
      return;
    }
    if (consistent) nodal_rates(h, x, s);
    const FrictionActionArgs a{h.view(), coef.ptr, tang.ptr, active.ptr, fa.ptr, fcoef.ptr, fbr.ptr, mu, dp.ptr, factor, x, face_y.ptr};
    face_dispatch_dim(h.dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      launch(consistent ? contact_friction_action_kernel<DIM, true> : contact_friction_action_kernel<DIM, false>,
             face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, s, a);
    });
    h.gather_vector(active.ptr, face_y.ptr, y, s);
  }
};

}  // namespace
}  // namespace mimi_hip
