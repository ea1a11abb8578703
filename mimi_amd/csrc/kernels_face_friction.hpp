// Coulomb friction of the mortar contact integrator (contact.hip fills FrictionArgs and launches): a penalty-regularised
// tangential traction t at every face point, on the layout of the frictionless pass 2 -- one WAVE per face, lane =
// quadrature point for the point quantities (handed round by face_lane_read), lane = (i, a) for the residual entries, lane =
// node pair for the DIM x DIM tangent blocks.  The kernels ADD into face_r / face_k behind contact_residual_wave_kernel /
// contact_tangent_kernel, so the fixed-order row gather of face_common.hpp assembles friction with everything else: no
// atomics, sums in a fixed order, equal bytes from equal inputs.  The reference has no friction; the model is DESIGN.md's:
//   p_N = -p_h;  p_N = 0: t = 0, trial (xi' = 0, c' = 0);  p_N > 0 and c = 0: t = 0, trial (0, 1);
//   p_N > 0 and c = 1: a = xi + x_q - xbar - d, s = (I - n n^T) a,
//     stick (eps_T |s| <= mu p_N): t = eps_T s, xi' = s;   slip: t = mu p_N s / |s|, xi' = t / eps_T;   c' = 1;
//   xbar' = x_q always;   r(a,i) += sum_q w |m| N_a t_i;
//   K(ai,bj) = sum_q w N_a (t_i n_k D_kbj + |m| dt_i / dx_bj), D = dm / dx, with p_A, xi, xbar, d, c and the branch frozen.
// State arrays are [n_faces][DIM][n_q] (c: [n_faces][n_q]): the lanes of a wave, one per point, read and write neighbours.
// An evaluation writes the TRIAL arrays only; contact_friction_commit_kernel copies them over the committed ones.
#pragma once

#include <hip/hip_runtime.h>

#include "face_common.hpp"

namespace mimi_hip {

constexpr int kFrictionScalars = 6;   // per face and in total: force[3] = sum da t, sum da |t|, sticking points, slipping points

struct FrictionArgs {
  // the face tables and stores of the contact handle (ContactArgs of contact.hip)
  int n_faces, n_dof, n_q;
  const int32_t* dofs;       // [n_faces][n_dof] global node ids
  const int32_t* local;      // [n_faces][n_dof] index into the nodal arrays
  const double* N;           // [n_faces][n_q][n_dof]
  const double* dN;          // [n_faces][n_q][dim-1][n_dof]
  const double* weight;      // [n_faces][n_q]
  const double* x_ref;       // [n_nodes][dim]
  const double* u;
  const double* pressure;    // [n_marked] nodal pressures of this evaluation
  double* face_r;            // [n_faces][dim][n_dof]  written by contact_residual_wave_kernel before
  double* face_k;            // [n_faces][(a, i)][(j, b)]  written by contact_tangent_kernel before
  // friction
  double mu, eps_t;
  double d[3];               // the rigid body's displacement over the current step
  const double* xi;          // committed: [n_faces][dim][n_q] elastic slip
  const double* xbar;        //            [n_faces][dim][n_q] position at the last commit
  const unsigned char* c;    //            [n_faces][n_q]      in contact at the last commit
  double* xi_t;              // trial, same shapes
  double* xbar_t;
  unsigned char* c_t;
  double* face_fr;           // [n_faces][kFrictionScalars]
};

// what lane q holds of its point after friction_point
template<int DIM>
struct FrictionPoint {
  double w, detJ, n[DIM], tq[(DIM - 1) * DIM];   // weight, |m|, unit normal, surface tangents
  double a[DIM], t[DIM], sh[DIM], coef;          // a; the traction; s / |s|; eps_T (stick) or mu p_N / |s| (slip)
  int br;                                        // 0 no friction, 1 stick, 2 slip
};

// lane c < n_dof holds node c of face f (pressure pc, position xc); lane q < n_q evaluates point q (the other lanes return
// br = 0) and, with `store`, writes the trial state of its point
template<int DIM>
MH_DEV FrictionPoint<DIM> friction_point(const FrictionArgs& fr, int f, int lane, double pc, const double* xc,
                                         bool store) {
  FrictionPoint<DIM> P;
  const int n_dof = fr.n_dof, n_q = fr.n_q;
  const bool on = lane < n_q;
  const int q = on ? lane : 0;
  const int64_t pt = (int64_t)f * n_q + q;
  const double* N = fr.N + pt * n_dof;
  const double* dN = fr.dN + pt * n_dof * (DIM - 1);
  double pq = 0.0, xq[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xq[i] = 0.0;
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) P.tq[k] = 0.0;
  for (int c = 0; c < n_dof; ++c) {
    pq = __builtin_fma(N[c], face_lane_read(pc, c), pq);
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double x = face_lane_read(xc[i], c);
      xq[i] = __builtin_fma(x, N[c], xq[i]);
#pragma unroll
      for (int k = 0; k < DIM - 1; ++k) P.tq[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], P.tq[k * DIM + i]);
    }
  }
  double m[DIM], mm = 0.0;
  face_normal<DIM>(P.tq, m);
#pragma unroll
  for (int i = 0; i < DIM; ++i) mm += m[i] * m[i];
  P.detJ = sqrt(mm);
  P.w = fr.weight[pt];
#pragma unroll
  for (int i = 0; i < DIM; ++i) P.n[i] = m[i] / P.detJ;
  const double pn = -pq;
  const bool in = on && pn > 0.0;
  double xi_new[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) P.a[i] = P.t[i] = P.sh[i] = xi_new[i] = 0.0;
  P.coef = 0.0;
  P.br = 0;
  if (in && fr.c[pt]) {
    double na = 0.0, s[DIM], sn = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const int64_t k = ((int64_t)f * DIM + i) * n_q + q;
      P.a[i] = fr.xi[k] + (xq[i] - fr.xbar[k]) - fr.d[i];
      na += P.n[i] * P.a[i];
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      s[i] = P.a[i] - P.n[i] * na;
      sn += s[i] * s[i];
    }
    sn = sqrt(sn);
    const double lim = fr.mu * pn;
    if (fr.eps_t * sn <= lim) {
      P.br = 1;
      P.coef = fr.eps_t;
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        P.t[i] = fr.eps_t * s[i];
        xi_new[i] = s[i];
        P.sh[i] = sn > 0.0 ? s[i] / sn : 0.0;
      }
    } else {
      P.br = 2;
      P.coef = lim / sn;
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        P.sh[i] = s[i] / sn;
        P.t[i] = lim * P.sh[i];
        xi_new[i] = P.t[i] / fr.eps_t;
      }
    }
  }
  if (store && on) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const int64_t k = ((int64_t)f * DIM + i) * n_q + q;
      fr.xi_t[k] = xi_new[i];
      fr.xbar_t[k] = xq[i];
    }
    fr.c_t[pt] = in ? 1 : 0;
  }
  return P;
}

// lane c < n_dof: the pressure and the position of node c of face f
template<int DIM>
MH_DEV void friction_face_nodes(const FrictionArgs& fr, int f, int lane, double& pc, double* xc) {
  pc = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < fr.n_dof) {
    pc = fr.pressure[fr.local[(int64_t)f * fr.n_dof + lane]];
    const int64_t node = fr.dofs[(int64_t)f * fr.n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = fr.u[node * DIM + i] + fr.x_ref[node * DIM + i];
  }
}

// point evaluation, trial-state store, face residual and history scalars of the face.  A face none of whose points carries
// a traction leaves face_r alone (it may be an inactive face, whose face_r nobody wrote).
template<int DIM>
__global__ __launch_bounds__(256) void contact_friction_kernel(FrictionArgs fr) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= fr.n_faces) return;
  const int n_dof = fr.n_dof, n_q = fr.n_q, NT = n_dof * DIM;
  double pc, xc[DIM];
  friction_face_nodes<DIM>(fr, f, lane, pc, xc);
  const FrictionPoint<DIM> P = friction_point<DIM>(fr, f, lane, pc, xc, true);
  double* hist = fr.face_fr + (int64_t)f * kFrictionScalars;
  if (__ballot(P.br != 0) == 0) {
    if (lane < kFrictionScalars) hist[lane] = 0.0;
    return;
  }
  // lane q: da t_i and da |t|
  const double da = P.w * P.detJ;
  double dat[DIM], tt = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    dat[i] = da * P.t[i];
    tt += P.t[i] * P.t[i];
  }
  const double datn = da * sqrt(tt);
  // lane k = i n_dof + a: R(a, i) = sum_q (da t_i)_q N_q[a], over the points in order
  {
    const int k = lane < NT ? lane : 0, i = k / n_dof, a = k % n_dof;
    double R = 0.0;
    for (int q = 0; q < n_q; ++q) {
      double v = face_lane_read(dat[0], q);
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double vi = face_lane_read(dat[ii], q);
        v = i == ii ? vi : v;
      }
      R += v * fr.N[((int64_t)f * n_q + q) * n_dof + a];
    }
    if (lane < NT) fr.face_r[(int64_t)f * NT + lane] += R;      // [i][a]
  }
  // history of the face, in the order of the points (every lane the same sums; lane 0 stores)
  {
    double force[3] = {0.0, 0.0, 0.0}, trac = 0.0, n_stick = 0.0, n_slip = 0.0;
    for (int q = 0; q < n_q; ++q) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) force[i] += face_lane_read(dat[i], q);
      trac += face_lane_read(datn, q);
      const int br = __builtin_amdgcn_readlane(P.br, q);
      n_stick += br == 1 ? 1.0 : 0.0;
      n_slip += br == 2 ? 1.0 : 0.0;
    }
    if (lane == 0) {
      hist[0] = force[0];
      hist[1] = force[1];
      hist[2] = force[2];
      hist[3] = trac;
      hist[4] = n_stick;
      hist[5] = n_slip;
    }
  }
}

// the friction tangent of the face added to its block of face_k (which contact_tangent_kernel wrote before): stage 1 as
// above without the store, stage 2 lane = node pair (a, b), the point's numbers read from the lane that computed them
template<int DIM>
__global__ __launch_bounds__(256) void contact_friction_tangent_kernel(FrictionArgs fr) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= fr.n_faces) return;
  const int n_dof = fr.n_dof, n_q = fr.n_q;
  double pc, xc[DIM];
  friction_face_nodes<DIM>(fr, f, lane, pc, xc);
  const FrictionPoint<DIM> P = friction_point<DIM>(fr, f, lane, pc, xc, false);
  if (__ballot(P.br != 0) == 0) return;
  double naq = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) naq += P.n[i] * P.a[i];
  const int n_pairs = n_dof * n_dof, NT = n_dof * DIM;
  double* Kf = fr.face_k + (int64_t)f * NT * NT;
  for (int pair0 = 0; pair0 < n_pairs; pair0 += 64) {
    const int pair = pair0 + lane;
    const bool on = pair < n_pairs;
    const int a = on ? pair / n_dof : 0, b = on ? pair % n_dof : 0;
    double acc[DIM * DIM];
#pragma unroll
    for (int k = 0; k < DIM * DIM; ++k) acc[k] = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const int br = __builtin_amdgcn_readlane(P.br, q);
      if (br == 0) continue;   // (wave-uniform)
      const int64_t pt = (int64_t)f * n_q + q;
      const double* dN = fr.dN + pt * n_dof * (DIM - 1);
      const double Nb = fr.N[pt * n_dof + b];
      const double wN = face_lane_read(P.w, q) * fr.N[pt * n_dof + a];
      const double detJ = face_lane_read(P.detJ, q), na = face_lane_read(naq, q), coef = face_lane_read(P.coef, q);
      double n[DIM], av[DIM], tv[DIM], sh[DIM], t[(DIM - 1) * DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        n[i] = face_lane_read(P.n[i], q);
        av[i] = face_lane_read(P.a[i], q);
        tv[i] = face_lane_read(P.t[i], q);
        sh[i] = face_lane_read(P.sh[i], q);
      }
      if constexpr (DIM == 3) {
#pragma unroll
        for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = face_lane_read(P.tq[k], q);
      }
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        double dm[DIM];   // d m / d x_bj
        if constexpr (DIM == 2) {
          dm[0] = (j == 1) ? dN[b] : 0.0;
          dm[1] = (j == 0) ? -dN[b] : 0.0;
        } else {
          double e[3] = {0, 0, 0};
          e[j] = 1.0;
          const double* t1 = t;
          const double* t2 = t + 3;
          const double d1 = dN[b], d2 = dN[n_dof + b];
          dm[0] = d1 * (e[1] * t2[2] - e[2] * t2[1]) + d2 * (t1[1] * e[2] - t1[2] * e[1]);
          dm[1] = d1 * (e[2] * t2[0] - e[0] * t2[2]) + d2 * (t1[2] * e[0] - t1[0] * e[2]);
          dm[2] = d1 * (e[0] * t2[1] - e[1] * t2[0]) + d2 * (t1[0] * e[1] - t1[1] * e[0]);
        }
        double nD = 0.0;   // d |m|
#pragma unroll
        for (int k = 0; k < DIM; ++k) nD += n[k] * dm[k];
        double dn[DIM], dna = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          dn[i] = (dm[i] - n[i] * nD) / detJ;
          dna += dn[i] * av[i];
        }
        double ds[DIM], shds = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          ds[i] = ((i == j ? 1.0 : 0.0) - n[i] * n[j]) * Nb - dn[i] * na - n[i] * dna;
          shds += sh[i] * ds[i];
        }
        if (br == 1) shds = 0.0;   // stick: dt = eps_T ds; slip: dt = (mu p_N / |s|) (I - sh sh^T) ds
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double dt = coef * (ds[i] - sh[i] * shds);
          acc[i * DIM + j] += wN * (tv[i] * nD + detJ * dt);
        }
      }
    }
    if (on) {
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int j = 0; j < DIM; ++j) Kf[(a * DIM + i) * NT + j * n_dof + b] += acc[i * DIM + j];
    }
  }
}

// commit: the trial state over the committed one (n_state = n_points * dim doubles each, n_points flags)
__global__ void contact_friction_commit_kernel(int64_t n_state, int64_t n_points, const double* __restrict__ xi_t,
                                               const double* __restrict__ xbar_t, const unsigned char* __restrict__ c_t,
                                               double* __restrict__ xi, double* __restrict__ xbar, unsigned char* __restrict__ c) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_state) {
    xi[k] = xi_t[k];
    xbar[k] = xbar_t[k];
  }
  if (k < n_points) c[k] = c_t[k];
}

}  // namespace mimi_hip
