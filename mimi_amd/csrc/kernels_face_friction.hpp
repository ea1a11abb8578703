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
// Wave index, node load, point stage, normal column, point scatter and the node-pair loop are face_wave.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include "face_common.hpp"

namespace mimi_hip {

constexpr int kFrictionScalars = 6;   // per face and in total: force[3] = sum da t, sum da |t|, sticking points, slipping points

struct FrictionArgs {
  // the face tables and stores of the contact handle (ContactArgs of contact.hip)
  FaceView v;
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
MH_WAVE FrictionPoint<DIM> friction_point(const FrictionArgs& fr, int f, int lane, double pc, const double* xc,
                                         bool store) {
  FrictionPoint<DIM> P;
  const int n_q = fr.v.n_q;
  const bool on = lane < n_q;
  const int q = on ? lane : 0;
  const int64_t pt = face_lane_point(fr.v, f, lane);
  double pq, xq[DIM], m[DIM], mm = 0.0;
  face_point_stage<DIM, true, true, true>(fr.v, pt, pc, xc, &pq, xq, P.tq);
  face_normal<DIM>(P.tq, m);
#pragma unroll
  for (int i = 0; i < DIM; ++i) mm += m[i] * m[i];
  P.detJ = sqrt(mm);
  P.w = fr.v.weight[pt];
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
MH_WAVE void friction_face_nodes(const FrictionArgs& fr, int f, int lane, double& pc, double* xc) {
  pc = face_load_nodes<DIM, true, kNodal>(fr.v, f, lane, fr.u, xc, fr.pressure);
}

// point evaluation, trial-state store, face residual and history scalars of the face.  A face none of whose points carries
// a traction leaves face_r alone (it may be an inactive face, whose face_r nobody wrote).
template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_friction_kernel(FrictionArgs fr) {
  int lane, f;
  if (!face_wave_index(fr.v, lane, f)) return;
  const int n_q = fr.v.n_q, NT = fr.v.n_dof * DIM;
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
  const double R = face_scatter_points<DIM, false>(fr.v, f, face_lane_entry<DIM>(fr.v, lane), dat);
  if (lane < NT) fr.face_r[(int64_t)f * NT + lane] += R;      // [i][a]
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
__global__ __launch_bounds__(kFaceWaveThreads) void contact_friction_tangent_kernel(FrictionArgs fr) {
  int lane, f;
  if (!face_wave_index(fr.v, lane, f)) return;
  const int n_dof = fr.v.n_dof, n_q = fr.v.n_q;
  double pc, xc[DIM];
  friction_face_nodes<DIM>(fr, f, lane, pc, xc);
  const FrictionPoint<DIM> P = friction_point<DIM>(fr, f, lane, pc, xc, false);
  if (__ballot(P.br != 0) == 0) return;
  double naq = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) naq += P.n[i] * P.a[i];
  face_pair_loop<DIM, true>(n_dof, lane, fr.face_k + (int64_t)f * (n_dof * DIM) * (n_dof * DIM), [&](int a, int b, double* acc) {
    for (int q = 0; q < n_q; ++q) {
      const int br = __builtin_amdgcn_readlane(P.br, q);
      if (br == 0) continue;   // (wave-uniform)
      const int64_t pt = (int64_t)f * n_q + q;
      const double* dN = fr.v.dN + pt * n_dof * (DIM - 1);
      const double Nb = fr.v.N[pt * n_dof + b];
      const double wN = face_lane_read(P.w, q) * fr.v.N[pt * n_dof + a];
      const double detJ = face_lane_read(P.detJ, q), na = face_lane_read(naq, q), coef = face_lane_read(P.coef, q);
      double n[DIM], av[DIM], tv[DIM], sh[DIM], t[(DIM - 1) * DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        n[i] = face_lane_read(P.n[i], q);
        av[i] = face_lane_read(P.a[i], q);
        tv[i] = face_lane_read(P.t[i], q);
        sh[i] = face_lane_read(P.sh[i], q);
      }
#pragma unroll
      for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = face_lane_read(P.tq[k], q);
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        double dm[DIM];   // d m / d x_bj
        face_normal_column<DIM>(t, dN, n_dof, b, j, dm);
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
  });
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
