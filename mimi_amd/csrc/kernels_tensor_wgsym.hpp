// Phase 1 for materials with a major-symmetric tangent (hyperelastic: dP_iJ/dF_jL = dP_jL/dF_iJ), p = 2, 3-D.
//
// K_(a,i),(b,j) = K_(b,j),(a,i): of the nine (i, j) blocks of an element only the six with i >= j
// are contracted; an off-diagonal block is stored twice, as computed into piece (element, i) and
// transposed (a <-> b) into piece (element, j).  The scratch layout and phase 2 are those of
// kernels_tensor_2phase.hpp; the stored matrix is exactly symmetric.
//
// Workgroup = 4 waves as in kernels_tensor_wgs.hpp (same roles, same register carry, same LDS
// hand-off), but TWO steps per element instead of three, and homogeneous ones -- the three
// contraction waves do equally expensive blocks in the same step (a diagonal block costs 0.73 of an
// off-diagonal one, and a lock step lasts as long as its slowest wave):
//
//   step D(e)   Y0: block (0,0) of element e   Y1: (1,1)   Y2: (2,2)     X: quadrature-point stage of e+1
//   step O(e)   Y0: block (1,0) of element e   Y1: (2,0)   Y2: (2,1)     X: rows 0, 1, 2 of element e+1
//   O(e) = [Y: read operands from LDS] barrier [X, Y: compute, write LDS] barrier;  D(e) runs free (no barriers):
//   what it reads was written before the previous barrier and nothing it writes is read before the next one
//
// The rows of Ahat of element e are written during O(e-1), read (into registers) in the read windows
// of D(e) and O(e) and rewritten during O(e): one LDS buffer, only the 54 entries (i, j <= i) kept.
// The three store-transposition buffers (one per piece i) are written by all three contraction waves
// during D(e) and O(e) and flushed, piece w by wave Y_w, in the read window of D(e+1).  A prologue
// step lets X write the rows of element 0; after the last element each contraction wave stores the carried
// rows (outside the lock steps).  Every wave executes 2 n + 1 barriers.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_tensor_wgs.hpp"
#include "wgsym_geometry.hpp"

namespace mimi_hip {

#ifndef WGSYM_PACK
#define WGSYM_PACK 1   // packing level of the S3 tiles (p2_tile_map.hpp p2_b1_packed): 0 a tile per chain, 1 shipped, 2 all
#endif

#ifndef WGSYM_DIAG_MODE
#define WGSYM_DIAG_MODE 2   // 2: contract only the a1 >= b1 chains of a diagonal block; 0: all nine
#endif

struct WgsymLds : P2Shape {
  static constexpr int off_ue = 0;                          // [3][27] (+1 pad)              X private
  static constexpr int off_tab = off_ue + 3 * ND + 1;       // [2 parity][3 dir][2][3][4]     X -> Y
  static constexpr int off_r = off_tab + 2 * 6 * NB * NQ;   // residual scratch, three rows    X private
  static constexpr int off_ah = off_r + p2_stage_r_size(3);  // [6 blocks (i, j <= i)][9 (m,n)][64]  X -> Y
  static constexpr int off_st = off_ah + 6 * 9 * NQ3;       // [3 i][1216] store transposition      Y
  static constexpr int off_dump = off_st + 3 * WgsLds::st_size;   // where lanes without an entry store (wgs_contract_block)
  static constexpr int off_cp = off_dump + 512;   // [3 contraction waves][4][64]: the riders' second carry value (wgs_contract_block)
  static constexpr int total = off_cp + 3 * 4 * 64;
  static_assert(2 * total * sizeof(double) <= 160 * 1024, "two workgroups per CU");
  // first Ahat entry of block (i, j), j <= i
  MH_DEV static constexpr int ah_block(int i, int j) { return (i * (i + 1) / 2 + j) * 9; }
};

// rows 0, 1, 2 of one element in one go: Ahat blocks (i, j <= i) -> LDS, residual pieces -> scratch_r
// (the three residual rows share their four LDS passes)
template<int KIND>
MH_DEV void wgsym_x_rows(const TensorArgs& p, double* lds, int lane, int64_t e, int par, const WgsPoint<KIND>& s) {
  using L = WgsymLds;
  constexpr int ND = L::ND, NQ3 = L::NQ3;
  static_assert(KIND == MIMI_HIP_MAT_NEOHOOKEAN, "symmetric-half kernel: hyperelastic materials only");
  const double* tab = lds + L::off_tab + par * WgsOperands::NT;
  double* AH = lds + L::off_ah;
  double* PH = lds + L::off_r;                  // [3 I][3 m][64]
#pragma unroll
  for (int I = 0; I < 3; ++I)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double c2gm = s.c2_w * s.G[m * 3 + I];
#pragma unroll
      for (int j = 0; j <= I; ++j) {
        const double c1gm = s.c1_w * s.G[m * 3 + j];
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          double v = c2gm * s.G[n * 3 + j] - c1gm * s.G[n * 3 + I];
          if (I == j) {
            const int lo = m < n ? m : n, hi = m < n ? n : m;
            v += s.mu_w * s.M[lo * 3 - lo * (lo - 1) / 2 + (hi - lo)];
          }
          AH[(L::ah_block(I, j) + m * 3 + n) * NQ3 + lane] = v;
        }
      }
    }
#pragma unroll
  for (int k = 0; k < 9; ++k) PH[k * NQ3 + lane] = s.Phat[k];   // k = I * 3 + m
  p2_stage_r<3>(tab, PH, lane, p.scratch_r + e * ND * 3, 0);
}

// ------------------------------------------------------------------------------------------------
// wave X, two steps per element
// ------------------------------------------------------------------------------------------------
template<int KIND>
MH_DEV void wgsym_x_loop(const TensorArgs& p, double* lds, int col0, int n_cols) {
  using L = WgsymLds;
  constexpr int P = L::P, NB = L::NB, NQ = L::NQ, ND = L::ND;
  const int lane = threadIdx.x & 63;
  double* ue = lds + L::off_ue;
  const int n_seq = n_cols * p.seg_len;   // the workgroup walks n_cols units back to back (ColumnWalk)
  ColumnWalk cq(p, col0);     // the element whose operands are requested next
  ColumnWalk cs = cq;         // the element of the next quadrature-point stage
  ColumnWalk cr = cq;         // the element whose rows are written next
  // the connectivity travels one element further ahead than the other operands
  int32_t node_n = lane < ND ? p.dofs[cq.e * ND + lane] : 0;
  double ue_r[3];
  WgsOperands op;
  // requests the operands of the element at cq (the walk moves on), and the node ids of the one after it
  auto request = [&]() {
#pragma unroll
    for (int c = 0; c < 3; ++c) ue_r[c] = p.u[(int64_t)node_n * 3 + c];
    op.request(p, cq, lane);
    if (cq.g + 1 < n_seq) {
      cq.advance(p);
      node_n = lane < ND ? p.dofs[cq.e * ND + lane] : 0;
    }
  };
  WgsPoint<KIND> s;
  // quadrature-point stage of the element at cs from the requested operands (tables -> LDS parity g & 1)
  auto point_stage = [&]() {
    double* tab = lds + L::off_tab + (cs.g & 1) * WgsOperands::NT;
    if (lane < ND) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ue[c * ND + lane] = ue_r[c];
    }
    op.tables_to_lds(tab, lane);
    double Ji[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ji[k] = op.geo[k];
    const double wd = op.geo[9];
    __builtin_amdgcn_wave_barrier();
    // F at the quadrature point of this lane, q = q0 + 4 q1 + 16 q2
    double F[9];
    {
      const int q0 = lane & 3, q1 = (lane >> 2) & 3, q2 = lane >> 4;
      double b0[NB], d0[NB], b1[NB], d1[NB], b2[NB], d2[NB];
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        b0[a] = tab_ptr<P>(tab, 0, 0)[a * NQ + q0];
        d0[a] = tab_ptr<P>(tab, 0, 1)[a * NQ + q0];
        b1[a] = tab_ptr<P>(tab, 1, 0)[a * NQ + q1];
        d1[a] = tab_ptr<P>(tab, 1, 1)[a * NQ + q1];
        b2[a] = tab_ptr<P>(tab, 2, 0)[a * NQ + q2];
        d2[a] = tab_ptr<P>(tab, 2, 1)[a * NQ + q2];
      }
      double H[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) H[k] = 0.0;
#pragma unroll
      for (int a2 = 0; a2 < NB; ++a2)
#pragma unroll
        for (int a1 = 0; a1 < NB; ++a1) {
          const double tbb = b1[a1] * b2[a2], tdb = d1[a1] * b2[a2], tbd = b1[a1] * d2[a2];
#pragma unroll
          for (int a0 = 0; a0 < NB; ++a0) {
            const int a = a0 + NB * (a1 + NB * a2);
            const double dn0 = d0[a0] * tbb, dn1 = b0[a0] * tdb, dn2 = b0[a0] * tbd;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              const double uu = ue[i * ND + a];
              H[i * 3 + 0] += uu * dn0;
              H[i * 3 + 1] += uu * dn1;
              H[i * 3 + 2] += uu * dn2;
            }
          }
          // keep the LDS reads of later (a1, a2) where they are (hoisted together they need 162 registers)
          #pragma unroll
          for (int k = 0; k < 9; ++k) asm volatile("" : "+v"(H[k]) : : "memory");
        }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int J = 0; J < 3; ++J) {
          double sf = (i == J) ? 1.0 : 0.0;
#pragma unroll
          for (int m = 0; m < 3; ++m) sf += H[i * 3 + m] * Ji[m * 3 + J];
          F[i + J * 3] = sf;
        }
    }
    wgs_neohookean_point(p.mat.m, F, Ji, wd, s);
    __builtin_amdgcn_wave_barrier();
    if (cs.g + 1 < n_seq) cs.advance(p);
  };

  request();
  point_stage();
  if (1 < n_seq) request();
  // ---- prologue: rows of element 0 ---------------------------------------------------------------------------
  wgsym_x_rows<KIND>(p, lds, lane, cr.e, 0, s);
  wgs_barrier();
  for (int it = 0; it < n_seq; ++it) {
    // ---- D(it), free running: quadrature-point stage of element it + 1 (touches nothing the other waves read
    // before the next barrier: its own ue / point data and the table buffer of the OTHER parity) -----------------
    if (it + 1 < n_seq) {
      point_stage();
      if (it + 2 < n_seq) request();
    }
    // ---- O(it), lock step: rows of element it + 1 once every contraction wave holds its operands of element it --
    wgs_barrier();
    if (it + 1 < n_seq) {
      cr.advance(p);
      wgsym_x_rows<KIND>(p, lds, lane, cr.e, (it + 1) & 1, s);
    }
    wgs_barrier();
  }
}

// ------------------------------------------------------------------------------------------------
// wave Y_W: diagonal block (W, W) in step D, off-diagonal block (I1, J1) in step O; flushes piece W
// ------------------------------------------------------------------------------------------------
template<int W>
MH_DEV void wgsym_y_loop(const TensorArgs& p, double* lds, int col0, int n_cols) {
  using L = WgsymLds;
  constexpr int NB2 = L::NB2, NQ3 = L::NQ3;
  // step O blocks: Y0 (1,0), Y1 (2,0), Y2 (2,1)
  constexpr int I1 = W == 0 ? 1 : 2, J1 = W == 2 ? 1 : 0;
  const WgsLane lc = wgs_lane_constants(true);
  const WgsPackLane pl = wgs_pack_lane_constants(lc);
  const int lane = lc.lane;
  const int n_seq = n_cols * p.seg_len;
  const double* AH0 = lds + L::off_ah + L::ah_block(W, W) * NQ3;
  const double* AH1 = lds + L::off_ah + L::ah_block(I1, J1) * NQ3;
  auto st_of = [&](int piece) -> double* { return lds + L::off_st + piece * WgsLds::st_size; };
  auto block_at = [&](int64_t e) -> double* { return p.scratch_k + e * (int64_t)P2Block::size; };
  ColumnWalk c(p, col0);
  int64_t e_prev = c.e;

  double C0[NB2], C1[NB2];  // packed carries of the two blocks
#pragma unroll
  for (int k = 0; k < NB2; ++k) C0[k] = C1[k] = 0.0;
  // the riders' second carry value (packed tiles, p2_tile_map.hpp), one per packed b1, in this lane's own LDS slots: the
  // diagonal block has one packed b1, the off-diagonal block three
  double* const CP0 = lds + L::off_cp + W * 4 * 64;
  double* const CP1 = CP0 + 64;
#pragma unroll
  for (int k = 0; k < 4; ++k) CP0[k * 64 + lane] = 0.0;
  double aS0[4], aS2[4];
  double uB1[L::NB][L::NQ], uD1[L::NB][L::NQ];

  // ---- prologue: X writes the rows of element 0 ---------------------------------------------------------------
  wgs_barrier();
  for (int it = 0; it < n_seq; ++it) {
    // ---- D(it), free running: flush element it - 1, tables of element it, diagonal block ----------------------
    {
      if (it >= 1) wgs_flush_final(lane, st_of(W), block_at(e_prev), W);
      wgs_load_tables(lds + L::off_tab + (it & 1) * WgsOperands::NT, lane, c.pos == 0, aS0, aS2, uB1, uD1);
      double ah[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) ah[k] = AH0[k * NQ3 + lane];
      // no barriers around the diagonal block: it reads operands nobody rewrites before O(it)'s first barrier and
      // writes only slots of this wave's own buffer that no other wave touches (the transposed entries other
      // waves add to it during O steps use the other two column components)
      wgs_contract_block<WGSYM_DIAG_MODE, true, WGSYM_PACK>(lc, ah, aS0, aS2, uB1, uD1, C0, st_of(W), W, st_of(W), W, lds + L::off_dump,
                                                                   &pl, CP0);
    }
    // ---- O(it), lock step: off-diagonal block, stored as computed and transposed ------------------------------
    {
      double ah[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) ah[k] = AH1[k * NQ3 + lane];
      wgs_barrier();
      wgs_contract_block<1, true, WGSYM_PACK>(lc, ah, aS0, aS2, uB1, uD1, C1, st_of(I1), J1, st_of(J1), I1, lds + L::off_dump, &pl, CP1);
      wgs_barrier();
      if (c.pos == p.seg_len - 1) {
        // last element of a unit (column, or column segment): the carried rows have no successor -- straight from the registers into the third
        // part of the pieces (no LDS, no lock step) -- and the next column starts with an empty carry
        double* E = block_at(c.e);
        wgs_stage_carry<WGSYM_DIAG_MODE, WGSYM_PACK>(lc, C0, P2Block::carry_of(E, W), W, P2Block::carry_of(E, W), W, CP0);
        wgs_stage_carry<1, WGSYM_PACK>(lc, C1, P2Block::carry_of(E, I1), J1, P2Block::carry_of(E, J1), I1, CP1);
#pragma unroll
        for (int k = 0; k < NB2; ++k) C0[k] = C1[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) CP0[k * 64 + lane] = 0.0;
      }
    }
    e_prev = c.e;
    if (it + 1 < n_seq) c.advance(p);
  }
  // ---- after the last element (no more lock steps): its pieces from the buffers ------------------------------------
  wgs_flush_final(lane, st_of(W), block_at(e_prev), W);
}

template<int KIND>
__global__ __launch_bounds__(256, 2) void tensor_wgsym_kernel(TensorArgs p) {
  extern __shared__ __align__(16) double smem_wgsym[];
  const int role = __builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) + WGS_ROT(blockIdx.x)) & 3);
  const int n_cols_all = p.box_n[0] * p.box_n[1] * (p.box_n[2] / p.seg_len);   // units
  const int col0 = blockIdx.x * p.cols_per_wg;
  const int n_cols = n_cols_all - col0 < p.cols_per_wg ? n_cols_all - col0 : p.cols_per_wg;
  if (role == 0) wgsym_x_loop<KIND>(p, smem_wgsym, col0, n_cols);
  else if (role == 1) wgsym_y_loop<0>(p, smem_wgsym, col0, n_cols);
  else if (role == 2) wgsym_y_loop<1>(p, smem_wgsym, col0, n_cols);
  else wgsym_y_loop<2>(p, smem_wgsym, col0, n_cols);
}

inline void launch_tensor_wgsym(mimi_hip_domain_s* h, const DomainCall& c, TensorArgs a) {
  h->scratch_k.resize((size_t)h->n_el * P2Block::size);
  h->scratch_r.resize((size_t)h->n_el * 3 * 27);
  a.scratch_k = h->scratch_k.ptr;
  a.scratch_r = h->scratch_r.ptr;
  a.n_units_u = a.box_n[0];
  a.n_units_v = a.box_n[1];
  const size_t lds = WgsymLds::total * sizeof(double);
  // segments per column, units per workgroup, workgroups: wgsym_geometry.hpp
  const WgsymGeometry g = wgsym_geometry(a.box_n, h->wgsym_min_wgs ? h->wgsym_min_wgs : WGSYM_MIN_WGS);
  a.seg_len = h->last_seg_len = g.seg_len;
  a.cols_per_wg = h->last_cols_per_wg = g.cols_per_wg;
  run_two_phase(
      h, c, false, [] {},
      [&] { launch(tensor_wgsym_kernel<MIMI_HIP_MAT_NEOHOOKEAN>, dim3(g.grid), dim3(256), lds, h->stream, a); },
      [&] { launch_tensor_p2(h, a); });
}

}  // namespace mimi_hip
