// TEST HARNESS ONLY: the node side of mimi_amd/csrc/patch_index.hpp -- NodeWindow<P>, what a wave of the row gathers computes
// for its node -- and the forward stages of mimi_amd/csrc/sum_factor.hpp compiled for the HOST, so that every node of a node
// window can be checked against a brute-force enumeration, and every point's parametric gradient and value against a dense
// contraction, without a GPU (tests/test_patch_index_cpu.py).  Nothing in mimi_amd builds or loads this.
#define MH_DEV __host__ __device__ inline
#include "../mimi_amd/csrc/common.hpp"
#include "../mimi_amd/csrc/patch_index.hpp"
#include "../mimi_amd/csrc/sum_factor.hpp"

namespace mimi_hip {
void set_last_error(const std::string&) {}
}
using namespace mimi_hip;

// head[node][18]: A0 A1 A2, A, empty, ex_lo ex_hi ey_lo ey_hi ez_lo ez_hi, lo0 lo1 lo2, w0 w1 w2, L
// slots[node][(P + 1)^3][3]: element index in the box, the node's local index in it, tbase -- slot (dz, dy, dx) counted from
// (ez_lo, ey_lo, ex_lo) as the lanes of node_residual_rows are; -1 where the box has no such element
template<int P>
static void fill(const TensorArgs& p, int64_t n_nodes, int64_t* head, int64_t* slots) {
  constexpr int NB = P + 1, NS = NB * NB * NB;
  for (int64_t Al = 0; Al < n_nodes; ++Al) {
    const NodeWindow<P> nw(p, Al);
    const int64_t h[18] = {nw.A0, nw.A1, nw.A2, nw.A, nw.empty() ? 1 : 0, nw.ex_lo, nw.ex_hi, nw.ey_lo, nw.ey_hi, nw.ez_lo, nw.ez_hi,
                           nw.lo0, nw.lo1, nw.lo2, nw.w0, nw.w1, nw.w2, nw.L};
    for (int k = 0; k < 18; ++k) head[Al * 18 + k] = h[k];
    for (int s = 0; s < NS; ++s) {
      const int ez = nw.ez_lo + s / (NB * NB), ey = nw.ey_lo + (s / NB) % NB, ex = nw.ex_lo + s % NB;
      const bool in = !nw.empty() && nw.holds(ex, ey, ez);
      int64_t* out = slots + (Al * NS + s) * 3;
      out[0] = in ? nw.elem(ex, ey, ez) : -1;
      out[1] = in ? nw.local(ex, ey, ez) : -1;
      out[2] = in ? nw.tbase(ex, ey, ez) : -1;
    }
  }
}

extern "C" int host_node_windows(int P, const int* box_begin, const int* box_n, const int* n_ctrl, const int* win_begin,
                                 const int* win_n, int64_t* head, int64_t* slots) {
  TensorArgs p{};
  for (int d = 0; d < 3; ++d) {
    p.box_begin[d] = box_begin[d];
    p.box_n[d] = box_n[d];
    p.n_ctrl[d] = n_ctrl[d];
    p.win_begin[d] = win_begin[d];
    p.win_n[d] = win_n[d];
  }
  const int64_t n_nodes = (int64_t)win_n[0] * win_n[1] * win_n[2];
  if (P == 1) fill<1>(p, n_nodes, head, slots);
  else if (P == 2) fill<2>(p, n_nodes, head, slots);
  else if (P == 3) fill<3>(p, n_nodes, head, slots);
  else return 1;
  return 0;
}

// The forward helpers as one thread runs them: NT = 1, tid = 0, an empty barrier; two component sets (NC = 2 DIM).
// tab_out[3][2][NB][NQ] (the loaded block), H[set][point][DIM DIM], val[point][DIM] (set 0)
template<int DIM, int P>
static void forward(const TensorArgs& p, const int (&el)[3], const double* ve, double* tab, double* H, double* val) {
  using S = ElementShape<DIM, P>;
  constexpr int NC = 2 * DIM, NQ01 = S::NQ * S::NQ;
  std::vector<double> X((size_t)NC * 2 * S::NB * S::NBZ * S::NQ), Y((size_t)NC * 3 * S::NBZ * NQ01);
  load_element_tables<DIM, P, 1>(p, el, 0, tab);
  forward_stages<DIM, P, NC, 1>(tab, ve, X.data(), Y.data(), 0, [] {});
  for (int q = 0; q < S::NPT; ++q) {
    for (int set = 0; set < 2; ++set) parametric_gradient<DIM, P>(tab, Y.data(), set, q % NQ01, q / NQ01, H + ((size_t)set * S::NPT + q) * S::DD);
    point_value<DIM, P>(tab, Y.data(), q % NQ01, q / NQ01, val + (size_t)q * DIM);
  }
}

// tables[dir < dim][B, D][n_spans][P + 1][P + 2]; the element is span box_begin[dir] + el[dir] of each direction
extern "C" int host_forward_stages(int dim, int P, int n_spans, const int* box_begin, const int* el_in, const double* tables,
                                   const double* ve, double* tab, double* H, double* val) {
  TensorArgs p{};
  const int TS = (P + 1) * (P + 2);
  int el[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) {
    p.box_begin[d] = box_begin[d];
    el[d] = el_in[d];
    p.tabB[d] = tables + (size_t)(d * 2 + 0) * n_spans * TS;
    p.tabD[d] = tables + (size_t)(d * 2 + 1) * n_spans * TS;
  }
  const int key = dim * 10 + P;
  if (key == 21) forward<2, 1>(p, el, ve, tab, H, val);
  else if (key == 22) forward<2, 2>(p, el, ve, tab, H, val);
  else if (key == 23) forward<2, 3>(p, el, ve, tab, H, val);
  else if (key == 31) forward<3, 1>(p, el, ve, tab, H, val);
  else if (key == 32) forward<3, 2>(p, el, ve, tab, H, val);
  else if (key == 33) forward<3, 3>(p, el, ve, tab, H, val);
  else return 1;
  return 0;
}
