// TEST HARNESS ONLY: the normal helpers of mimi_amd/csrc/face_wave.hpp -- face_normal_len, face_normal_rate and
// face_normal_column -- compiled for the HOST with -ffp-contract=off, as a stand-alone program (tests/test_face_wave_host_cpu.py).
// It touches no GPU.  usage: host_face_wave_main SEED N_DOF
//   t DIM k hex                 the seeded tangents t[(DIM-1) DIM]
//   dN DIM k hex                the seeded derivatives dN[(DIM-1) n_dof]
//   len DIM hex m_0 .. m_DIM-1  face_normal_len and its m
//   col DIM b j i hex hex       dm_i of face_normal_column(b, j), and of face_normal_rate with dt_k = dN[k n_dof + b] e_j
// Nothing in mimi_amd builds or loads this.
#define MH_DEV __host__ __device__ inline
#include "../mimi_amd/csrc/face_wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mimi_hip;

constexpr int kMaxNodes = 16;   // kFaceMaxDof of face_common.hpp

static unsigned long long state;
static double next_unit() {   // in (-1, 1), never 0: a 64-bit LCG, the top 52 bits
  state = state * 6364136223846793005ULL + 1442695040888963407ULL;
  const double u = (double)((state >> 12) | 1ULL) / 4503599627370496.0;
  return 2.0 * u - 1.0;
}

static void put(double v) {
  unsigned long long bits;
  std::memcpy(&bits, &v, sizeof bits);
  std::printf(" %016llx", bits);
}

template<int DIM>
static void run(int n_dof) {
  constexpr int NT = (DIM - 1) * DIM;
  double t[NT], dN[2 * kMaxNodes];
  for (int k = 0; k < NT; ++k) t[k] = next_unit();
  for (int k = 0; k < (DIM - 1) * n_dof; ++k) dN[k] = next_unit();
  for (int k = 0; k < NT; ++k) {
    std::printf("t %d %d", DIM, k);
    put(t[k]);
    std::printf("\n");
  }
  for (int k = 0; k < (DIM - 1) * n_dof; ++k) {
    std::printf("dN %d %d", DIM, k);
    put(dN[k]);
    std::printf("\n");
  }
  double m[DIM];
  const double len = face_normal_len<DIM>(t, m);
  std::printf("len %d", DIM);
  put(len);
  for (int i = 0; i < DIM; ++i) put(m[i]);
  std::printf("\n");
  for (int b = 0; b < n_dof; ++b)
    for (int j = 0; j < DIM; ++j) {
      double col[DIM], rate[DIM], dt[NT], mm[DIM];
      face_normal_column<DIM>(t, dN, n_dof, b, j, col);
      for (int k = 0; k < NT; ++k) dt[k] = 0.0;
      for (int k = 0; k < DIM - 1; ++k) dt[k * DIM + j] = dN[k * n_dof + b];
      face_normal_rate<DIM>(t, dt, mm, rate);
      for (int i = 0; i < DIM; ++i) {
        std::printf("col %d %d %d %d", DIM, b, j, i);
        put(col[i]);
        put(rate[i]);
        std::printf("\n");
      }
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  state = std::strtoull(argv[1], nullptr, 10);
  const int n_dof = std::atoi(argv[2]);
  if (n_dof < 1 || n_dof > kMaxNodes) return 2;
  run<2>(n_dof);
  run<3>(n_dof);
  return 0;
}
