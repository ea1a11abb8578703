// TEST HARNESS ONLY: the least-squares side of the device GMRES (mimi_amd/csrc/gmres_host.hpp) replayed on the host from a
// file of Hessenberg columns (tests/test_gmres_host_cpu.py builds and runs it, with the sanitizers where the box has them).
//   input, one record per line, numbers as C99 hexadecimal floats:
//     kdim K                        first line
//     cycle BETA                    a cycle starts from ||r|| = BETA
//     column I H_0 .. H_I NORM2     column I in the wire format of the device
//     solve K                       the coefficients of the first K basis vectors
//   output: "resid R" per column, "y Y_0 .. Y_{K-1}" per solve
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../mimi_amd/csrc/gmres_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line, word;
  int kdim = 0;
  if (!std::getline(in, line) || std::sscanf(line.c_str(), "kdim %d", &kdim) != 1 || kdim < 1) {
    std::fprintf(stderr, "no kdim line\n");
    return 2;
  }
  mimi_hip::GmresLeastSquares ls(kdim);
  while (std::getline(in, line)) {
    std::istringstream rec(line);
    if (!(rec >> word)) continue;
    std::vector<double> numbers;
    for (std::string t; rec >> t;) numbers.push_back(std::strtod(t.c_str(), nullptr));
    if (word == "cycle" && numbers.size() == 1) {
      ls.start_cycle(numbers[0]);
    } else if (word == "column" && !numbers.empty() && numbers[0] >= 0 && numbers[0] < kdim && numbers.size() == (size_t)numbers[0] + 3) {
      std::printf("resid %a\n", ls.push_column((int)numbers[0], numbers.data() + 1));
    } else if (word == "solve" && numbers.size() == 1 && numbers[0] >= 0 && numbers[0] <= kdim) {
      const int k = (int)numbers[0];
      const double* y = ls.solve(k);
      std::printf("y");
      for (int i = 0; i < k; ++i) std::printf(" %a", y[i]);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "bad record: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
