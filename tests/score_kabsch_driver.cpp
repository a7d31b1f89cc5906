// Drives score_kabsch (xivo_amd/csrc/score_device.h), the closed-form alignment of the trajectory score, under a host compiler:
// the header alone, no HIP. tests/test_score_kabsch_cpu.py passes one 3 x 3 matrix H per call, row-major, as nine numbers that
// strtod reads (hex floats, "nan", "inf"), and reads back one line: R row-major (9), sv (3), the flag - each bit-exact ("%a").
#include <cstdio>
#include <cstdlib>

#include "score_device.h"

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s h00 h01 h02 h10 h11 h12 h20 h21 h22\n", argv[0]);
    return 2;
  }
  double h[3][3], R[3][3], sv[3];
  for (int i = 0; i < 9; ++i) {
    char* end = nullptr;
    h[i / 3][i % 3] = std::strtod(argv[1 + i], &end);
    if (end == argv[1 + i] || *end) {
      std::fprintf(stderr, "not a number: %s\n", argv[1 + i]);
      return 2;
    }
  }
  const int flag = xivo_hip::score_kabsch(h, R, sv);
  for (int i = 0; i < 9; ++i) std::printf("%a ", R[i / 3][i % 3]);
  for (int i = 0; i < 3; ++i) std::printf("%a ", sv[i]);
  std::printf("%d\n", flag);
  return 0;
}
