// Stand-alone driver of xivo_amd/csrc/innov_device.h (tests/test_innov_log_cpu.py): evaluates one filter's innovation record
// on the host exactly as innov_record_kernel maps it onto a workgroup - the 64 lanes of a wave and the 256 threads as arrays,
// the butterfly and the tree of the header - and prints it as hex floats. Compiled from the header alone, no HIP.
//
// stdin, whitespace separated (doubles as C hex floats / nan / inf), any number of cases until end of input:
//   M N er lead_k status ldlt          rows [0, er) compressed (er even or er == M), rows [er, M) dense
//   idx  [(er + 1) / 2][28]            ints
//   val  [(er + 1) / 2][28][2]
//   lead [2 * ((er + 1) / 2)][lead_k]  row-major, only when lead_k > 0
//   H    [M - er][N]                   the dense rows, row-major
//   inn [M]   R [M]   dx [N]
// stdout: one "layout" line (sizeof / offsetof of xivo_innov_rec), then per case
//   rec nis prefit postfit inn_max dx_max dof rows flags
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../xivo_amd/csrc/innov_device.h"

using namespace xivo_hip;

static bool read_int(int& v) { return scanf("%d", &v) == 1; }
static double read_double() {
  char buf[128];
  if (scanf("%127s", buf) != 1) { fprintf(stderr, "innov_row_driver: truncated input\n"); exit(2); }
  return strtod(buf, nullptr);
}

int main() {
  printf("layout sizeof=%zu nis=%zu prefit=%zu postfit=%zu inn_max=%zu dx_max=%zu dof=%zu rows=%zu flags=%zu reserved=%zu reserved2=%zu\n",
         sizeof(xivo_innov_rec), offsetof(xivo_innov_rec, nis), offsetof(xivo_innov_rec, prefit), offsetof(xivo_innov_rec, postfit),
         offsetof(xivo_innov_rec, inn_max), offsetof(xivo_innov_rec, dx_max), offsetof(xivo_innov_rec, dof),
         offsetof(xivo_innov_rec, rows), offsetof(xivo_innov_rec, flags), offsetof(xivo_innov_rec, reserved),
         offsetof(xivo_innov_rec, reserved2));
  int M;
  while (read_int(M)) {
    int N, er, lead_k, status, ldlt;
    if (!read_int(N) || !read_int(er) || !read_int(lead_k) || !read_int(status) || !read_int(ldlt)) return 2;
    if (M <= 0 || N <= 0 || er < 0 || er > M || (er != M && (er & 1)) || lead_k < 0 || lead_k > kInnovWave || lead_k > N) return 2;
    const int pairs = (er + 1) / 2, W = 28, Me = (M + 1) & ~1;
    std::vector<int> idx((size_t)pairs * W);
    std::vector<double> val((size_t)pairs * W * 2), lead((size_t)2 * pairs * lead_k), H((size_t)(M - er) * N), inn(M), R(M), dx(N);
    for (int& v : idx) { if (!read_int(v) || v < 0 || v >= N) return 2; }
    for (double& v : val) v = read_double();
    for (double& v : lead) v = read_double();
    for (double& v : H) v = read_double();
    for (double& v : inn) v = read_double();
    for (double& v : R) v = read_double();
    for (double& v : dx) v = read_double();

    std::vector<InnovAcc> part(kInnovThreads, innov_zero());
    for (int t = 0; t < kInnovThreads; ++t)
      for (int k = t; k < N; k += kInnovThreads) innov_add_dx(part[t], dx[k]);
    std::vector<double> hdx(Me, 0.0);
    std::vector<int> nz(Me, 0);
    for (int p = 0; p < pairs; ++p) {               // a wave per pair, a lane per slot / lead column
      double h0[kInnovWave], h1[kInnovWave];
      int z = 0;
      for (int lane = 0; lane < kInnovWave; ++lane) {
        h0[lane] = 0.0; h1[lane] = 0.0;
        if (lane < W) {
          const size_t s = (size_t)p * W + lane;
          const double d = dx[idx[s]];
          h0[lane] = innov_term(val[2 * s], d); h1[lane] = innov_term(val[2 * s + 1], d);
          z |= (val[2 * s] != 0.0 ? 1 : 0) | (val[2 * s + 1] != 0.0 ? 2 : 0);
        }
        if (lane < lead_k) {
          const double l0 = lead[(size_t)(2 * p) * lead_k + lane], l1 = lead[(size_t)(2 * p + 1) * lead_k + lane];
          h0[lane] = innov_term_add(h0[lane], l0, dx[lane]); h1[lane] = innov_term_add(h1[lane], l1, dx[lane]);
          z |= (l0 != 0.0 ? 1 : 0) | (l1 != 0.0 ? 2 : 0);
        }
      }
      hdx[2 * p] = innov_wave_sum(h0); hdx[2 * p + 1] = innov_wave_sum(h1);
      nz[2 * p] = z & 1; nz[2 * p + 1] = (z >> 1) & 1;
    }
    for (int i = er; i < M; ++i) {                  // a thread per dense row
      double h = 0.0;
      int z = 0;
      for (int n = 0; n < N; ++n) {
        const double v = H[(size_t)(i - er) * N + n];
        h = innov_term_add(h, v, dx[n]);
        z |= v != 0.0 ? 1 : 0;
      }
      hdx[i] = h; nz[i] = z;
    }
    for (int t = 0; t < kInnovThreads; ++t)
      for (int i = t; i < M; i += kInnovThreads) innov_add_row(part[t], inn[i], R[i], hdx[i], nz[i] != 0);
    const xivo_innov_rec r = innov_finish(innov_tree(part.data()), M, status, ldlt);
    printf("rec %a %a %a %a %a %d %d %d\n", r.nis, r.prefit, r.postfit, r.inn_max, r.dx_max, r.dof, r.rows, r.flags);
  }
  return 0;
}
