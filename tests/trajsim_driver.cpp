// Host driver of xivo_amd/csrc/trajsim_device.h (tests/test_trajsim_cpu.py): compiled with g++ against the header alone, it runs
// the functions the kernel of trajsim_kernels.hip calls, serially, over arrays read from a binary file.
//   trajsim_driver times   in out   in: imu_dt (double), n (int64), k[n] (uint64)    out: t[n], dt[n] doubles (dt of k = 0: 0)
//   trajsim_driver words   in out   in: n (int64), n x (seed, k, b, j) uint64        out: n x 4 uint32, then n x 2 uniforms
//   trajsim_driver normals in out   in: seed, k0, nb, nk, want_a, want_g (uint64)    out: nb x nk x 6 doubles (trajsim_normals)
//   trajsim_driver frame   in out   in: model (22 doubles: imu_dt, rot_amp, rot_w[3], noise_accel, noise_gyro, grav_s[3],
//                                       Rbc[9], Tbc[3]), seed, k0 (uint64), B, n (int64), motion[B] (int32), rate[B]
//                                   out: recs[B][n] (13 doubles each), gt[B][12], gsc[B][12] - what one kernel launch writes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trajsim_device.h"

using namespace xivo_hip;

template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}
template <class T> static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 4) return 1;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  const char* mode = argv[1];
  if (!strcmp(mode, "times")) {
    const double imu_dt = rd<double>(in, 1)[0];
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto k = rd<uint64_t>(in, n);
    std::vector<double> t(n), dt(n, 0.0);
    for (size_t i = 0; i < n; ++i) { t[i] = trajsim_time(k[i], imu_dt); if (k[i] > 0) dt[i] = trajsim_dt(k[i], imu_dt); }
    wr(out, t); wr(out, dt);
  } else if (!strcmp(mode, "words")) {
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto a = rd<uint64_t>(in, 4 * n);
    std::vector<uint32_t> w(4 * n);
    std::vector<double> u(2 * n);
    for (size_t i = 0; i < n; ++i) {
      trajsim_noise_words(a[4 * i], a[4 * i + 1], (int)a[4 * i + 2], (int)a[4 * i + 3], &w[4 * i]);
      u[2 * i] = philox_uniform(w[4 * i], w[4 * i + 1]); u[2 * i + 1] = philox_uniform(w[4 * i + 2], w[4 * i + 3]);
    }
    wr(out, w); wr(out, u);
  } else if (!strcmp(mode, "normals")) {
    const auto h = rd<uint64_t>(in, 6);
    const int nb = (int)h[2], nk = (int)h[3];
    std::vector<double> v((size_t)nb * nk * 6);
    for (int b = 0; b < nb; ++b)
      for (int k = 0; k < nk; ++k) trajsim_normals(h[0], h[1] + (uint64_t)k, b, h[4] != 0, h[5] != 0, &v[6 * ((size_t)b * nk + k)]);
    wr(out, v);
  } else if (!strcmp(mode, "frame")) {
    const auto d = rd<double>(in, 22);
    const auto u = rd<uint64_t>(in, 2);
    const auto h = rd<int64_t>(in, 2);
    const int B = (int)h[0], n = (int)h[1];
    const auto motion = rd<int32_t>(in, B);
    const auto rate = rd<double>(in, B);
    TrajsimModel m{};
    m.imu_dt = d[0]; m.rot_amp = d[1]; m.noise_accel = d[5]; m.noise_gyro = d[6]; m.seed = u[0];
    for (int i = 0; i < 3; ++i) { m.rot_w[i] = d[2 + i]; m.grav_s[i] = d[7 + i]; m.Tbc[i] = d[19 + i]; }
    for (int i = 0; i < 9; ++i) m.Rbc[i] = d[10 + i];
    static_assert(sizeof(TrajsimRecord) == 13 * sizeof(double), "13 doubles");
    std::vector<TrajsimRecord> recs((size_t)B * n);
    std::vector<double> gt((size_t)B * 12), gsc((size_t)B * 12);
    for (int b = 0; b < B; ++b) {
      for (int j = 0; j < n; ++j) trajsim_record(m, motion[b], rate[b], b, u[1] + 1 + (uint64_t)j, &recs[(size_t)b * n + j]);
      trajsim_truth(m, motion[b], rate[b], u[1] + (uint64_t)n, &gt[(size_t)b * 12], &gsc[(size_t)b * 12]);
    }
    wr(out, recs); wr(out, gt); wr(out, gsc);
  } else {
    return 1;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
