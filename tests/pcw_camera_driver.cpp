// Host driver of the camera-model projection of xivo_amd/csrc/pcw_device.h (tests/test_pcw_camera_cpu.py, and the reference of
// the pixel bound in tests/test_pcw_camera_gpu.py): compiled with g++ against the header alone, it runs pcw_project over
// (point, pose) pairs read from a binary file.
//   pcw_camera_driver in out   in: n, model, rows, cols (int64), fx, fy, cx, cy, d[5], max_radius (double), X[n][3], g[n][12]
//                              out: vis[n] (uint8), uvz[n][3] (double)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pcw_device.h"

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
  if (argc != 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  const auto h = rd<int64_t>(in, 4);
  const size_t n = (size_t)h[0];
  const auto k = rd<double>(in, 10);
  xivo_cam cam{};
  cam.model = (int)h[1]; cam.rows = (int)h[2]; cam.cols = (int)h[3];
  cam.fx = k[0]; cam.fy = k[1]; cam.cx = k[2]; cam.cy = k[3];
  for (int i = 0; i < 5; ++i) cam.d[i] = k[4 + i];
  const double max_radius = k[9];
  const auto X = rd<double>(in, 3 * n);
  const auto g = rd<double>(in, 12 * n);
  std::vector<uint8_t> vis(n);
  std::vector<double> uvz(3 * n);
  for (size_t i = 0; i < n; ++i) vis[i] = pcw_project(&X[3 * i], &g[12 * i], cam, max_radius, &uvz[3 * i]) ? 1 : 0;
  wr(out, vis); wr(out, uvz);
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
