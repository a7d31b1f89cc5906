// Host driver of the camera models of xivo_amd/csrc/camera_device.h (tests/test_geometry_edges_cpu.py, and the fp64
// reference of the bounds in tests/test_geometry_edges_gpu.py): compiled with g++ against the header alone, it runs
// camera_project_jacc over normalised points and camera_unproject over pixels read from a binary file.
//   camera_edge_driver in out   in: n_proj, n_unproj, model (int64), fx, fy, cx, cy, d[5] (double), xy[n_proj][2], uv[n_unproj][2]
//                               out: per point xp[2], J[2][2], jacc[2][9], dim (25 doubles); per pixel xc[2]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "camera_device.h"

using namespace xivo_hip;

template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  const auto h = rd<int64_t>(in, 3);
  const size_t np = (size_t)h[0], nu = (size_t)h[1];
  const auto k = rd<double>(in, 9);
  xivo_cam cam{};
  cam.model = (int)h[2]; cam.rows = 480; cam.cols = 640;
  cam.fx = k[0]; cam.fy = k[1]; cam.cx = k[2]; cam.cy = k[3];
  for (int i = 0; i < 5; ++i) cam.d[i] = k[4 + i];
  const auto xy = rd<double>(in, 2 * np);
  const auto uv = rd<double>(in, 2 * nu);
  std::vector<double> o(25 * np + 2 * nu);
  for (size_t i = 0; i < np; ++i) {
    double xp[2], J[2][2], jacc[2][9];
    const int dim = camera_project_jacc(cam, xy[2 * i], xy[2 * i + 1], xp, J, jacc);
    double* p = &o[25 * i];
    p[0] = xp[0]; p[1] = xp[1];
    p[2] = J[0][0]; p[3] = J[0][1]; p[4] = J[1][0]; p[5] = J[1][1];
    for (int r = 0; r < 2; ++r) for (int c = 0; c < 9; ++c) p[6 + 9 * r + c] = jacc[r][c];
    p[24] = dim;
  }
  for (size_t i = 0; i < nu; ++i) camera_unproject(cam, uv[2 * i], uv[2 * i + 1], &o[25 * np + 2 * i]);
  if (!o.empty() && fwrite(o.data(), sizeof(double), o.size(), out) != o.size()) return 2;
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
