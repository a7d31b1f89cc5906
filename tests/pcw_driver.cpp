// Host driver of xivo_amd/csrc/pcw_device.h (tests/test_pcw_tracks_cpu.py): compiled with g++ against the header alone, it
// runs the functions the kernel of pcw_kernels.hip calls, serially, over arrays read from a binary file.
//   pcw_driver philox  in out   in: n (int64), n x (ctr[4], key[2]) uint32            out: n x 4 uint32 (pcw_philox4x32_10)
//   pcw_driver words   in out   in: n (int64), n x (seed, frame, b, p) uint64         out: n x 4 uint32 (pcw_noise_words)
//   pcw_driver normals in out   in: seed, frame, nb, np (uint64)                      out: nb x np x 2 doubles (pcw_normal_pair)
//   pcw_driver frames  in out   in: B, npts, T (int64), cam[6], next_id[B] (int64), Xs[B][npts][3], ids[B][npts] (int64),
//                                   gsc[T][B][12]
//                               out: per frame vis[B][npts] (uint8), ids[B][npts], next_id[B] (int64), cnt[B] (int32),
//                                    uvz[B][npts][3] (noise-free), rank_vis[B][npts] (int32, -1: not visible)
// The walk of a world is the kernel's in serial form: ascending points, one running count of visible and of new points.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  if (argc != 4) return 1;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  const char* mode = argv[1];
  if (!strcmp(mode, "philox")) {
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto a = rd<uint32_t>(in, 6 * n);
    std::vector<uint32_t> w(4 * n);
    for (size_t i = 0; i < n; ++i) pcw_philox4x32_10(&a[6 * i], &a[6 * i + 4], &w[4 * i]);
    wr(out, w);
  } else if (!strcmp(mode, "words")) {
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto a = rd<uint64_t>(in, 4 * n);
    std::vector<uint32_t> w(4 * n);
    for (size_t i = 0; i < n; ++i) pcw_noise_words(a[4 * i], a[4 * i + 1], (int)a[4 * i + 2], (int)a[4 * i + 3], &w[4 * i]);
    wr(out, w);
  } else if (!strcmp(mode, "normals")) {
    const auto h = rd<uint64_t>(in, 4);
    const int nb = (int)h[2], np = (int)h[3];
    std::vector<double> v((size_t)nb * np * 2);
    for (int b = 0; b < nb; ++b)
      for (int p = 0; p < np; ++p) pcw_normal_pair(h[0], h[1], b, p, &v[2 * ((size_t)b * np + p)], &v[2 * ((size_t)b * np + p) + 1]);
    wr(out, v);
  } else if (!strcmp(mode, "frames")) {
    const auto h = rd<int64_t>(in, 3);
    const int B = (int)h[0], npts = (int)h[1], T = (int)h[2];
    const auto cam = rd<double>(in, 6);
    const PcwCam k{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]};
    auto next_id = rd<int64_t>(in, B);
    const auto Xs = rd<double>(in, (size_t)B * npts * 3);
    auto ids = rd<int64_t>(in, (size_t)B * npts);
    const auto gsc = rd<double>(in, (size_t)T * B * 12);
    for (int t = 0; t < T; ++t) {
      std::vector<uint8_t> vis((size_t)B * npts);
      std::vector<int32_t> cnt(B), rank((size_t)B * npts, -1);
      std::vector<double> uvz((size_t)B * npts * 3);
      for (int b = 0; b < B; ++b) {
        int n_vis = 0, n_new = 0;
        for (int p = 0; p < npts; ++p) {
          const size_t i = (size_t)b * npts + p;
          const bool v = pcw_project(&Xs[3 * i], &gsc[((size_t)t * B + b) * 12], k, &uvz[3 * i]);
          const bool is_new = pcw_is_new(v, ids[i]);
          ids[i] = pcw_id_after(v, ids[i], next_id[b], n_new);
          vis[i] = v;
          if (v) rank[i] = n_vis++;
          if (is_new) ++n_new;
        }
        next_id[b] += n_new; cnt[b] = n_vis;
      }
      wr(out, vis); wr(out, ids); wr(out, next_id); wr(out, cnt); wr(out, uvz); wr(out, rank);
    }
  } else {
    return 1;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
