// Host driver of the track-fault rules of xivo_amd/csrc/pcw_device.h (tests/test_pcw_faults_cpu.py): compiled with g++ against
// the header alone, it runs the functions the fault instances of pcw_tracks_kernel call, serially, over arrays read from a
// binary file. A program of its own, so that it also runs built with -fsanitize=address,undefined.
//   pcw_fault_driver words  in out   in: n (int64), n x (seed, frame, b, p, draw) uint64, draw 0: A, 1: B
//                                    out: n x 4 uint32 (pcw_fault_words)
//   pcw_fault_driver draws  in out   in: seed, frame, nb, np (uint64), fault[6] = t1, t2, t3, min_px, max_px, tail_scale (double)
//                                    out: event [nb][np] (int32), off [nb][np][2] (double; pcw_fault_offset of every point)
//   pcw_fault_driver cells  in out   in: n (int64), n x (mask, flag) uint8      out: n x int32 (pcw_fault_cell)
//   pcw_fault_driver frames in out   in: B, npts, T, sticky, stream_mod (int64), seed (uint64), noise_px_std, fault[6], cam[6]
//                                        (double), next_id[B] (int64), Xs[B][npts][3], ids[B][npts] (int64), gsc[T][B][12]
//                                    out: per frame vis_eff[B][npts] (uint8), ids[B][npts], next_id[B] (int64), cnt[B] (int32),
//                                         flag[B][npts] (uint8, 0: no track), pix[B][npts][3] (what the track reports; 0: no
//                                         track), bias[B][npts][2], counters[B][5] (int64, summed over the frames so far: tracks,
//                                         dropped, outlier_events, tail_events, biased)
// The walk of a world is the kernel's in serial form: ascending points, one running count of tracks and of new points.
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
  if (!strcmp(mode, "words")) {
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto a = rd<uint64_t>(in, 5 * n);
    std::vector<uint32_t> w(4 * n);
    for (size_t i = 0; i < n; ++i)
      pcw_fault_words(a[5 * i], a[5 * i + 1], (int)a[5 * i + 2], (int)a[5 * i + 3], a[5 * i + 4] ? kPcwDrawB : kPcwDrawA, &w[4 * i]);
    wr(out, w);
  } else if (!strcmp(mode, "draws")) {
    const auto h = rd<uint64_t>(in, 4);
    const auto fd = rd<double>(in, 6);
    const PcwFault f{fd[0], fd[1], fd[2], fd[3], fd[4], fd[5], 0};
    const int nb = (int)h[2], np = (int)h[3];
    std::vector<int32_t> ev((size_t)nb * np);
    std::vector<double> off((size_t)nb * np * 2);
    for (int b = 0; b < nb; ++b)
      for (int p = 0; p < np; ++p) {
        const size_t i = (size_t)b * np + p;
        uint32_t wa[4], wb[4];
        pcw_fault_words(h[0], h[1], b, p, kPcwDrawA, wa);
        pcw_fault_words(h[0], h[1], b, p, kPcwDrawB, wb);
        ev[i] = pcw_fault_event(f, philox_uniform(wa[0], wa[1]));
        pcw_fault_offset(f, wa, wb, &off[2 * i]);
      }
    wr(out, ev); wr(out, off);
  } else if (!strcmp(mode, "cells")) {
    const size_t n = (size_t)rd<int64_t>(in, 1)[0];
    const auto a = rd<uint8_t>(in, 2 * n);
    std::vector<int32_t> c(n);
    for (size_t i = 0; i < n; ++i) c[i] = pcw_fault_cell(a[2 * i], a[2 * i + 1]);
    wr(out, c);
  } else if (!strcmp(mode, "frames")) {
    const auto h = rd<int64_t>(in, 5);
    const int B = (int)h[0], npts = (int)h[1], T = (int)h[2], stream_mod = (int)h[4];
    const uint64_t seed = rd<uint64_t>(in, 1)[0];
    const double noise_px_std = rd<double>(in, 1)[0];
    const auto fd = rd<double>(in, 6);
    const PcwFault f{fd[0], fd[1], fd[2], fd[3], fd[4], fd[5], (int)h[3]};
    const auto cam = rd<double>(in, 6);
    const PcwCam k{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]};
    auto next_id = rd<int64_t>(in, B);
    const auto Xs = rd<double>(in, (size_t)B * npts * 3);
    auto ids = rd<int64_t>(in, (size_t)B * npts);
    const auto gsc = rd<double>(in, (size_t)T * B * 12);
    std::vector<double> bias((size_t)B * npts * 2, 0.0);
    std::vector<int64_t> counters((size_t)B * 5, 0);
    for (int t = 0; t < T; ++t) {
      std::vector<uint8_t> vis((size_t)B * npts), flag((size_t)B * npts, 0);
      std::vector<int32_t> cnt(B);
      std::vector<double> pix((size_t)B * npts * 3, 0.0);
      for (int b = 0; b < B; ++b) {
        const int bw = pcw_stream_filter(b, stream_mod);
        int n_vis = 0, n_new = 0;
        for (int p = 0; p < npts; ++p) {
          const size_t i = (size_t)b * npts + p;
          double uvz[3], off[2], scale;
          unsigned char fl;
          int ev;
          const bool geo = pcw_project(&Xs[3 * i], &gsc[((size_t)t * B + b) * 12], k, uvz);
          const bool v = pcw_fault_point(f, seed, (uint64_t)t, bw, p, geo, &bias[2 * i], off, &scale, &fl, &ev);
          const bool is_new = pcw_is_new(v, ids[i]);
          ids[i] = pcw_id_after(v, ids[i], next_id[b], n_new);
          vis[i] = v;
          if (geo && !v) ++counters[5 * b + 1];
          if (v) {
            double nu = 0.0, nv = 0.0;
            if (noise_px_std != 0.0) pcw_normal_pair(seed, (uint64_t)t, bw, p, &nu, &nv);
            const double std_eff = pcw_fault_std(noise_px_std, scale);
            pix[3 * i] = pcw_fault_pixel(uvz[0], off[0], std_eff, nu);
            pix[3 * i + 1] = pcw_fault_pixel(uvz[1], off[1], std_eff, nv);
            pix[3 * i + 2] = uvz[2];
            flag[i] = fl;
            ++n_vis;
            if (fl & PCW_FLAG_OUTLIER) ++counters[5 * b + 2];
            if (fl & PCW_FLAG_TAIL) ++counters[5 * b + 3];
            if (fl & PCW_FLAG_BIASED) ++counters[5 * b + 4];
          }
          if (is_new) ++n_new;
        }
        next_id[b] += n_new; cnt[b] = n_vis; counters[5 * b] += n_vis;
      }
      wr(out, vis); wr(out, ids); wr(out, next_id); wr(out, cnt); wr(out, flag); wr(out, pix); wr(out, bias); wr(out, counters);
    }
  } else {
    return 1;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
