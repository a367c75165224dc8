// libear_amd/csrc/host_gather.h on the CPU, the parts behind earhip_render_process_frames: the contiguous-range staging copy
// (stream_copy_bytes against memcpy for every size and misalignment, guard bytes around the destination; range_slice's slices
// tile a range exactly, with inner boundaries on 64-byte multiples, and the sliced copy of a chunked frame buffer equals one
// memcpy), and the shared chunk plan (plan_host_chunks) against the plan earhip_render_process made inline before it was
// shared, restated below, over a sweep of shapes: same short / long decision, same chunk boundaries.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host_gather.h"

using namespace earhip;

// The float path's chunk plan as it stood inline in earhip_render_process (api_render.hip) before plan_host_chunks: the yardstick.
static bool float_path_plan(size_t nblocks, int B, int M, bool in_st, bool has_mb, int mb, int host_first, size_t *cstart, int *nch_out) {
  const size_t n = nblocks * (size_t)B;
  const size_t in_bytes = sizeof(float) * n * M;
  const bool short_call = in_bytes < ((size_t)16 << 20) || M < 16 || (has_mb && mb <= 0);
  if (short_call) return true;
  const size_t block_bytes = sizeof(float) * (size_t)B * M;
  const size_t want_bytes = (size_t)std::max(1, has_mb ? mb : (in_st ? 32 : 16)) << 20;
  size_t cb = std::max<size_t>(1, want_bytes / block_bytes);
  cb = std::max(cb, (nblocks + 64 - 2) / (64 - 1));
  size_t gran = 1;
  while ((gran * (size_t)B) % 4 != 0) gran++;
  cb = (cb + gran - 1) / gran * gran;
  size_t cb0 = in_st || host_first == 0 ? cb : std::max(gran, cb / 4 / gran * gran);
  if (cb0 >= nblocks) cb0 = cb;
  int nch = 0;
  for (size_t b = 0; b < nblocks; b += nch == 1 ? cb0 : cb) cstart[nch++] = b * B;
  cstart[nch] = n;
  *nch_out = nch;
  return false;
}

int main() {
  int bad = 0;
  std::mt19937 rng(5);
  // --- stream_copy_bytes == memcpy
  std::vector<unsigned char> src(20000), dst(20000), ref(20000);
  for (auto &v : src) v = (unsigned char)rng();
  long copies = 0;
  for (int rep = 0; rep < 4000; rep++) {
    const size_t n = rep < 300 ? (size_t)rep : rng() % 9000;
    const size_t so = rng() % 67, d_o = 16 + rng() % 67;
    std::fill(dst.begin(), dst.end(), 0xa5);
    std::fill(ref.begin(), ref.end(), 0xa5);
    stream_copy_bytes(dst.data() + d_o, src.data() + so, n);
#if defined(__x86_64__)
    _mm_sfence();
#endif
    std::memcpy(ref.data() + d_o, src.data() + so, n);
    if (dst != ref) {
      if (bad < 5) printf("stream_copy_bytes differs: n=%zu src+%zu dst+%zu\n", n, so, d_o);
      bad++;
    }
    copies++;
  }
  // --- range_slice: exact tiling, 64-byte inner boundaries
  long slices = 0;
  for (size_t bytes : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000, (size_t)4097, (size_t)1 << 20, (size_t)12345679})
    for (int nt = 1; nt <= 17; nt++) {
      size_t at = 0;
      for (int t = 0; t < nt; t++) {
        size_t lo, hi;
        range_slice(bytes, t, nt, &lo, &hi);
        if (lo != at || hi < lo || (t + 1 < nt && hi % 64 != 0 && hi != bytes)) {
          if (bad < 10) printf("range_slice(%zu, %d, %d) = [%zu, %zu) after %zu\n", bytes, t, nt, lo, hi, at);
          bad++;
        }
        at = hi;
        slices++;
      }
      if (at != bytes) printf("range_slice(%zu, *, %d) ends at %zu\n", bytes, nt, at), bad++;
    }
  // --- the staging threads' contiguous job, as GatherPool runs it: chunk g's byte range, sliced among nt threads, each slice
  // streamed to the same offset of the staging buffer == one memcpy of the whole call's frames
  for (int rep = 0; rep < 60; rep++) {
    const size_t unit = 1 + rng() % 200;  // frame bytes (s24 frames of an odd channel count included)
    const int nch = 1 + (int)(rng() % 9), nt = 1 + (int)(rng() % 9);
    std::vector<size_t> cs(nch + 1, 0);
    for (int g = 1; g <= nch; g++) cs[g] = cs[g - 1] + rng() % 300;
    const size_t total = cs[nch] * unit;
    std::vector<unsigned char> s(total + 7), d(total + 64, 0x5a), want(total + 64, 0x5a);
    for (auto &v : s) v = (unsigned char)rng();
    const size_t so = rng() % 7;
    for (int t = 0; t < nt; t++)
      for (int g = 0; g < nch; g++) {
        size_t lo, hi;
        range_slice((cs[g + 1] - cs[g]) * unit, t, nt, &lo, &hi);
        const size_t o = cs[g] * unit + lo;
        if (hi > lo) stream_copy_bytes(d.data() + o, s.data() + so + o, hi - lo);
      }
#if defined(__x86_64__)
    _mm_sfence();
#endif
    std::memcpy(want.data(), s.data() + so, total);
    if (d != want) {
      if (bad < 15) printf("sliced chunk copy differs: unit %zu, %d chunks, %d threads\n", unit, nch, nt);
      bad++;
    }
  }
  // --- the shared chunk plan == the float path's own
  long plans = 0, longs = 0, multi = 0;
  const int Bs[] = {16, 17, 64, 100, 480, 512, 1000, 1024, 2048, 4096};
  const int Ms[] = {1, 15, 16, 17, 64, 250, 1024, 1027, 4096};
  for (int B : Bs)
    for (int M : Ms)
      for (size_t nblocks : {(size_t)1, (size_t)2, (size_t)7, (size_t)31, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)1000, (size_t)4096})
        for (int direct = 0; direct < 2; direct++)
          for (int opt = 0; opt < 5; opt++) {
            if ((int64_t)nblocks * B >= ((int64_t)1 << 30)) continue;
            const bool has_mb = opt == 1 || opt == 2 || opt == 4;
            const int mb = opt == 1 ? 4 : opt == 2 ? 0 : opt == 4 ? 64 : 0;
            const int first = opt == 3 ? 1 : 0;
            size_t want[66];
            int wn = 0;
            const bool wshort = float_path_plan(nblocks, B, M, direct != 0, has_mb, mb, first, want, &wn);
            const HostChunkPlan p = plan_host_chunks(nblocks, B, M, direct != 0, has_mb, mb, first);
            bool same = p.short_call == wshort;
            if (same && !wshort) {
              same = p.nch == wn;
              for (int c = 0; same && c <= wn; c++) same = p.cstart[c] == want[c];
              longs++;
              multi += wn >= 3;
            }
            if (!same) {
              if (bad < 25) printf("plan differs: B %d M %d nblocks %zu direct %d opt %d\n", B, M, nblocks, direct, opt);
              bad++;
            }
            plans++;
          }
  printf("%ld byte copies, %ld slices, %ld plans (%ld long, %ld of 3+ chunks) checked: %d problem(s)\n", copies, slices, plans, longs,
         multi, bad);
  return bad ? 1 : 0;
}
