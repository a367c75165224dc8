// extent_host.cpp — libear_amd/csrc/extent.h compiled for the host alone (g++, no HIP, under ASan and UBSan): is the
// classification of the chunks that k_pan_objects_extent relies on EXACT?  For every position of the input file the program
// prepares the renderings as k_pan_objects does (extent_passes, extent_setup with at least half the fade in each dimension,
// the float direction: extent_job_fill of panner_kernels.h), takes the angle of every chunk of the grid as extent_render does
// (float dot product, clamped, acosf), classifies it with extent_chunk_class, and then weighs ALL of the chunk's points with
// extent_weight: a chunk classed outside must weigh 0.0f at each point, one classed inside 1.0f — exact comparisons.
// tests/test_extent_cases_cpu.py writes the input file:
//   in:  float64 rows[n][6]: azimuth, elevation, distance, width, height, depth
//   out (stdout, one line): positions, renderings, chunks classed outside / inside / edge, violations, and the smallest slack
//        seen in radians: for a point of weight > 0 its distance inside r_out + margin, for a point of weight < 1 its distance
//        outside r_in - margin (angles between the float direction and the float point, in double)
// exit status: 0, 1 with violations (the first ten on stderr), 2 for a bad call.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../libear_amd/csrc/extent.h"

using namespace earhip;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> rows;
  double row[6];
  while (std::fread(row, sizeof(double), 6, f) == 6) rows.insert(rows.end(), row, row + 6);
  std::fclose(f);
  const size_t n = rows.size() / 6;

  const ExtentGrid G = extent_grid();
  if (G.n_chunks > (size_t)kExtentMaxChunks) return 2;
  const size_t np = G.points.size();
  std::vector<float> xs(np), ys(np), zs(np);
  for (size_t q = 0; q < np; q++) xs[q] = (float)G.points[q].x, ys[q] = (float)G.points[q].y, zs[q] = (float)G.points[q].z;

  long renderings = 0, n_out = 0, n_in = 0, n_edge = 0, violations = 0;
  double slack_out = 1e30, slack_in = 1e30;
  for (size_t i = 0; i < n; i++) {
    const double *r = &rows[6 * i];
    const Vec3 p = polar_to_cart(r[0], r[1], r[2]);
    ExtentPasses X;
    extent_passes(p, r[3], r[4], r[5], X);
    const double norm = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
    const float dir[3] = {norm < 1e-10 ? 0.0f : (float)(p.x / norm), norm < 1e-10 ? 1.0f : (float)(p.y / norm),
                          norm < 1e-10 ? 0.0f : (float)(p.z / norm)};
    for (int k = 0; k < X.n_pass; k++) {
      if (!(X.spread[k] > 1e-10)) continue;
      ExtentWeighting W;
      extent_setup(p, std::fmax(X.w[k], kExtentFade / 2.0), std::fmax(X.h[k], kExtentFade / 2.0), W);
      renderings++;
      double far_dot = 2.0, near_dot = -2.0;
      for (size_t c = 0; c < G.n_chunks; c++) {
        const float cd = G.chunk_dir[c] * dir[0] + G.chunk_dir[G.n_chunks + c] * dir[1] + G.chunk_dir[2 * G.n_chunks + c] * dir[2];
        const float chunk_angle = acosf(fminf(fmaxf(cd, -1.0f), 1.0f));
        const ExtentChunkClass cls = extent_chunk_class(W, chunk_angle, G.chunk_rad[c]);
        n_out += cls == kExtentChunkOutside, n_in += cls == kExtentChunkInside, n_edge += cls == kExtentChunkEdge;
        const size_t lo = 64 * c, hi = std::min(lo + 64, np);
        for (size_t q = lo; q < hi; q++) {
          const float w = extent_weight(W, xs[q], ys[q], zs[q]);
          const bool bad = (cls == kExtentChunkOutside && !(w == 0.0f)) || (cls == kExtentChunkInside && !(w == 1.0f));
          if (bad && violations++ < 10)
            std::fprintf(stderr, "row %zu (az %g el %g dist %g width %.17g height %.17g depth %g) rendering %d chunk %zu classed %s: point %zu weighs %.9g\n",
                         i, r[0], r[1], r[2], r[3], r[4], r[5], k, c, cls == kExtentChunkOutside ? "outside" : "inside", q, (double)w);
          const double dot = (double)xs[q] * dir[0] + (double)ys[q] * dir[1] + (double)zs[q] * dir[2];
          if (w > 0.0f) far_dot = std::min(far_dot, dot);
          if (w < 1.0f) near_dot = std::max(near_dot, dot);
        }
      }
      // (the furthest point that weighs something and the nearest that does not weigh 1, per rendering)
      if (far_dot < 2.0)
        slack_out = std::min(slack_out, ((double)W.r_out + kExtentChunkMargin) - std::acos(std::min(1.0, std::max(-1.0, far_dot))));
      if (near_dot > -2.0)
        slack_in = std::min(slack_in, std::acos(std::min(1.0, std::max(-1.0, near_dot))) - ((double)W.r_in - kExtentChunkMargin));
    }
  }
  std::printf("positions %zu renderings %ld outside %ld inside %ld edge %ld violations %ld slack_out %.6e slack_in %.6e\n", n, renderings,
              n_out, n_in, n_edge, violations, slack_out, slack_in);
  return violations ? 1 : 0;
}
