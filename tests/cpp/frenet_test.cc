// Stand-alone check of the Frenet functions of include/cilqr/trajectory_queries.hpp (project_rows, project_point,
// cartesian_point) on the crafted cases of tests/frenet_cases.py, meant to be built with -fsanitize=address,undefined:
//   frenet_test <cases file>
// The file is what frenet_cases.write_cases produces (little-endian): "FCASES01", i32 n_cases, i32 n_inverses; per case
// i32 layout, i32 n_center, i32 M, center [n][7], rows [M][F], expected [M][8], cross [M]; per inverse i32 n_center, i32 M,
// center, sl [M][2], expected [M][3].  Every array lives in a heap block of exactly its size, so a read or write past
// either end is the sanitizer's to report.  Exit status 0: every element of every result is the expected one bit for bit
// (a NaN matches any NaN; where the expected cross product is a NaN the sign of the lateral offset is not compared).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cilqr/trajectory_queries.hpp"

namespace {

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

bool same(double a, double b) {
  if (std::isnan(a) && std::isnan(b)) return true;
  return std::memcmp(&a, &b, 8) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char magic[8];
  int32_t counts[2] = {0, 0};
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "FCASES01", 8) != 0 || !read_exact(f, counts, 8) || counts[0] < 0 ||
      counts[0] > (1 << 16) || counts[1] < 0 || counts[1] > (1 << 16)) {
    std::fprintf(stderr, "not a cases file\n");
    return 2;
  }
  namespace tq = cilqr::trajectory_queries;
  int failures = 0;
  long rows_out = 0;
  for (int32_t c = 0; c < counts[0]; ++c) {
    int32_t head[3];
    if (!read_exact(f, head, 12)) return 2;
    const int32_t layout = head[0], n = head[1], M = head[2];
    int F = 0, xc = 0;
    if (!tq::point_columns(layout, &F, &xc) || n < 2 || n > (1 << 20) || M < 1 || M > (1 << 20)) return 2;
    std::vector<double> center((size_t)n * 7), rows((size_t)M * F), want((size_t)M * 8), cross((size_t)M), got((size_t)M * 8, -7.0);
    if (!read_exact(f, center.data(), center.size() * 8) || !read_exact(f, rows.data(), rows.size() * 8) ||
        !read_exact(f, want.data(), want.size() * 8) || !read_exact(f, cross.data(), cross.size() * 8))
      return 2;
    tq::project_rows(center.data(), n, layout, rows.data(), M, got.data());
    rows_out += M;
    for (int m = 0; m < M; ++m) {
      double one[8], side = 0.0;   // the single-point form gives the same row and hands the cross product out
      tq::project_point(center.data(), n, rows[(size_t)m * F + xc], rows[(size_t)m * F + xc + 1], one, &side);
      if (!same(side, cross[m])) {
        std::fprintf(stderr, "case %d query %d: cross %.17g, expected %.17g\n", (int)c, m, side, cross[m]);
        ++failures;
      }
      for (int e = 0; e < 8; ++e) {
        double g = got[(size_t)m * 8 + e], w = want[(size_t)m * 8 + e], o = one[e];
        if (e == 1 && std::isnan(cross[m])) g = std::fabs(g), w = std::fabs(w), o = std::fabs(o);
        if (!same(g, w) || !same(o, w)) {
          std::fprintf(stderr, "case %d query %d column %d: %.17g / %.17g, expected %.17g\n", (int)c, m, e, g, o, w);
          ++failures;
        }
      }
    }
  }
  for (int32_t c = 0; c < counts[1]; ++c) {
    int32_t head[2];
    if (!read_exact(f, head, 8)) return 2;
    const int32_t n = head[0], M = head[1];
    if (n < 2 || n > (1 << 20) || M < 1 || M > (1 << 20)) return 2;
    std::vector<double> center((size_t)n * 7), sl((size_t)M * 2), want((size_t)M * 3), got((size_t)M * 3, -7.0);
    if (!read_exact(f, center.data(), center.size() * 8) || !read_exact(f, sl.data(), sl.size() * 8) ||
        !read_exact(f, want.data(), want.size() * 8))
      return 2;
    for (int m = 0; m < M; ++m) tq::cartesian_point(center.data(), n, sl[(size_t)m * 2], sl[(size_t)m * 2 + 1], got.data() + (size_t)m * 3);
    rows_out += M;
    for (size_t e = 0; e < got.size(); ++e) {
      if (!same(got[e], want[e])) {
        std::fprintf(stderr, "inverse %d pair %d column %d: %.17g, expected %.17g\n", (int)c, (int)(e / 3), (int)(e % 3), got[e], want[e]);
        ++failures;
      }
    }
  }
  std::fclose(f);
  std::printf("%d cases, %d inverses, %ld rows, %d failures\n", (int)counts[0], (int)counts[1], rows_out, failures);
  return failures == 0 ? 0 : 1;
}
