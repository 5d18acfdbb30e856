// Stand-alone check of include/cilqr/trajectory_queries.hpp on the crafted cases of tests/resample_cases.py, meant to be
// built with -fsanitize=address,undefined:
//   trajectory_queries_test <cases file>
// The file is what resample_cases.write_cases produces (little-endian): "RCASES01", i32 n; per case i32 layout, i32 key,
// i32 K, i32 M, rows [K][F], queries [M], expected [M][F].  Rows, queries and results live in heap blocks of exactly their
// size, so a read or write past either end is the sanitizer's to report.  Exit status 0: every element of every result is
// the expected one bit for bit (a NaN matches any NaN).
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
  int32_t n_cases = 0;
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "RCASES01", 8) != 0 || !read_exact(f, &n_cases, 4) || n_cases < 0 ||
      n_cases > (1 << 16)) {
    std::fprintf(stderr, "not a cases file\n");
    return 2;
  }
  namespace tq = cilqr::trajectory_queries;
  int failures = 0;
  long rows_out = 0;
  for (int32_t c = 0; c < n_cases; ++c) {
    int32_t head[4];
    if (!read_exact(f, head, 16)) return 2;
    const int32_t layout = head[0], key = head[1], K = head[2], M = head[3];
    const int F = tq::columns_of(layout).fields;
    if (F == 0 || tq::key_column(layout, key) < 0 || K < 2 || K > (1 << 20) || M < 1 || M > (1 << 20)) return 2;
    std::vector<double> rows((size_t)K * F), queries((size_t)M), want((size_t)M * F), got((size_t)M * F, -7.0);
    if (!read_exact(f, rows.data(), rows.size() * 8) || !read_exact(f, queries.data(), queries.size() * 8) ||
        !read_exact(f, want.data(), want.size() * 8))
      return 2;
    tq::resample_rows(layout, rows.data(), K, key, queries.data(), M, got.data());
    rows_out += M;
    for (size_t e = 0; e < got.size(); ++e) {
      if (!same(got[e], want[e])) {
        std::fprintf(stderr, "case %d query %d column %d: %.17g, expected %.17g\n", (int)c, (int)(e / F), (int)(e % F), got[e],
                     want[e]);
        ++failures;
      }
    }
  }
  std::fclose(f);
  std::printf("%d cases, %ld rows, %d failures\n", (int)n_cases, rows_out, failures);
  return failures == 0 ? 0 : 1;
}
