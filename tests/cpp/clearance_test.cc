// Stand-alone check of DpEnvironment::Clearance (include/cilqr/dp_planner.hpp) on the crafted table of
// tests/clearance_cases.py, meant to be built with -fsanitize=address,undefined:
//   clearance_test <cases file>
// The file is what clearance_cases.write_cases produces (little-endian): "CLCASE01", i32 n; per case i32 n_center,
// center [n][7], f64 front_hang wheel_base rear_hang width, i32 n_static x (i32 m, [m][2]), i32 n_dynamic x (i32 m, [m][2],
// i32 T, [T][4]), i32 K, rows [K][4] = time x y theta, clearance [K][4] f64, nearest [K][4] i32 counted over the obstacles
// the environment keeps.  Exit status 0: every value of every knot has the expected bits and the expected obstacle.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cilqr/dp_planner.hpp"

namespace {

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

bool read_count(std::FILE* f, int32_t* n, int32_t limit) { return read_exact(f, n, 4) && *n >= 0 && *n <= limit; }

bool read_points(std::FILE* f, int32_t n, std::vector<cilqr::DpPoint2>* out) {
  std::vector<double> raw((size_t)n * 2);
  if (!read_exact(f, raw.data(), raw.size() * 8)) return false;
  out->clear();
  for (int32_t i = 0; i < n; ++i) out->push_back(cilqr::DpPoint2{raw[2 * i], raw[2 * i + 1]});
  return true;
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
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "CLCASE01", 8) != 0 || !read_count(f, &n_cases, 1 << 16)) {
    std::fprintf(stderr, "not a cases file\n");
    return 2;
  }
  int failures = 0, knots = 0;
  for (int32_t c = 0; c < n_cases; ++c) {
    int32_t n_center = 0, n_static = 0, n_dynamic = 0, K = 0;
    double vehicle[4];
    if (!read_count(f, &n_center, 1 << 20) || n_center < 2) return 2;
    std::vector<std::array<double, 7>> center(n_center);
    if (!read_exact(f, center.data(), (size_t)n_center * 7 * 8) || !read_exact(f, vehicle, sizeof(vehicle))) return 2;
    cilqr::DpConfig cfg;
    cfg.front_hang_length = vehicle[0]; cfg.wheel_base = vehicle[1]; cfg.rear_hang_length = vehicle[2]; cfg.width = vehicle[3];
    const cilqr::ReferenceLine ref(center);
    cilqr::DpEnvironment env(cfg, ref);
    if (!read_count(f, &n_static, 1 << 16)) return 2;
    for (int32_t o = 0; o < n_static; ++o) {
      int32_t m = 0;
      std::vector<cilqr::DpPoint2> poly;
      if (!read_count(f, &m, 1 << 16) || !read_points(f, m, &poly)) return 2;
      if (m > 0) env.AddStatic(poly);   // no vertices: the slot is unused
    }
    if (!read_count(f, &n_dynamic, 1 << 16)) return 2;
    for (int32_t o = 0; o < n_dynamic; ++o) {
      int32_t m = 0, T = 0;
      std::vector<cilqr::DpPoint2> poly;
      if (!read_count(f, &m, 1 << 16) || !read_points(f, m, &poly) || !read_count(f, &T, 1 << 20)) return 2;
      std::vector<std::array<double, 4>> traj(T);
      if (!read_exact(f, traj.data(), (size_t)T * 4 * 8)) return 2;
      if (m > 0) env.AddDynamic(poly, traj);
    }
    if (!read_count(f, &K, 1 << 20)) return 2;
    std::vector<std::array<double, 4>> rows(K), clearance(K);
    std::vector<std::array<int32_t, 4>> nearest(K);
    if (!read_exact(f, rows.data(), (size_t)K * 4 * 8) || !read_exact(f, clearance.data(), (size_t)K * 4 * 8) ||
        !read_exact(f, nearest.data(), (size_t)K * 4 * 4))
      return 2;
    for (int32_t k = 0; k < K; ++k) {
      const auto& r = rows[k];
      const cilqr::DpEnvironment::ClearanceRow got = env.Clearance(r[0], r[1], r[2], r[3]);
      ++knots;
      for (int col = 0; col < 4; ++col)
        if (std::memcmp(&got.clearance[col], &clearance[k][col], 8) != 0 || got.nearest[col] != nearest[k][col]) {
          std::fprintf(stderr, "case %d knot %d column %d: %.17g by obstacle %d, expected %.17g by %d\n", (int)c, (int)k, col,
                       got.clearance[col], got.nearest[col], clearance[k][col], (int)nearest[k][col]);
          ++failures;
        }
    }
  }
  std::fclose(f);
  std::printf("%d cases, %d knots, %d failures\n", (int)n_cases, knots, failures);
  return failures == 0 ? 0 : 1;
}
