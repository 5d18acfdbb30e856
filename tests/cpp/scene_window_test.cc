// A program of its own around include/cilqr/scene_window.hpp: the crafted table of tests/scene_window_cases.py (written by
// write_cases) with the host call's results as expected values.  Built with -fsanitize=address,undefined by
// tests/test_scene_window.py: the source trajectory and the output lie in heap blocks of exactly their size, so an index
// outside [0, T) or a row past out_samples is a report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cilqr/scene_window.hpp"

namespace {

bool read_exact(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  char magic[8];
  int32_t n = 0;
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "SWCASE01", 8) != 0 || !read_exact(f, &n, 4)) return 2;
  int failures = 0;
  for (int c = 0; c < n; ++c) {
    int32_t T = 0, out_samples = 0, count = 0;
    double t0 = 0.0, span = 0.0;
    if (!read_exact(f, &T, 4)) return 2;
    std::vector<double> traj((size_t)T * 4);
    if (!read_exact(f, traj.data(), traj.size() * 8) || !read_exact(f, &t0, 8) || !read_exact(f, &span, 8) ||
        !read_exact(f, &out_samples, 4) || !read_exact(f, &count, 4))
      return 2;
    std::vector<double> want((size_t)out_samples * 4);
    if (!read_exact(f, want.data(), want.size() * 8)) return 2;
    const double sentinel = -777.25;
    std::vector<double> got((size_t)out_samples * 4, sentinel);
    const cilqr::scene_window::Bounds w = cilqr::scene_window::window_bounds(traj.data(), T, t0, span);
    const int got_count = cilqr::scene_window::window_trajectory(traj.data(), T, t0, span, out_samples, got.data());
    const bool bounds_ok = T < 1 ? w.count == 0 : (w.lo >= 0 && w.hi <= T - 1 && w.count >= 1 && w.count == w.hi - w.lo + 1);
    const bool same = got_count == count && std::memcmp(got.data(), want.data(), want.size() * 8) == 0;
    if (!bounds_ok || !same) {
      std::printf("case %d: count %d (want %d), bounds %d..%d\n", c, got_count, count, w.lo, w.hi);
      ++failures;
    }
  }
  std::fclose(f);
  std::printf("%d cases, %d failures\n", n, failures);
  return failures == 0 ? 0 : 1;
}
