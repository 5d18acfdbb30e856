// A program of its own around include/cilqr/scene_predict.hpp: the crafted table of tests/predict_cases.py (written by
// write_cases) with the host call's results as expected values.  Built with -fsanitize=address,undefined by
// tests/test_predict.py: the source trajectory and the output lie in heap blocks of exactly their size, so an index outside
// [0, T) or a row past out_samples is a report.  Two values are the same when their bits are, or when both are NaNs (which
// NaN an operation returns is the processor's choice, not the rule's).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cilqr/scene_predict.hpp"

namespace {

bool read_exact(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

bool same_value(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  char magic[8];
  int32_t n = 0;
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "SPCASE01", 8) != 0 || !read_exact(f, &n, 4)) return 2;
  int failures = 0;
  for (int c = 0; c < n; ++c) {
    int32_t T = 0, mode = 0, out_samples = 0, count = 0;
    double t0 = 0.0, max_age = 0.0, sample_dt = 0.0;
    if (!read_exact(f, &T, 4)) return 2;
    std::vector<double> traj((size_t)T * 4);
    if (!read_exact(f, traj.data(), traj.size() * 8) || !read_exact(f, &t0, 8) || !read_exact(f, &max_age, 8) ||
        !read_exact(f, &sample_dt, 8) || !read_exact(f, &mode, 4) || !read_exact(f, &out_samples, 4) || !read_exact(f, &count, 4))
      return 2;
    std::vector<double> want((size_t)out_samples * 4);
    if (!read_exact(f, want.data(), want.size() * 8)) return 2;
    const double sentinel = -777.25;
    std::vector<double> got((size_t)out_samples * 4, sentinel);
    const cilqr::scene_predict::Motion m = cilqr::scene_predict::motion(traj.data(), T, t0, mode, max_age);
    const int got_count =
        cilqr::scene_predict::predict_trajectory(traj.data(), T, t0, mode, max_age, sample_dt, out_samples, got.data());
    bool same = got_count == count && m.j >= -1 && m.j < T && (m.j >= 0) == (count > 0);
    for (size_t i = 0; same && i < got.size(); ++i) same = same_value(got[i], want[i]);
    if (!same) {
      std::printf("case %d: count %d (want %d), latest observation %d of %d\n", c, got_count, count, m.j, T);
      ++failures;
    }
  }
  std::fclose(f);
  std::printf("%d cases, %d failures\n", n, failures);
  return failures == 0 ? 0 : 1;
}
