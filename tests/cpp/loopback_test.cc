// Stand-alone host test of the loopback rendezvous (cilqr_amd/csrc/loopback.hpp): threads as ranks, memcpy as the copy.
// Built with -fsanitize=thread and run as a child process by tests/test_loopback.py.
// Prints "<n> checks, <f> failures"; the exit status is 0 only without failures.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "loopback.hpp"

namespace lb = cilqr::loopback;
using lb::Endpoint;
using lb::Status;

static std::atomic<int> g_checks{0}, g_failures{0};
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

enum { kI64 = 4, kF64 = 8 };   // type tags, as a caller would pass its own

static std::atomic<int> g_copies{0}, g_syncs{0};
static bool do_sync() {
  ++g_syncs;
  return true;
}
static bool do_copy(void* dst, const void* src, size_t bytes) {
  ++g_copies;
  std::memcpy(dst, src, bytes);
  return true;
}

static double value(int rank, int round, size_t i) { return rank * 1e6 + round * 1e3 + (double)i; }

static std::vector<std::unique_ptr<Endpoint>> make_world(uint64_t key, int W, int timeout_ms) {
  std::vector<std::unique_ptr<Endpoint>> eps(W);
  for (int r = 0; r < W; ++r) CHECK(Endpoint::create(key, r, W, timeout_ms, &eps[r]) == Status::ok);
  return eps;
}

// the shape of the results gather: an agreement (every rank one int64 to the root, a verdict back), then one block per rank
// into the root's slots -- `rounds` times on one communicator, for every root
static void gather_rounds(int W, int rounds) {
  auto eps = make_world(100 + W, W, 20000);
  const size_t n = 257;
  for (int root = 0; root < W; ++root) {
    std::vector<std::thread> th;
    std::vector<std::vector<double>> recv(rounds, std::vector<double>((size_t)(W - 1) * n, -1.0));
    for (int r = 0; r < W; ++r)
      th.emplace_back([&, r] {
        Endpoint& e = *eps[r];
        for (int round = 0; round < rounds; ++round) {
          std::vector<long long> said(W, -1);
          long long mine = 40 + round, verdict = -1;
          CHECK(e.group_start() == Status::ok);
          if (r == root) {
            for (int p = 0; p < W; ++p)
              if (p != root) CHECK(e.recv(&said[p], 1, kI64, 8, p) == Status::ok);
          } else {
            CHECK(e.send(&mine, 1, kI64, 8, root) == Status::ok);
          }
          CHECK(e.group_end(do_sync, do_copy) == Status::ok);
          if (r == root) {
            verdict = 1;
            for (int p = 0; p < W; ++p)
              if (p != root && said[p] != mine) verdict = 0;
          }
          CHECK(e.group_start() == Status::ok);
          if (r == root) {
            for (int p = 0; p < W; ++p)
              if (p != root) CHECK(e.send(&verdict, 1, kI64, 8, p) == Status::ok);
          } else {
            CHECK(e.recv(&verdict, 1, kI64, 8, root) == Status::ok);
          }
          CHECK(e.group_end(do_sync, do_copy) == Status::ok);
          CHECK(verdict == 1);
          std::vector<double> block(n);
          for (size_t i = 0; i < n; ++i) block[i] = value(r, round, i);
          CHECK(e.group_start() == Status::ok);
          if (r == root) {
            for (int p = 0; p < W; ++p)
              if (p != root) CHECK(e.recv(recv[round].data() + (size_t)(p - (p > root)) * n, n, kF64, 8, p) == Status::ok);
          } else {
            CHECK(e.send(block.data(), n, kF64, 8, root) == Status::ok);
          }
          CHECK(e.group_end(do_sync, do_copy) == Status::ok);
        }
      });
    for (auto& t : th) t.join();
    for (int round = 0; round < rounds; ++round)
      for (int p = 0; p < W; ++p) {
        if (p == root) continue;
        bool same = true;
        for (size_t i = 0; i < n; ++i) same = same && recv[round][(size_t)(p - (p > root)) * n + i] == value(p, round, i);
        CHECK(same);
      }
  }
  eps.clear();
  CHECK(lb::registry_size() == 0);
}

// both directions inside one group, and two sends to one peer in one group (first in, first out)
static void exchange_both_ways() {
  auto eps = make_world(7, 2, 20000);
  double out[2][2] = {{1.5, 2.5}, {3.5, 4.5}}, in[2][2] = {{0, 0}, {0, 0}};
  std::vector<std::thread> th;
  for (int r = 0; r < 2; ++r)
    th.emplace_back([&, r] {
      Endpoint& e = *eps[r];
      CHECK(e.group_start() == Status::ok);
      CHECK(e.recv(&in[r][0], 1, kF64, 8, 1 - r) == Status::ok);
      CHECK(e.send(&out[r][0], 1, kF64, 8, 1 - r) == Status::ok);
      CHECK(e.send(&out[r][1], 1, kF64, 8, 1 - r) == Status::ok);
      CHECK(e.recv(&in[r][1], 1, kF64, 8, 1 - r) == Status::ok);
      CHECK(e.group_end(do_sync, do_copy) == Status::ok);
    });
  for (auto& t : th) t.join();
  CHECK(in[0][0] == 3.5 && in[0][1] == 4.5 && in[1][0] == 1.5 && in[1][1] == 2.5);
}

// rank 1 posts one int64 against the root's block of doubles: both fail at the rendezvous, nothing is copied for the pair,
// and rank 2's block in the same group of the root still arrives
static void count_mismatch() {
  auto eps = make_world(8, 3, 20000);
  const size_t n = 33;
  std::vector<double> recv(2 * n, -1.0), block(n, 9.25);
  long long one = 5;
  Status st[3];
  const int copies_before = g_copies.load();
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  th.emplace_back([&] {
    Endpoint& e = *eps[0];
    e.group_start();
    e.recv(recv.data(), n, kF64, 8, 1);
    e.recv(recv.data() + n, n, kF64, 8, 2);
    st[0] = e.group_end(do_sync, do_copy);
  });
  th.emplace_back([&] {
    Endpoint& e = *eps[1];
    e.group_start();
    e.send(&one, 1, kI64, 8, 0);
    st[1] = e.group_end(do_sync, do_copy);
  });
  th.emplace_back([&] {
    Endpoint& e = *eps[2];
    e.group_start();
    e.send(block.data(), n, kF64, 8, 0);
    st[2] = e.group_end(do_sync, do_copy);
  });
  for (auto& t : th) t.join();
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  CHECK(st[0] == Status::mismatch && st[1] == Status::mismatch && st[2] == Status::ok);
  CHECK(secs < 10.0);                                 // at the rendezvous, not at the 20 s bound
  CHECK(g_copies.load() == copies_before + 1);
  bool untouched = true, arrived = true;
  for (size_t i = 0; i < n; ++i) {
    untouched = untouched && recv[i] == -1.0;
    arrived = arrived && recv[n + i] == 9.25;
  }
  CHECK(untouched && arrived);
  // same count, another type: a mismatch as well
  std::vector<std::thread> th2;
  double d = 0;
  long long l = 3;
  th2.emplace_back([&] {
    eps[0]->group_start();
    eps[0]->recv(&d, 1, kF64, 8, 1);
    st[0] = eps[0]->group_end(do_sync, do_copy);
  });
  th2.emplace_back([&] {
    eps[1]->group_start();
    eps[1]->send(&l, 1, kI64, 8, 0);
    st[1] = eps[1]->group_end(do_sync, do_copy);
  });
  for (auto& t : th2) t.join();
  CHECK(st[0] == Status::mismatch && st[1] == Status::mismatch && d == 0);
}

// a peer that never comes: the receive and the send end at the bound; the withdrawn send leaves nothing behind
static void missing_peer() {
  auto eps = make_world(9, 2, 300);
  double x = 1.0, y = 0.0;
  auto timed = [&](const std::function<Status()>& f, Status* s) {
    const auto t0 = std::chrono::steady_clock::now();
    *s = f();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  Status s;
  double secs = timed([&] {
    eps[0]->group_start();
    eps[0]->recv(&y, 1, kF64, 8, 1);
    return eps[0]->group_end(do_sync, do_copy);
  }, &s);
  CHECK(s == Status::timeout && secs >= 0.25 && secs < 5.0);
  secs = timed([&] {
    eps[0]->group_start();
    eps[0]->send(&x, 1, kF64, 8, 1);
    return eps[0]->group_end(do_sync, do_copy);
  }, &s);
  CHECK(s == Status::timeout && secs >= 0.25 && secs < 5.0);
  // the communicator is still good, and the withdrawn send is not what rank 1 receives now
  double fresh = 2.0;
  Status st[2];
  std::thread a([&] {
    eps[0]->group_start();
    eps[0]->send(&fresh, 1, kF64, 8, 1);
    st[0] = eps[0]->group_end(do_sync, do_copy);
  });
  std::thread b([&] {
    eps[1]->group_start();
    eps[1]->recv(&y, 1, kF64, 8, 0);
    st[1] = eps[1]->group_end(do_sync, do_copy);
  });
  a.join();
  b.join();
  CHECK(st[0] == Status::ok && st[1] == Status::ok && y == 2.0);
}

static void registry_and_usage() {
  CHECK(lb::registry_size() == 0);
  std::unique_ptr<Endpoint> a, b, c;
  CHECK(Endpoint::create(1, 0, 2, 100, &a) == Status::ok);
  CHECK(lb::registry_size() == 1);
  CHECK(Endpoint::create(1, 0, 2, 100, &b) == Status::taken);       // the rank is taken
  CHECK(Endpoint::create(1, 1, 3, 100, &b) == Status::taken);       // another world
  CHECK(Endpoint::create(1, 2, 2, 100, &b) == Status::usage);       // a rank outside the world
  CHECK(Endpoint::create(1, 1, 2, 0, &b) == Status::usage);         // no bound, no endpoint
  CHECK(b == nullptr);
  CHECK(Endpoint::create(1, 1, 2, 100, &b) == Status::ok);
  CHECK(Endpoint::create(2, 0, 1, 100, &c) == Status::ok);          // another group beside it
  CHECK(lb::registry_size() == 2);
  double x = 0;
  CHECK(a->send(&x, 1, kF64, 8, 1) == Status::usage);               // outside a group
  CHECK(a->group_end(do_sync, do_copy) == Status::usage);
  CHECK(a->group_start() == Status::ok);
  CHECK(a->group_start() == Status::usage);
  CHECK(a->send(&x, 1, kF64, 8, 0) == Status::usage);               // to itself
  CHECK(a->send(&x, 1, kF64, 8, 2) == Status::usage);               // outside the world
  CHECK(a->group_end(do_sync, do_copy) == Status::ok);              // an empty group
  a.reset();
  CHECK(lb::registry_size() == 2);                                  // rank 1 still holds group 1
  CHECK(Endpoint::create(1, 0, 2, 100, &a) == Status::ok);          // the rank is free again
  a.reset();
  b.reset();
  CHECK(lb::registry_size() == 1);
  c.reset();
  CHECK(lb::registry_size() == 0);
  CHECK(Endpoint::create(1, 0, 5, 100, &a) == Status::ok);          // the key is free again, for any world
  a.reset();
  CHECK(lb::registry_size() == 0);
  // a group whose first create fails leaves nothing behind
  CHECK(Endpoint::create(3, 4, 2, 100, &a) == Status::usage);
  CHECK(lb::registry_size() == 0);
}

int main() {
  registry_and_usage();
  for (int W : {2, 3, 8}) gather_rounds(W, 3);
  exchange_both_ways();
  count_mismatch();
  missing_peer();
  CHECK(lb::registry_size() == 0);
  std::printf("%d checks, %d failures\n", g_checks.load(), g_failures.load());
  return g_failures.load() == 0 ? 0 : 1;
}
