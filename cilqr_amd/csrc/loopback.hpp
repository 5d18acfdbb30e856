// Loopback rendezvous: W endpoints inside ONE process stand in for W ranks of a communicator, so that the W > 1 paths of
// cilqr_gather_results (comm.hip) run on a machine with one GPU.  TEST transport only -- RCCL is the product transport.
//
// No HIP in here: the registry, the mailboxes, the matching and the bounded waits are plain C++ (tests/cpp/loopback_test.cc
// runs them under ThreadSanitizer with memcpy as the copy and threads as ranks).  How a payload is completed on the
// sending side and copied on the receiving side is passed to group_end as two callables.
//
// Host-synchronous on purpose.  send / recv between group_start and group_end only record the operation; group_end
//   1. completes the sender's own work (sync()), so that every payload it is about to publish is final,
//   2. publishes (pointer, count, type) of every send in the mailbox of the ordered pair (this rank, peer),
//   3. for every receive waits for the mailbox entry of (peer, this rank), compares count and type with its own and --
//      only if they match -- calls copy(dst, src, bytes), which returns when the bytes have arrived; then acknowledges,
//   4. waits for the acknowledgement of every send.
// Nothing waits on the device for another endpoint's work, so the hardware queues the endpoints share cannot make a
// wait depend on work queued behind itself.  The price: an operation is complete when group_end returns, which is
// stricter than RCCL's stream order, so this transport cannot see a buffer that is reused before it has left.
//
// Every wait is a condition-variable wait against ONE deadline per group_end (now + timeout_ms): a peer that never comes
// is Status::timeout, not a hang.  (The one wait without a deadline: a sender whose entry a receiver has already taken
// waits until that receiver's copy is over -- the entry and the payload are the sender's, and the copy is finite.)  A pair
// whose counts or types differ fails on both sides at once, with no copy; group_end still carries out every other
// operation of its group before it reports the first failure, so that uninvolved peers are not left waiting.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace cilqr {
namespace loopback {

enum class Status : int { ok = 0, mismatch = 1, timeout = 2, copy_failed = 3, usage = 4, taken = 5 };

inline const char* status_string(Status s) {
  switch (s) {
    case Status::ok: return "ok";
    case Status::mismatch: return "loopback: count or type differs between the two sides of a send/receive pair";
    case Status::timeout: return "loopback: timed out waiting for the peer";
    case Status::copy_failed: return "loopback: completing or copying a payload failed";
    case Status::usage: return "loopback: send/recv outside a group, a peer outside the world, or a group left open";
    case Status::taken: return "loopback: the rank is taken, or the group was created with another world size";
  }
  return "loopback: unknown status";
}

using SyncFn = std::function<bool()>;                                         // sender: my payloads are final
using CopyFn = std::function<bool(void* dst, const void* src, size_t bytes)>; // receiver: returns when the bytes are there

namespace detail {

// what a sender publishes; lives in its group_end until acknowledged or withdrawn
struct Entry {
  const void* ptr = nullptr;
  size_t count = 0, elem_bytes = 0;
  int type = 0;
  bool taken = false, done = false;   // a receiver holds it / has answered
  Status status = Status::ok;
};

struct Group {
  explicit Group(int w) : world(w), member(w, false), box((size_t)w * w) {}
  const int world;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<bool> member;
  int members = 0;
  std::vector<std::deque<Entry*>> box;   // [src * world + dst], first in first out
};

struct Registry {
  std::mutex mu;
  std::map<uint64_t, std::shared_ptr<Group>> groups;
};
inline Registry& registry() {
  static Registry r;
  return r;
}

}  // namespace detail

// groups alive in the process (a group lives from its first endpoint's creation to its last endpoint's destruction)
inline size_t registry_size() {
  detail::Registry& R = detail::registry();
  std::lock_guard<std::mutex> lk(R.mu);
  return R.groups.size();
}

class Endpoint {
 public:
  // joins group `key` as `rank` of `world` (the first endpoint creates the group); not collective
  static Status create(uint64_t key, int rank, int world, int timeout_ms, std::unique_ptr<Endpoint>* out) {
    if (out == nullptr || world < 1 || rank < 0 || rank >= world || timeout_ms <= 0) return Status::usage;
    detail::Registry& R = detail::registry();
    std::lock_guard<std::mutex> lk(R.mu);
    std::shared_ptr<detail::Group>& slot = R.groups[key];
    const bool fresh = slot == nullptr;
    if (fresh) slot = std::make_shared<detail::Group>(world);
    std::shared_ptr<detail::Group> g = slot;
    {
      std::lock_guard<std::mutex> gl(g->mu);
      if (g->world != world || g->member[rank]) {
        if (fresh) R.groups.erase(key);
        return Status::taken;
      }
      g->member[rank] = true;
      ++g->members;
    }
    out->reset(new Endpoint(key, std::move(g), rank, timeout_ms));
    return Status::ok;
  }

  ~Endpoint() {
    detail::Registry& R = detail::registry();
    std::lock_guard<std::mutex> lk(R.mu);
    std::lock_guard<std::mutex> gl(g_->mu);
    g_->member[rank_] = false;
    if (--g_->members == 0) {
      auto it = R.groups.find(key_);
      if (it != R.groups.end() && it->second == g_) R.groups.erase(it);
    }
  }

  Endpoint(const Endpoint&) = delete;
  Endpoint& operator=(const Endpoint&) = delete;

  int rank() const { return rank_; }
  int world() const { return g_->world; }

  Status group_start() {
    if (open_) return Status::usage;
    open_ = true;
    ops_.clear();
    return Status::ok;
  }
  Status send(const void* buf, size_t count, int type, size_t elem_bytes, int peer) {
    return record(true, const_cast<void*>(buf), count, type, elem_bytes, peer);
  }
  Status recv(void* buf, size_t count, int type, size_t elem_bytes, int peer) {
    return record(false, buf, count, type, elem_bytes, peer);
  }

  // carries out every recorded operation; the first failure (in the order the operations were recorded) is returned
  Status group_end(const SyncFn& sync, const CopyFn& copy) {
    if (!open_) return Status::usage;
    open_ = false;
    detail::Group& g = *g_;
    const int W = g.world;
    // (system_clock: libstdc++ then waits with pthread_cond_timedwait, which ThreadSanitizer follows; the steady clock's
    // pthread_cond_clockwait is unknown to older ThreadSanitizer runtimes, which then report the mutex as held across the wait)
    const auto deadline = std::chrono::system_clock::now() + std::chrono::milliseconds(timeout_ms_);
    std::vector<Status> result(ops_.size(), Status::ok);
    std::vector<detail::Entry> entries(ops_.size());
    bool sends = false;
    for (const Op& o : ops_) sends = sends || o.is_send;
    // 1. + 2. my payloads are final, then published (a failed sync publishes nothing: the receivers time out)
    const bool synced = !sends || sync();
    {
      std::lock_guard<std::mutex> lk(g.mu);
      for (size_t i = 0; i < ops_.size(); ++i) {
        const Op& o = ops_[i];
        if (!o.is_send) continue;
        if (!synced) {
          result[i] = Status::copy_failed;
          continue;
        }
        detail::Entry& e = entries[i];
        e.ptr = o.buf;
        e.count = o.count;
        e.elem_bytes = o.elem_bytes;
        e.type = o.type;
        g.box[(size_t)rank_ * W + o.peer].push_back(&e);
      }
    }
    g.cv.notify_all();
    // 3. the receives, in the order they were recorded
    for (size_t i = 0; i < ops_.size(); ++i) {
      const Op& o = ops_[i];
      if (o.is_send) continue;
      std::deque<detail::Entry*>& q = g.box[(size_t)o.peer * W + rank_];
      detail::Entry* e = nullptr;
      {
        std::unique_lock<std::mutex> lk(g.mu);
        if (!g.cv.wait_until(lk, deadline, [&] { return !q.empty(); })) {
          result[i] = Status::timeout;
          continue;
        }
        e = q.front();
        q.pop_front();
        e->taken = true;
        if (e->count != o.count || e->type != o.type || e->elem_bytes != o.elem_bytes) {
          e->status = result[i] = Status::mismatch;
          e->done = true;
        }
      }
      if (result[i] == Status::ok) {
        const bool copied = copy(o.buf, e->ptr, o.count * o.elem_bytes);   // (outside the lock: the entry is mine while taken)
        std::lock_guard<std::mutex> lk(g.mu);
        if (!copied) e->status = result[i] = Status::copy_failed;
        e->done = true;
      }
      g.cv.notify_all();
    }
    // 4. the acknowledgements of my sends; one that nobody took by the deadline is withdrawn
    for (size_t i = 0; i < ops_.size(); ++i) {
      const Op& o = ops_[i];
      if (!o.is_send || !synced) continue;
      detail::Entry& e = entries[i];
      std::unique_lock<std::mutex> lk(g.mu);
      if (!g.cv.wait_until(lk, deadline, [&] { return e.done; })) {
        if (e.taken) {
          g.cv.wait(lk, [&] { return e.done; });   // a receiver is copying from it: finite, and the payload is mine
        } else {
          std::deque<detail::Entry*>& q = g.box[(size_t)rank_ * W + o.peer];
          for (auto it = q.begin(); it != q.end(); ++it)
            if (*it == &e) {
              q.erase(it);
              break;
            }
          result[i] = Status::timeout;
          continue;
        }
      }
      result[i] = e.status;
    }
    ops_.clear();
    for (Status s : result)
      if (s != Status::ok) return s;
    return Status::ok;
  }

 private:
  struct Op {
    bool is_send;
    void* buf;
    size_t count;
    int type;
    size_t elem_bytes;
    int peer;
  };
  Endpoint(uint64_t key, std::shared_ptr<detail::Group> g, int rank, int timeout_ms)
      : key_(key), g_(std::move(g)), rank_(rank), timeout_ms_(timeout_ms) {}
  Status record(bool is_send, void* buf, size_t count, int type, size_t elem_bytes, int peer) {
    if (!open_ || peer < 0 || peer >= g_->world || peer == rank_ || (buf == nullptr && count > 0)) return Status::usage;
    ops_.push_back(Op{is_send, buf, count, type, elem_bytes, peer});
    return Status::ok;
  }

  const uint64_t key_;
  const std::shared_ptr<detail::Group> g_;
  const int rank_, timeout_ms_;
  bool open_ = false;
  std::vector<Op> ops_;
};

}  // namespace loopback
}  // namespace cilqr
