// Private to cilqr_amd/csrc: how the entry points that take HOST or DEVICE arrays lay several arrays out in ONE device
// block -- every array at a 256-byte boundary, in the order asked for -- and move them in and out of it.  `staged_call`
// is what an entry point uses: every array is handed to it in ONE statement, which says where the caller has it, how long
// it is, which way it travels and which device pointer the kernels will take; stage() and finish() do the rest.  `slot`,
// `block_layout` (both in solve_io.hpp, which has no HIP dependency), copy_in and copy_out are what it is made of, and what the
// pipelines that keep their intermediates and the caller's arrays in one work block (scene_pipeline.hip, carry_pipeline.hip) use.
#pragma once
#include <cassert>
#include <cstring>

#include "solver_priv.hpp"

namespace cilqr {

// the caller's HOST array into its slot / the slot into the caller's HOST array: nothing for an empty slot or an array
// the caller did not give
inline int copy_in(void* block, const slot& s, const void* src, hipStream_t st) {
  if (s.bytes && src) HIP_TRY(hipMemcpyAsync(s.in<char>(block), src, s.bytes, hipMemcpyHostToDevice, st));
  return CILQR_OK;
}
inline int copy_out(void* dst, void* block, const slot& s, hipStream_t st) {
  if (s.bytes && dst) HIP_TRY(hipMemcpyAsync(dst, s.in<char>(block), s.bytes, hipMemcpyDeviceToHost, st));
  return CILQR_OK;
}

// The six per-problem arrays of a scene batch, in the order they are laid out: f(member, elements) for each.
template <class F>
void scene_arrays(const cilqr_scene_batch& sb, F&& f) {
  const size_t B = (size_t)sb.batch, S = B * sb.max_static, D = B * sb.max_dynamic, V = (size_t)sb.max_vertices * 2;
  f(&cilqr_scene_batch::static_points, S * V);
  f(&cilqr_scene_batch::static_counts, S);
  f(&cilqr_scene_batch::dynamic_polygon_points, D * V);
  f(&cilqr_scene_batch::dynamic_polygon_counts, D);
  f(&cilqr_scene_batch::dynamic_trajectories, D * sb.max_samples * 4);
  f(&cilqr_scene_batch::dynamic_trajectory_counts, D);
}

// One call of an entry point on its blocks.  Between the argument checks and the launches:
//   staged_call c(h, h->xx, on_host, st);
//   c.counter(&d_count);  c.in(rows, n, &d_rows);  c.out(flags, m, &d_flags);  ...      one statement per array
//   if (int rc = c.stage()) return rc;            the blocks grown, HOST inputs and tables on their way, the count zeroed,
//   launch(..., d_rows, d_flags, d_count, st);    every device pointer valid
//   return c.finish(n_flagged);                   HOST outputs and the count back, THIS stream waited for
// A device pointer is the caller's own on DEVICE arrays, the array's slot on HOST arrays, and NULL for an array the caller
// did not give (no slot bytes, no copy).  Blocks are sized layout + 256; a DEVICE call grows neither `in` nor `out`.  The
// pinned block is free again at the next call because every call ends with the wait.
class staged_call {
 public:
  staged_call(cilqr_solver* h, call_blocks& b, bool on_host, hipStream_t st)
      : tab_(b), io_(&b), io_account_(&h->grown_bytes), account_(&h->grown_bytes), on_host_(on_host), st_(st) {}
  // `in` and `out` of THIS call come from blocks of the caller's own, which the handle does not account for
  void io_blocks(call_blocks& own) { io_ = &own; io_account_ = nullptr; }

  template <class T> void in(const T* a, size_t n, const T** dev) { *dev = a; bind(kIn, a, n * sizeof(T), dev, &put<const T>); }
  template <class T> void out(T* a, size_t n, T** dev) { *dev = a; bind(kOut, a, n * sizeof(T), dev, &put<T>); }
  // HOST: into the output block before the launches and back after them (what the kernels leave alone stays the caller's)
  template <class T> void inout(T* a, size_t n, T** dev) { *dev = a; bind(kInOut, a, n * sizeof(T), dev, &put<T>); }
  // the six arrays of a scene batch; *view = the batch as the kernels take it
  void scenes(const cilqr_scene_batch& sb, cilqr_scene_batch* view) {
    *view = sb;
    view->memory = CILQR_MEM_DEVICE;
    scene_arrays(sb, [&](auto member, size_t n) { in(sb.*member, n, &(view->*member)); });
  }
  // a table in HOST memory whatever the call's arrays are: through the pinned block into the table block.  ONE copy carries
  // the tables of a call, from the first to the end of the last: a count or scratch declared between two tables is copied
  // over, which is why stage() zeroes the count BEHIND that copy and why scratch holds nothing before the launches.
  template <class T> void table(const T* a, size_t n, const T** dev) {
    *dev = nullptr;
    if (table_end_ == table_begin_) table_begin_ = l_tab_.bytes();   // the first table with bytes: where what travels begins
    const slot s = l_tab_.add(n * sizeof(T));
    add(kTable, a, s, dev, &put<const T>);
    table_end_ = s.off + s.bytes;
    pinned_end_ = l_tab_.bytes();
  }
  // device memory of the call behind the tables declared so far
  template <class T> void scratch(size_t n, T** dev) { *dev = nullptr; add(kScratch, nullptr, l_tab_.add(n * sizeof(T)), dev, &put<T>); }
  // the count the kernels add to: zero before the launches, fetched by finish()
  void counter(int** dev) {
    *dev = nullptr;
    s_count_ = l_tab_.add(4);
    add(kScratch, nullptr, s_count_, dev, &put<int>);
    pinned_end_ = l_tab_.bytes();
  }

  int stage() {
    if (l_tab_.bytes()) {
      HIP_TRY(tab_.tab_host.grow(pinned_end_ + 256));
      HIP_TRY(tab_.tab.grow(l_tab_.bytes() + 256, account_));
    }
    if (on_host_) {
      HIP_TRY(io_->in.grow(l_in_.bytes() + 256, io_account_));
      HIP_TRY(io_->out.grow(l_out_.bytes() + 256, io_account_));
    }
    char *th = tab_.tab_host.as<char>(), *td = tab_.tab.as<char>();
    for (int i = 0; i < n_; ++i) {
      const bound& b = a_[i];
      void* block = b.kind == kIn ? io_->in.get() : b.kind == kTable || b.kind == kScratch ? td : io_->out.get();
      if (b.kind == kTable && b.s.bytes) std::memcpy(th + b.s.off, b.host, b.s.bytes);
      if (b.kind == kIn || b.kind == kInOut)
        if (int rc = copy_in(block, b.s, b.host, st_)) return rc;
      b.put(b.dev, b.s.in<char>(block));
    }
    if (table_end_ > table_begin_)
      HIP_TRY(hipMemcpyAsync(td + table_begin_, th + table_begin_, table_end_ - table_begin_, hipMemcpyHostToDevice, st_));
    if (s_count_.bytes) HIP_TRY(hipMemsetAsync(td + s_count_.off, 0, 4, st_));
    return CILQR_OK;
  }

  // the closing step without its wait, for a call that waits its own way: count() is valid once the stream has been waited for
  int fetch() {
    for (int i = 0; i < n_; ++i)
      if (a_[i].kind == kOut || a_[i].kind == kInOut)
        if (int rc = copy_out(const_cast<void*>(a_[i].host), io_->out.get(), a_[i].s, st_)) return rc;
    if (s_count_.bytes)
      HIP_TRY(hipMemcpyAsync(tab_.tab_host.as<char>() + s_count_.off, tab_.tab.as<char>() + s_count_.off, 4, hipMemcpyDeviceToHost, st_));
    return CILQR_OK;
  }
  int count() const { return *s_count_.in<int>(tab_.tab_host.get()); }
  int finish(int32_t* count_out = nullptr) {
    if (int rc = fetch()) return rc;
    HIP_TRY(hipStreamSynchronize(st_));   // this stream alone: solves on other handles go on
    if (count_out) *count_out = count();
    return CILQR_OK;
  }

 private:
  enum kind_t { kIn, kOut, kInOut, kTable, kScratch };
  struct bound {
    kind_t kind;
    const void* host;   // the caller's array (kIn, kOut, kInOut), the table's source
    slot s;
    void* dev;          // the device pointer to fill, and how
    void (*put)(void* dev, void* p);
  };
  template <class T> static void put(void* dev, void* p) { *static_cast<T**>(dev) = static_cast<T*>(p); }

  // arrays of the caller: nothing to do on DEVICE arrays or for an array that was not given
  void bind(kind_t kind, const void* a, size_t bytes, void* dev, void (*p)(void*, void*)) {
    if (on_host_ && a != nullptr) add(kind, a, (kind == kIn ? l_in_ : l_out_).add(bytes), dev, p);
  }
  void add(kind_t kind, const void* a, slot s, void* dev, void (*p)(void*, void*)) {
    assert(n_ < kMax && "staged_call: more arrays than kMax");
    a_[n_++] = bound{kind, a, s, dev, p};
  }

  static constexpr int kMax = 24;   // the planner binds fifteen; an entry point with more raises it (add() asserts)
  call_blocks& tab_;
  call_blocks* io_;
  std::atomic<int64_t>*io_account_, *account_;
  bool on_host_;
  hipStream_t st_;
  block_layout l_tab_, l_in_, l_out_;
  size_t table_begin_ = 0, table_end_ = 0, pinned_end_ = 0;
  slot s_count_;
  bound a_[kMax];
  int n_ = 0;
};

}  // namespace cilqr
