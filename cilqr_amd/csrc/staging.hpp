// Private to cilqr_amd/csrc: how the entry points that take HOST or DEVICE arrays lay several arrays out in ONE device
// block -- every array at a 256-byte boundary, in the order asked for -- and move them in and out of it.
#pragma once
#include "solver_priv.hpp"

namespace cilqr {

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// one array's place in a block
struct slot {
  size_t off = 0, bytes = 0;
  template <typename T>
  T* in(void* block) const { return reinterpret_cast<T*>(static_cast<char*>(block) + off); }
};

class block_layout {
 public:
  slot add(size_t bytes) { const slot s{end_, bytes}; end_ += round256(bytes); return s; }
  size_t bytes() const { return end_; }   // of all slots handed out so far

 private:
  size_t end_ = 0;
};

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

}  // namespace cilqr
