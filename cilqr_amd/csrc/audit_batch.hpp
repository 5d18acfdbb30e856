// Private to cilqr_amd/csrc: what the host sides of the two batched audits (collision_batch.hip, clearance_batch.hip)
// have literally in common -- the checks around their own arguments, the input block of a HOST call, the count's way back.
#pragma once
#include "collision.hpp"
#include "scene_batch.hpp"

namespace cilqr {

// before an audit's own scalar checks: the batch, then layout, knot count and buffer
inline int check_audit_batch(const cilqr_scene_batch& sb, int layout, int n_knots, double collision_buffer) {
  if (int rc = check_scene_batch(sb)) return rc;
  return check_audit_arguments(layout, n_knots, collision_buffer);
}
// after them: the declared limits, the handle, the counts of HOST arrays
inline int check_audit_admissible(cilqr_solver* h, const cilqr_scene_batch& sb, int n_knots) {
  if (beyond_limits(sb, n_knots)) return CILQR_ERR_CAPACITY;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;
  if (sb.memory == CILQR_MEM_HOST && !host_counts_valid(sb)) return CILQR_ERR_ARG;
  return CILQR_OK;
}

// max_* of the batch into the parameters of a launch
template <class Params>
void scene_limits_into(Params* P, const cilqr_scene_batch& sb) {
  P->max_static = sb.max_static; P->max_dynamic = sb.max_dynamic; P->max_vertices = sb.max_vertices; P->max_samples = sb.max_samples;
}

// the input block of a HOST call: the rows, then the scene's arrays
struct AuditInput {
  block_layout l;
  slot rows;
  SceneImage im;
  AuditInput(const cilqr_scene_batch& sb, int n_knots, const RowLayout& r)
      : rows(l.add((size_t)sb.batch * n_knots * r.fields * 8)), im(l, sb) {}
  // both into `block`; *d_rows and *view = where they are there
  int upload(const cilqr_scene_batch& sb, const double* host_rows, char* block, hipStream_t st, const double** d_rows,
             cilqr_scene_batch* view) const {
    if (int rc = copy_in(block, rows, host_rows, st)) return rc;
    if (int rc = im.upload(sb, block, st, view)) return rc;
    *d_rows = rows.in<const double>(block);
    return CILQR_OK;
  }
};

// the count of a call (zeroed on the device before the launch): into the pinned int, the stream waited for (this stream
// alone: solves on other handles go on), and out to the caller who asked
inline int wait_and_fetch_count(const int* d_count, int* count_host, hipStream_t st, int32_t* out) {
  HIP_TRY(hipMemcpyAsync(count_host, d_count, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (out) *out = *count_host;
  return CILQR_OK;
}

}  // namespace cilqr
