// cilqr_check_collisions_batch (include/cilqr.h): the host side -- argument checks, the barrier table and the vehicle's
// discs by DpEnvironment's own constructor (so that they are the host audit's bits), staging of HOST arrays, the launch of
// kernels_collision.hip, the count's way back.
#include <cstring>
#include <vector>

#include "audit_batch.hpp"

using namespace cilqr;

extern "C" int cilqr_check_collisions_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                                            int32_t layout, const double* rows, int32_t n_knots, double collision_buffer,
                                            uint8_t* mask, int32_t* first_hit, int32_t* n_hit, int32_t* n_colliding) {
  if (h == nullptr || cfg == nullptr || scenes == nullptr || rows == nullptr || first_hit == nullptr ||
      scenes->center == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_audit_batch(sb, layout, n_knots, collision_buffer)) return rc;
  if (int rc = check_audit_admissible(h, sb, n_knots)) return rc;
  const bool on_host = sb.memory == CILQR_MEM_HOST;

  // ---- the road and the vehicle, by the host planner's own constructor
  const DpEnvironment env(dp_config_of(*cfg), reference_line_of(sb.center, sb.n_center));
  const std::vector<DpPoint2>& barrier = env.barrier();
  static_assert(sizeof(DpPoint2) == 16, "the barrier table travels as [n][2] doubles");
  CollisionParams P;
  std::memset(&P, 0, sizeof(P));
  P.h = env.disc_radius() + collision_buffer;
  P.r2x = env.rear_disc_x(); P.f2x = env.front_disc_x();
  P.n_knots = n_knots; P.n_barrier = (int)barrier.size();
  scene_limits_into(&P, sb);
  P.rows = row_layout(layout);

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  // ---- work space of the handle (grown, never shrunk): the table and the count; HOST arrays: one block in, one block out
  block_layout l_tab, l_out;
  const slot s_barrier = l_tab.add(barrier.size() * 2 * 8), s_count = l_tab.add(4);
  const AuditInput in(sb, n_knots, P.rows);
  const slot s_mask = l_out.add(mask ? B * K : 0), s_first = l_out.add(B * 4), s_nhit = l_out.add(n_hit ? B * 4 : 0);
  HIP_TRY(h->cc_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->cc_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  if (on_host) {
    HIP_TRY(h->cc_in.grow(in.l.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->cc_out.grow(l_out.bytes() + 256, &h->grown_bytes));
  }

  // ---- table: pinned block -> device (the stream is waited for at the end of every call, so the block is free again)
  char* th = h->cc_tab_host.as<char>();
  char* td = h->cc_tab.as<char>();
  if (s_barrier.bytes) {
    std::memcpy(th + s_barrier.off, barrier.data(), s_barrier.bytes);
    HIP_TRY(hipMemcpyAsync(td + s_barrier.off, th + s_barrier.off, s_barrier.bytes, hipMemcpyHostToDevice, st));
  }
  P.barrier = s_barrier.in<const double>(td);
  int* d_count = s_count.in<int>(td);
  HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));

  cilqr_scene_batch dv = sb;
  const double* d_rows = rows;
  uint8_t* d_mask = mask;
  int *d_first = first_hit, *d_nhit = n_hit;
  char* bo = h->cc_out.as<char>();
  if (on_host) {
    if (int rc = in.upload(sb, rows, h->cc_in.as<char>(), st, &d_rows, &dv)) return rc;
    if (mask) d_mask = s_mask.in<uint8_t>(bo);
    d_first = s_first.in<int>(bo);
    if (n_hit) d_nhit = s_nhit.in<int>(bo);
  }
  launch_check_collisions(P, dv, d_rows, d_mask, d_first, d_nhit, d_count, st);
  HIP_TRY(hipGetLastError());
  if (on_host) {
    if (int rc = copy_out(mask, bo, s_mask, st)) return rc;
    if (int rc = copy_out(first_hit, bo, s_first, st)) return rc;
    if (int rc = copy_out(n_hit, bo, s_nhit, st)) return rc;
  }
  return wait_and_fetch_count(d_count, s_count.in<int>(th), st, n_colliding);
}
