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
  P.rows = pose_columns(layout);

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  // ---- the count, the table and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->cc, on_host, st);
  cilqr_scene_batch dv;
  const double* d_rows;
  uint8_t* d_mask;
  int *d_first, *d_nhit, *d_count;
  c.table(reinterpret_cast<const double*>(barrier.data()), barrier.size() * 2, &P.barrier);
  c.counter(&d_count);
  c.in(rows, B * K * P.rows.fields, &d_rows);
  c.scenes(sb, &dv);
  c.out(mask, B * K, &d_mask);
  c.out(first_hit, B, &d_first);
  c.out(n_hit, B, &d_nhit);
  if (int rc = c.stage()) return rc;
  launch_check_collisions(P, dv, d_rows, d_mask, d_first, d_nhit, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_colliding);
}
