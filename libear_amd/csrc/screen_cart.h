// screen_cart.h — screenRef scaling and screenEdgeLock of a CARTESIAN Objects position (earhip group V; ITU-R BS.2127-0 sections
// 7.3.3 and 7.3.4 for cartesian == 1), as __host__ __device__ double-precision code shared by the host form and the device
// kernel of api_screen.hip.  One element is group K's point conversion to polar (conversion.h), group R's scale and lock
// (screen.h) and group K's point conversion back, each called as it stands: the bits of a flagged element are those of the
// three entry points chained on the same side, and an element with no flag set never meets any of them.
#pragma once

#include "conversion.h"
#include "screen.h"

namespace earhip {
namespace screen {

// One element.  Returns EARHIP_OK and the new position; EARHIP_INVALID_ARGUMENT for an element that is refused (a non-finite
// coordinate or a lock code above 2, with a flag set); or the code of a conversion that failed.  On any code but EARHIP_OK the
// outputs are the inputs.  An element with no flag set is not looked at: its bits pass through, whatever they are.
__host__ __device__ inline int apply_cart_one(const Map &m, double x, double y, double z, unsigned screen_ref, unsigned lock_h,
                                              unsigned lock_v, double out[3]) {
  out[0] = x, out[1] = y, out[2] = z;
  if (m.identity || (screen_ref == 0 && lock_h == 0 && lock_v == 0)) return EARHIP_OK;
  // (the comparisons are false for a NaN)
  const double inf = HUGE_VAL;
  if (!(fabs(x) < inf) || !(fabs(y) < inf) || !(fabs(z) < inf) || lock_h > 2 || lock_v > 2) return EARHIP_INVALID_ARGUMENT;
  double polar[3], az, el, cart[3];
  int st = conv::point_cart_to_polar(x, y, z, polar);
  if (st != EARHIP_OK) return st;
  // azimuth in [-180, 180] and elevation in [-90, 90]: group R's own checks pass; the distance is carried through
  if (apply_one(m, polar[0], polar[1], screen_ref, lock_h, lock_v, az, el) != 0) return EARHIP_INVALID_ARGUMENT;
  st = conv::point_polar_to_cart(az, el, polar[2], cart);
  if (st != EARHIP_OK) return st;
  out[0] = cart[0], out[1] = cart[1], out[2] = cart[2];
  return EARHIP_OK;
}

}  // namespace screen
}  // namespace earhip
