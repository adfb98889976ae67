// cssm_fleet_d.hip -- k_fleet_series for ONE latent dimension (-DCSSM_FLEET_D=d): sixteen objects `make -j` builds side by side, as
// cssm_prop.hip does for k_propagate.
#include <hip/hip_runtime.h>

#include "cssm_fleet.hip.h"

#ifndef CSSM_FLEET_D
#error "compile with -DCSSM_FLEET_D=<latent dimension>"
#endif

#define CSSM_FLEET_NAME2(d) cssm_fleet_launch_d##d
#define CSSM_FLEET_NAME(d) CSSM_FLEET_NAME2(d)

int CSSM_FLEET_NAME(CSSM_FLEET_D)(const FleetLaunch& l) {
#define CSSM_FLEET_RUN(...) hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, __VA_ARGS__>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args)
  if (l.lgcp) {       // an LGCP fleet serves the record calls without a rider and `filter` (cssm_fleet.hip refuses the others before a launch)
    if (l.kind == FleetKind::path) CSSM_FLEET_RUN(true, false, false, false, false, true);
    else if (l.kind == FleetKind::plain) CSSM_FLEET_RUN(false, false, false, false, false, true);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
  }
  switch (l.kind) {   // (the object holds the kernels in the order they are named here: reordering the cases reorders its code)
    case FleetKind::fcst: CSSM_FLEET_RUN(false, false, false, true); break;
    case FleetKind::ival: CSSM_FLEET_RUN(false, false, true); break;
    case FleetKind::hist: CSSM_FLEET_RUN(false, true); break;
    case FleetKind::path: CSSM_FLEET_RUN(true); break;
    case FleetKind::plain: CSSM_FLEET_RUN(false); break;
    case FleetKind::ring: CSSM_FLEET_RUN(false, false, false, false, true); break;
  }
#undef CSSM_FLEET_RUN
  return (int)hipGetLastError();
}
