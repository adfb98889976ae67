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
  if (l.fcst) hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, false, false, false, true>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  else if (l.ival) hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, false, false, true>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  else if (l.hist) hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, false, true>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  else if (l.path) hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, true>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  else hipLaunchKernelGGL((k_fleet_series<CSSM_FLEET_D, false>), dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  return (int)hipGetLastError();
}
