/* cssm_window.h -- the bookkeeping of the ring cssm_pf_window keeps on a single handle (cssm_intervals.hip): which slot holds the newest
 * slice, how deep the window is behind a put, the slot of row j, and the restart.  Integers only; the host and the sequential twin
 * tests/cpp/window_twin.c share it.
 *
 * A window of `slices` slots holds `count` slices, 0 .. slices: the base slice and the records behind it.  Its depth -- the records
 * remembered behind the base slice -- is count - 1 (0 for an empty window); a full ring overwrites its oldest slot and the depth stays
 * slices - 1.  Row j, 0 <= j <= depth, lives j slots behind the newest: no row is ever read from a slot written since. */
#ifndef CSSM_WINDOW_H
#define CSSM_WINDOW_H

#include <stdint.h>

#ifndef CSSM_HD
#if defined(__HIPCC__)
#define CSSM_HD __host__ __device__ inline
#else
#define CSSM_HD static inline
#endif
#endif

typedef struct cssm_window {
  uint32_t slices;   /* slots of the ring; 0 = no window */
  uint32_t newest;   /* slot of the newest slice (count >= 1) */
  uint32_t count;    /* slices held, 0 .. slices */
} cssm_window;

/* opening (slices >= 2) and closing (0): an empty window either way */
CSSM_HD void cssm_window_open(cssm_window* w, uint32_t slices) { w->slices = slices; w->newest = 0u; w->count = 0u; }
/* what every call that writes the handle's cloud, key or parameters does: the slices held say nothing about the cloud any more */
CSSM_HD void cssm_window_restart(cssm_window* w) { w->newest = 0u; w->count = 0u; }
CSSM_HD uint32_t cssm_window_depth(const cssm_window* w) { return w->count ? w->count - 1u : 0u; }
/* the slot the next slice goes to, which becomes the newest; the window must be open */
CSSM_HD uint32_t cssm_window_put(cssm_window* w) {
  const uint32_t slot = w->count ? (w->newest + 1u == w->slices ? 0u : w->newest + 1u) : 0u;
  w->newest = slot;
  if (w->count < w->slices) w->count++;
  return slot;
}
/* the slot of row j (0 = the newest), j <= depth */
CSSM_HD uint32_t cssm_window_slot(const cssm_window* w, uint32_t j) { return w->newest >= j ? w->newest - j : w->newest + w->slices - j; }
/* the rows a call with `lag` returns: min(lag, depth) + 1 */
CSSM_HD uint32_t cssm_window_rows(const cssm_window* w, uint32_t lag) {
  const uint32_t depth = cssm_window_depth(w);
  return (lag < depth ? lag : depth) + 1u;
}

#endif
