/* window_twin.c -- the sequential twin of the ring cssm_pf_window keeps on a single handle, written on the bookkeeping the host uses
 * (composablestatespacemodels_amd/csrc/cssm_window.h): a window is driven through a sequence of events -- open, put, restart, re-open --
 * and reports, behind every event, its depth, the slot the event wrote and the slot of every row it would return.
 *
 *   gcc -O2 -ffp-contract=off -mfma -std=c99 -shared -fPIC -o window_twin.so window_twin.c -lm
 *
 * Events: op[e] = 0 open with arg[e] slices (0 closes), 1 put, 2 restart.  Outputs per event: depth[e]; slot[e] = the slot a put wrote
 * (0xffffffff for the other events); rows[e * max_rows + j] = the slot of row j for j <= depth (0xffffffff beyond, and for an empty or
 * closed window).  Returns 0, or 1 + e for an event the window cannot take (a put on a closed window, an unknown op). */
#include <stddef.h>
#include <stdint.h>

#include "../../composablestatespacemodels_amd/csrc/cssm_window.h"

#define TWIN_NONE 0xffffffffu

int twin_window_run(const uint32_t* op, const uint32_t* arg, size_t n_events, uint32_t max_rows, uint32_t* depth, uint32_t* slot, uint32_t* rows) {
  cssm_window w;
  cssm_window_open(&w, 0u);
  for (size_t e = 0; e < n_events; ++e) {
    slot[e] = TWIN_NONE;
    if (op[e] == 0u) {
      if (arg[e] == 1u) return (int)(1 + e);
      cssm_window_open(&w, arg[e]);
    } else if (op[e] == 1u) {
      if (w.slices == 0u) return (int)(1 + e);
      slot[e] = cssm_window_put(&w);
    } else if (op[e] == 2u) {
      cssm_window_restart(&w);
    } else {
      return (int)(1 + e);
    }
    depth[e] = cssm_window_depth(&w);
    for (uint32_t j = 0; j < max_rows; ++j)
      rows[e * (size_t)max_rows + j] = (w.count && j <= cssm_window_depth(&w)) ? cssm_window_slot(&w, j) : TWIN_NONE;
  }
  return 0;
}

/* min(lag, depth) + 1 of a window holding `count` of `slices` slices */
uint32_t twin_window_rows(uint32_t slices, uint32_t count, uint32_t lag) {
  cssm_window w;
  cssm_window_open(&w, slices);
  w.count = count;
  return cssm_window_rows(&w, lag);
}
