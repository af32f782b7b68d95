// rs_revalidate.h -- what restir.hip asks of shadow_revalidate.hip in a phase-A call, and what its temporal merge gets back.
#pragma once
#include "rs_light_history.h"

#if defined(__HIPCC__)
namespace rs {
// The marked form of the temporal merge (k_temporal_marked): pixel i's temporal candidate merges as if its slot held W = 0 when
// flag[i] == epoch.  flag null: the call launched no k_revalidate and takes the unmarked kernel.
struct RevalMarks { const unsigned* flag; unsigned epoch; };
}  // namespace rs

// After rs_light_history_phase_a, on the library stream: notes the scene and its count of geometry edits for the end of the frame and,
// with the switch on in a call that merges, launches k_revalidate for rows [y0, y1) when rs_plan_revalidation (rs_revalidate_plan.h) says
// so.  rtFlag: k_retarget's flags of this call, null when it was not launched.
int rs_revalidate_phase_a(rs_restir* r, const rs_scene* scene, bool merges, const rs::SurfPlanes& sp, const GBufView& g, int y0, int y1, int tilesX, int tilesY,
                          unsigned long long* rayCounter, const int* rtFlag, rs::RevalMarks* marks);
#endif
