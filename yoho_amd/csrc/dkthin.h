// The thinning rounds of disk.hip for the two entries that run them: yoho_disk_sample (disk.hip) and yoho_disk_sample_prio (salient.hip).
#pragma once
#include "common.h"

namespace yoho {

// What both entries do behind their argument checks: the workspace (B, cnt, [key64 with a priority,] the grid), the grid build and the
// launches of THE ROUNDS on `s`.  prio == nullptr: the hashed key of include/yoho_disk.h, the state handed in with resume = 1 taken
// as it is; otherwise key64 of include/yoho_salient.h, and a non-finite row handed in as 0 becomes 2.  0, or the error of the
// workspace / the grid build / a launch.
int dk_thin(yoho_ctx* c, const float* pts, int N, float radius, const float* prio, unsigned seed, int rounds, int resume, uint8_t* state,
            int32_t* n_out, hipStream_t s);

}  // namespace yoho
