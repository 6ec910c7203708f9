// asg_rollout_q.hip -- the rollout kernel instances that write the agent's Q rows instead of
// selecting (asg_step_forward / asg_reset_forward, both benefit sources).
#include "rollout_kernel.h"

#pragma clang fp contract(fast)

namespace asg {

hipError_t launch_rollout_q(const RolloutArgs &ra, const RolloutLaunch &lc, hipStream_t s) {
    if (!ra.table32) return launch_rollout_inst<0, true>(ra, lc, s);
    return ra.tmask ? launch_rollout_inst<2, true>(ra, lc, s) : launch_rollout_inst<1, true>(ra, lc, s);
}

}  // namespace asg
