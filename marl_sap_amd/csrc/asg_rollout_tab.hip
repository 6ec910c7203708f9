// asg_rollout_tab.hip -- the rollout kernel instances of the float64-table benefit modes
// (MT19937 compat, injected sat_prox_mat), epsilon-greedy selection.
#include "rollout_kernel.h"

#pragma clang fp contract(fast)

namespace asg {

hipError_t launch_rollout_tab(const RolloutArgs &ra, const RolloutLaunch &lc, hipStream_t s) {
    return ra.tmask ? launch_rollout_inst<2, false>(ra, lc, s) : launch_rollout_inst<1, false>(ra, lc, s);
}

}  // namespace asg
