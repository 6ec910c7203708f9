"""QLearner: the training step of independent Q-learning (reference: learners/q_learner.py:10-231,
mock_constellation_iql.yaml), with everything on the device.

train() is SAPQLearner's -- reward and return standardisation, the live and target unrolls
(BasicMAC.forward_sequence), the 1-step target, the masked L2 loss, gradient clipping, Adam,
hard / soft target updates, the selector-agent sync and the logged stats are the same lines in
both reference learners -- with the reference's own target (q_learner.py:87-98): unavailable
actions at -9999999, then the per-agent maximum of the target Q or, with double_q, the target
Q at the argmax of the masked live Q.  No assignment problem is solved.

Only mixer = None (the IQL config's setting) is ported.
"""
import torch

from .sap_q_learner import SAPQLearner


class QLearner(SAPQLearner):
    def _target_max_qvals(self, target_mac_out, avail_actions, mac_out):
        unavailable = avail_actions == 0
        target_mac_out = target_mac_out.masked_fill(unavailable[:, 1:], -9999999.0)
        if self.args.double_q:
            # the actions that maximise the live Q (double Q-learning)
            live = mac_out.detach().masked_fill(unavailable, -9999999.0)
            cur_max_actions = live[:, 1:].max(dim=3, keepdim=True)[1]
            return torch.gather(target_mac_out, 3, cur_max_actions).squeeze(3)
        return target_mac_out.max(dim=3)[0]
