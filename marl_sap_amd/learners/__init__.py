"""Learners on the rollout path's kernels: the SAP Q-learner (REDA's training step) and the
Q-learner (IQL's: per-agent max targets), both with the agent unrolled in one launch each way
(the GRU agent always, the Linear agent with fused_linear_unroll), the batched LSA targets the
SAP learner uses, and the continuous PPO learner (ippo_sap.yaml's: the
bids_as_actions episodes, an ACCritic from modules/critics, the loss side in asg_ppo.hip).
Mixers and the reference's other learners are not ported."""
from .cont_ppo_learner import ContinuousPPOLearner
from .q_learner import QLearner
from .sap_q_learner import SAPQLearner
from .sap_targets import sap_target_max_qvals

REGISTRY = {"sap_q_learner": SAPQLearner, "q_learner": QLearner, "cont_ppo_learner": ContinuousPPOLearner}

__all__ = ["REGISTRY", "ContinuousPPOLearner", "QLearner", "SAPQLearner", "sap_target_max_qvals"]
