"""Learners on the rollout path's kernels: the SAP Q-learner (REDA's training step) with the
agent unrolled in one launch each way, and the batched LSA targets it uses (SURVEY §8(f)
row 1).  Mixers, critics and the reference's other learners are not ported."""
from .sap_q_learner import SAPQLearner
from .sap_targets import sap_target_max_qvals

REGISTRY = {"sap_q_learner": SAPQLearner}

__all__ = ["REGISTRY", "SAPQLearner", "sap_target_max_qvals"]
