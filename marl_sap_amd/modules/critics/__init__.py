"""Critic registry (reference: modules/critics/__init__.py).  Only the actor-critic learners'
ACCritic is ported; the reference's COMA, centralV and MADDPG critics are not."""
from .ac import ACCritic

REGISTRY = {"ac_critic": ACCritic}

__all__ = ["REGISTRY", "ACCritic"]
