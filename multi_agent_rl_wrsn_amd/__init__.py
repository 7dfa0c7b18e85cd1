"""MI355X-native vectorised WRSN environment: the step path of nguyenngocbaocmt02/multi_agent_rl_wrsn
(physical_env.network / physical_env.mc dynamics behind rl_env.WRSN) as hand-written gfx950 HIP kernels behind a
C-ABI (include/wrsn_hip.h).  Python here is host glue: scenario I/O, the batched `VecWRSN`, the drop-in `WRSN`
facade and the environment sharding helpers.  Importing the package does not load the HIP library; constructing an
environment does, and fails loudly when it is missing or no HIP device is present."""
from .scenario import (DEFAULT_MC_SPEC, DEFAULT_NODE_SPEC, Scenario, load_mc_yaml, load_scenario_yaml,  # noqa: F401
                       scenario_from_golden, synth_batch, synth_scenario)
from .sharding import RolloutStats, init_distributed, launch_ranks, shard_range  # noqa: F401
from ._lib import ENT_ENV, ENT_ENV_F, ENT_MC, ENT_MC_F, ENT_NODE, ENT_NODE_F, pool_draw  # noqa: F401
from .vec_env import EpisodeLog, Lookahead, VecWRSN, build_scenario_pool  # noqa: F401
from .evaluate import EntityPolicy, HeuristicLabelPolicy, HeuristicPolicy, LookaheadPolicy, PointerPolicy, UniformPolicy, evaluate_policy  # noqa: F401
from .wrsn import WRSN  # noqa: F401
from .ippo import (BatchedEntityIPPO, BatchedEntityPointerIPPO, BatchedIPPO, EntityPointerPPOLearner, EntityPPOLearner, EntityTransitionBuffers, PPOLearner, TransitionBuffers,  # noqa: F401
                   build_entity_networks, build_networks, entity_row_elems, pack_entity_actor, pack_entity_critic, select_batch, unpack_entity_actor, unpack_entity_critic,
                   build_entity_pointer_networks, pack_entity_pointer_actor, unpack_entity_pointer_actor)

__all__ = ["Scenario", "load_scenario_yaml", "load_mc_yaml", "synth_scenario", "synth_batch", "scenario_from_golden",
           "DEFAULT_NODE_SPEC", "DEFAULT_MC_SPEC", "VecWRSN", "build_scenario_pool", "pool_draw", "ENT_NODE", "ENT_MC", "ENT_ENV", "ENT_NODE_F", "ENT_MC_F", "ENT_ENV_F", "WRSN", "RolloutStats", "init_distributed", "launch_ranks", "shard_range",
           "BatchedIPPO", "PPOLearner", "TransitionBuffers", "build_networks", "select_batch",
           "EntityTransitionBuffers", "EntityPPOLearner", "BatchedEntityIPPO", "build_entity_networks", "entity_row_elems", "pack_entity_actor", "pack_entity_critic", "unpack_entity_actor",
           "unpack_entity_critic", "EpisodeLog", "evaluate_policy", "EntityPolicy", "HeuristicPolicy", "HeuristicLabelPolicy", "UniformPolicy",
           "build_entity_pointer_networks", "pack_entity_pointer_actor", "unpack_entity_pointer_actor", "EntityPointerPPOLearner", "BatchedEntityPointerIPPO",
           "PointerPolicy", "Lookahead", "LookaheadPolicy"]
