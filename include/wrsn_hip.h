/*
 * wrsn_hip.h -- C-ABI of libwrsn_hip.so, the MI355X (gfx950) implementation of the
 * WRSN environment step path of nguyenngocbaocmt02/multi_agent_rl_wrsn.
 *
 * The reference exposes this path as a Python class, not an FFI:
 *     rl_env/WRSN.py:21   class WRSN(gym.Env)
 *     rl_env/WRSN.py:22   WRSN(scenario_path, agent_type_path, num_agent, map_size, warm_up_time, density_map)
 *     rl_env/WRSN.py:41   reset()
 *     rl_env/WRSN.py:289  step(agent_id, input_action)
 * The entry points below are what a ctypes binding for a *batched* version of that class
 * binds (INTEGRATION.md shows the stub); the Python classes `VecWRSN` / `WRSN` of
 * multi_agent_rl_wrsn_amd are built on exactly these calls.
 *
 * Conventions
 *   - every function returns 0 on success or a negative wrsn_status; nothing throws
 *     across the boundary; wrsn_last_error() returns a thread-local message;
 *   - a handle is bound to one HIP device and one stream; calls on one handle must be
 *     serialised by the caller, different handles are independent (one per GPU);
 *   - pointers documented "device" are caller-owned HIP device pointers (for instance
 *     torch.Tensor.data_ptr()); pointers documented "host" are ordinary host memory;
 *   - the library owns only its internal environment state;
 *   - step/reset are asynchronous on the handle's stream (no host synchronisation).
 */
#ifndef WRSN_HIP_H
#define WRSN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wrsn_handle wrsn_t;

enum wrsn_status {
    WRSN_OK = 0,
    WRSN_ERR_ARG = -1,        /* bad argument */
    WRSN_ERR_HIP = -2,        /* HIP runtime error, see wrsn_last_error() */
    WRSN_ERR_NO_DEVICE = -3,  /* no usable gfx950 device */
    WRSN_ERR_CAPACITY = -4,   /* neighbour / coverage / connection list capacity exceeded */
    WRSN_ERR_STATE = -5       /* call sequence error (e.g. step before scenario set) */
};

/* Batch geometry.  Mirrors the constructor arguments of WRSN (rl_env/WRSN.py:22-30). */
typedef struct wrsn_cfg {
    int32_t n_env;            /* B: number of independent environments on this handle            */
    int32_t n_node;           /* N: sensor nodes per environment (max over the batch)            */
    int32_t n_target;         /* T: targets per environment (max over the batch)                 */
    int32_t n_mc;             /* M: mobile chargers, `num_agent` (WRSN.py:26); 1..8               */
    int32_t map_size;         /* G: observation is 4 x G x G (WRSN.py:27,31); 4..128              */
    int32_t device;           /* HIP device ordinal                                               */
    int32_t max_degree;       /* average neighbour-list capacity per node (0 = default 24)        */
    int32_t max_cover;        /* average covered-target capacity per node (0 = default 8)         */
    double  warm_up_time;     /* `warm_up_time` (WRSN.py:29,53), simulated seconds                */
} wrsn_cfg;

/* node_phy_spe of a scenario file (network_scenarios/hanoi1000n50.yaml:1-11), in this order. */
typedef struct wrsn_node_spec {
    double capacity, threshold, com_range, sen_range, prob_gp, package_size, er, et, efs, emp;
    double max_time;          /* scenario key `max_time` (NetworkIO.py:34, Network.py:78)         */
} wrsn_node_spec;

/* mc_types/default.yaml:2-9 */
typedef struct wrsn_mc_spec {
    double capacity, threshold, velocity, pm, charging_range, alpha, beta, epsilon;
} wrsn_mc_spec;

/* Per-call outputs of reset/step: the numeric content of the request dict WRSN.step returns
 * (WRSN.py:323-330; terminal form :313-320).  All pointers are DEVICE pointers, caller-owned;
 * obs may be NULL (no observation is rendered). */
typedef struct wrsn_step_out {
    int32_t *agent_id;        /* [B]  id of the charger that needs an action; -1 = none (terminal / fell off) */
    double  *reward;          /* [B]  get_reward (WRSN.py:222-227); 0 when agent_id < 0            */
    uint8_t *terminal;        /* [B]  1 when net.alive == 0 at return (WRSN.py:312)                */
    double  *now;             /* [B]  env.now at return                                            */
    float   *obs;             /* [B,4,G,G] get_state(agent_id) (WRSN.py:130-186); untouched rows for agent_id < 0;
                                 uint16 bf16 bit patterns with WRSN_OBS_BF16 (wrsn_set_obs_format) */
    int32_t *status;          /* [B]  0 ok; 1 step fell off the end (reference returns None);
                                      2 every charger dead (reference would hang); 3 auto-reset performed;
                                      4 the step is still in flight (wrsn_set_step_budget), call wrsn_step again;
                                      negative: per-env error (capacity);
                                      WRSN_STATUS_POOL_INDEX: wrsn_pool_reset found pool_index outside the pool */
} wrsn_step_out;

/* per-row status of wrsn_pool_reset for a selected row whose pool_index is outside [0, n_records): the row is left as it was */
#define WRSN_STATUS_POOL_INDEX (-5)

/* what wrsn_peek copies; dst is a HOST pointer, dense [B, ...] in the listed dtype */
enum wrsn_peek_what {
    WRSN_PEEK_NODE_ENERGY = 0,   /* double [B,N]   Node.energy                                   */
    WRSN_PEEK_NODE_CS = 1,       /* double [B,N]   Node.energyCS                                  */
    WRSN_PEEK_NODE_RR = 2,       /* double [B,N]   Node.energyRR                                  */
    WRSN_PEEK_NODE_STATUS = 3,   /* int32  [B,N]   Node.status                                    */
    WRSN_PEEK_NODE_LEVEL = 4,    /* int32  [B,N]   Node.level                                     */
    WRSN_PEEK_MC = 5,            /* double [B,M,16] loc_x, loc_y, energy, status, charging, cur_x, cur_y,
                                                    cur_t, n_conn, excl, prev_minfit, act0, act1, act2, error, safe
                                                    (error: the ENVIRONMENT's error code behind a row of status
                                                    WRSN_ERR_CAPACITY, 0 = none; safe: the seconds the ENVIRONMENT may
                                                    advance before a node can reach its threshold, -1 once the network is
                                                    declared dead -- what the launch-order estimate reads; both the same
                                                    in every charger's row) */
    WRSN_PEEK_ENV = 6,           /* double [B,16]  xmin,xmax,ymin,ymax,density,moving_time_max,charging_time_max,
                                                    avg_nodes_agent,now,alive,ticks,exact_ticks,events,min_fitness,
                                                    n_edges,n_cover                                 */
    WRSN_PEEK_NODE_DEGREE = 7,   /* int32  [B,N]   len(Node.neighbors)                            */
    WRSN_PEEK_NODE_NCOVER = 8,   /* int32  [B,N]   len(Node.listTargets)                          */
    WRSN_PEEK_NODE_DIRECT = 9,   /* int32  [B,N]   node in BaseStation.direct_nodes               */
    WRSN_PEEK_TARGETS_ACTIVE = 11, /* int32 [B,T]   Network.targets_active (Network.py:9,45-55): target covered by a node the last
                                                    setLevels reached; 0 beyond an environment's own target count.  (10 is
                                                    taken by the per-phase cycle counters of diagnostic builds.)       */
    WRSN_PEEK_POOL = 13,         /* int32  [B,2]   scenario pool: the pool record the environment runs (-1 after wrsn_set_scenario* /
                                                    wrsn_load_envs, the source's value after wrsn_clone_envs) and its swaps since
                                                    wrsn_pool_set                                  */
    WRSN_PEEK_ORDER = 14,        /* uint32 [2,B]   launch order of the last wrsn_step: row 0 the keys the estimate wrote,
                                                    (0xFFFF - work in quarter seconds) << 13 | environment, from the states
                                                    and actions the call started with; row 1 the environments in launch
                                                    order, longest job first, ties by environment index.  A time-sliced call
                                                    (wrsn_set_step_deadline) walks its cyclic order and computes neither: the
                                                    peek then shows what the last call without a deadline left.  WRSN_ERR_STATE
                                                    on handles whose batch is too large to be sorted (the order is 0..B-1). */
    WRSN_PEEK_RNG_STATE = 12     /* uint32 [B,627] the environment's MT19937: the 624 state words and the index as
                                                    random.getstate()[1] lists them, then the draws since the last reset
                                                    (low, high word).  Handles that run the stochastic kernels only
                                                    (wrsn_set_scenario_seeded); WRSN_ERR_STATE otherwise. */
};

/* Create a handle for B environments on cfg->device.  Fails with WRSN_ERR_NO_DEVICE when no HIP
 * device is usable: there is no CPU fallback. */
int wrsn_create(const wrsn_cfg *cfg, wrsn_t **out);
void wrsn_destroy(wrsn_t *h);

/* Bind the handle to a HIP stream (hipStream_t passed as void*; NULL = default stream). */
int wrsn_set_stream(wrsn_t *h, void *hip_stream);

/* Load scenarios for environments [env0, env0+nenv): replaces NetworkIO.makeNetwork
 * (NetworkIO.py:19-34) + Network.__init__ (Network.py:4-33) + the t=0 probes
 * (Node.py:80-90, BaseStation.py:20-23).  HOST pointers:
 *   node_xy   [nenv, n_node, 2]   target_xy [nenv, n_target, 2]   bs_xy [nenv, 2]
 *   n_node_env / n_target_env [nenv] actual sizes (NULL = cfg sizes for all)
 *   node_spec [nenv] (or one spec broadcast when spec_stride == 0), mc_spec likewise.
 * Builds topology on the device, runs the warm-up (WRSN.py:53) on the device and caches the
 * post-warm-up snapshot reset() restores (the state after run(until=warm_up_time) is a pure
 * function of the scenario).  Synchronous.  Refuses node_spec.prob_gp != 1 (use
 * wrsn_set_scenario_seeded). */
int wrsn_set_scenario(wrsn_t *h, int32_t env0, int32_t nenv,
                      const double *node_xy, const double *target_xy, const double *bs_xy,
                      const int32_t *n_node_env, const int32_t *n_target_env,
                      const wrsn_node_spec *node_spec, int32_t node_spec_stride,
                      const wrsn_mc_spec *mc_spec, int32_t mc_spec_stride);

/* wrsn_set_scenario plus the scenario key `seed` of every environment (HOST pointer [nenv]):
 * accepts 0 <= prob_gp <= 1.  Node.py:61 draws random.random() once per live node and second and
 * generates the node's packets only when the draw is below prob_gp; NetworkIO.py:22-23 seeds
 * Python's MT19937 with random.seed(seed) on every reset.  The handle keeps that generator per
 * environment (in the post-warm-up snapshot too: every episode starts from the same stream) and
 * runs the stochastic kernels as soon as one environment has prob_gp != 1; with prob_gp == 1
 * everywhere it runs the kernels of wrsn_set_scenario and does not track the generator. */
int wrsn_set_scenario_seeded(wrsn_t *h, int32_t env0, int32_t nenv,
                             const double *node_xy, const double *target_xy, const double *bs_xy,
                             const int32_t *n_node_env, const int32_t *n_target_env,
                             const wrsn_node_spec *node_spec, int32_t node_spec_stride,
                             const wrsn_mc_spec *mc_spec, int32_t mc_spec_stride, const int64_t *seed);

/* WRSN.reset (WRSN.py:41-83) for the environments whose env_mask byte is non-zero
 * (DEVICE pointer [B]; NULL = all).  Outputs follow the reset request (agent 0, reward 0).  Rows of environments
 * the mask leaves out are not written at all: their pending request (agent_id included) stays valid. */
int wrsn_reset(wrsn_t *h, const uint8_t *env_mask, const wrsn_step_out *out);

/* WRSN.step (WRSN.py:289-330) for every environment, density_map=False path.
 *   agent_id [B] DEVICE int32: charger receiving `action` (>= 0), -1 = "just run" (WRSN.py:290),
 *                              -2 = leave this environment untouched (none of its output rows is written);
 *   action   [B,3] DEVICE double: normalised action, clipped to [0,1] inside (WRSN.py:299).
 * auto_reset != 0: an environment whose previous return was terminal is reset instead of stepped
 * and reports status 3 with the reset request (agent 0, reward 0).
 * agent_id MAY be the same array as out->agent_id, in every launch mode: row e of the inputs is read before row e of the outputs is
 * written, by the one thread block that owns environment e in the launch. */
int wrsn_step(wrsn_t *h, const int32_t *agent_id, const double *action, int32_t auto_reset,
              const wrsn_step_out *out);

/* Bound the work one wrsn_step launch spends on an environment (0, the default: every environment runs its
 * WRSN.step to the end, like the blocking call of the reference).  The duration of a WRSN.step is heavy-tailed (it
 * runs until the next charger finishes: 1 .. several thousand simulated seconds), so in a batch a launch waits for
 * its slowest environment.  With a budget (in work units of roughly 400 shader cycles, counted per simulated second, grid item,
 * service, routing rebuild and packet-exact second; deterministic, not wall-clock) an environment whose step is not finished reports status 4 / agent_id -1
 * and the next wrsn_step goes on with it, ignoring agent_id/action of that row.  Every WRSN.step is still executed
 * in full and returns the same request (agent, time, terminal flag identical; rewards to ~1e-10, because a
 * suspension may split a closed-form jump / a batch of the float32 priority pipeline in two); only the launch it is reported in changes. */
int wrsn_set_step_budget(wrsn_t *h, int32_t work_units);

/* TIME-SLICED launches: a common deadline for the waves of a wrsn_step launch, in microseconds after it started (0, the default:
 * none).  The launch walks the environments in a cyclic order that starts where the previous launch stopped; a wave runs its
 * environment's WRSN.step until it returns or the deadline passes -- then it stops at the next grid-item boundary exactly as if a work
 * budget were used up (status 4 / agent_id -1; the next wrsn_step goes on with it) -- and a wave that would only start when the slice is
 * (nearly) over does not touch its environment at all: the action given for that row is kept in the environment's latch, the row
 * reports status 4 like a step in flight, and the next launches take it up (the caller passes -1 / anything for a status-4 row, as with
 * a step budget; -2 still leaves a row untouched for one call, a reset drops a latched action).  Every environment a launch takes
 * advances by at least one item, a packet-exact second is not begun in the last ~60 us of a slice.  The wave slots stay busy for the
 * whole slice -- with one work cap per environment a quarter of the slot time of a launch is idle while the capped waves finish -- and
 * no launch-order kernels are needed.  The requests are the same as ever (tests: agent, time, terminal identical, rewards to ~1e-9);
 * WHICH launch reports a request depends on timing (the work budget alone is deterministic).  A step budget, if set, still caps what one
 * visit may spend. */
int wrsn_set_step_deadline(wrsn_t *h, int32_t microseconds);

/* WRSN.density_map_to_action (WRSN.py:229-287) with the normalisation of WRSN.step (WRSN.py:293-296), for the
 * `density_map=True` policies of runner/IPPO.py: dmap DEVICE double [B, G, G] (probability map or logits), agent_id
 * DEVICE int32 [B] (< 0: row skipped), action DEVICE double [B, 3] = [x, y, map[argmax] / sum(map >= 99.9th
 * percentile)], ready for wrsn_step.  Arg-max cell, box and third component follow the reference exactly; the
 * charging spot inside the box comes from a deterministic bounded search instead of SciPy's L-BFGS-B (objective value
 * >= the optimiser's; parity of the spot itself is unpinned).  Asynchronous on the handle's stream. */
int wrsn_density_action(wrsn_t *h, const int32_t *agent_id, const double *dmap, double *action);

/* Rollout table accumulated by the step kernel since create (or since the last call with zero_after != 0):
 * dst DEVICE double [B, M + 3] = sum of rewards per charger (the returns IPPO consumes, IPPO.py:80-81), finished
 * episodes, sum of env.now at terminal, completed WRSN.step calls.  Asynchronous on the handle's stream; this is the
 * buffer a data-parallel trainer all-gathers (one collective per rollout, no per-step reduction kernels). */
int wrsn_rollout_table(wrsn_t *h, double *dst, int32_t zero_after);

/* Roll-out bookkeeping of the asynchronous-agent batch: what controller/ippo/IPPO.py:119-156 (and controller/ppo/PPO.py:
 * 115-152) keep in Python lists per environment, for B environments on the device.  All pointers are caller-owned DEVICE
 * memory (torch tensors); the library keeps no roll-out state of its own.
 *   pend_*   : per (environment, charger) the observation the charger last acted on, its raw policy output
 *              (`input_action`: action_elems = 3, or G*G for density-map policies) and the log-probability;
 *   the rest : per charger a list of `capacity` transitions (prev_state, input_action, log-prob, reward, state) plus the
 *              environment index and env.now of every transition; count[m] = transitions appended for charger m so far
 *              (it keeps counting past `capacity`: the excess is dropped, not stored). */
typedef struct wrsn_transition_buffers {
    int32_t capacity, action_elems;
    float   *pend_state;      /* [B, M, 4, G, G]  (this, state and next_state: uint16 bf16 patterns with WRSN_OBS_BF16) */
    float   *pend_action;     /* [B, M, action_elems] */
    float   *pend_logp;       /* [B, M] */
    uint8_t *pend_valid;      /* [B, M]  1: the charger has acted in the running episode */
    float   *state;           /* [M, capacity, 4, G, G]  request["prev_state"]   (IPPO.py:150) */
    float   *action;          /* [M, capacity, action_elems]  request["input_action"] (IPPO.py:151) */
    float   *next_state;      /* [M, capacity, 4, G, G]  request["state"]        (IPPO.py:152) */
    float   *reward;          /* [M, capacity]           request["reward"]       (IPPO.py:153) */
    float   *logp;            /* [M, capacity]           log_probs_pre[agent]    (IPPO.py:154) */
    double  *now;             /* [M, capacity]           env.now at the return */
    int32_t *env;             /* [M, capacity]           environment of the transition */
    int32_t *count;           /* [M] */
} wrsn_transition_buffers;
/* ENTITY ROWS.  The same struct serves wrsn_rollout_record_entities / wrsn_rollout_collect_entities (declared after wrsn_entity_out):
 * a stored state is then one packed float32 row of R = 8 N + 12 M + 8 elements (N = cfg.n_node) -- node [N][8], then mc [M][12], then
 * env [8], as wrsn_entity_out lays them out -- and
 *   pend_state [B, M, R]      state, next_state [M, capacity, R]      float32 whatever wrsn_set_obs_format says, 16-byte aligned;
 * every other member is as above.  Each part is a multiple of 16 bytes, so every row and every part boundary is 16-byte aligned. */

/* The chargers named by agent_id (DEVICE int32 [B], < 0: row skipped) are about to be given `action` (DEVICE float
 * [B, action_elems], the policy's raw output) chosen with log-probability logp (DEVICE float [B]) on observation obs (DEVICE
 * [B,4,G,G] in the handle's observation format): remember them as pending (IPPO.py:141-142).  Call before wrsn_step with the same agent_id. */
int wrsn_rollout_record(wrsn_t *h, const wrsn_transition_buffers *buf, const int32_t *agent_id, const float *action,
                        const float *logp, const float *obs);

/* After wrsn_step / wrsn_reset wrote `out` (every field non-NULL): rows whose WRSN.step completed in that launch and returned a
 * charger with a pending action append one transition to that charger's list (IPPO.py:146-155: a charger that has not acted yet
 * in the episode is skipped); terminal rows and (auto-)reset rows discard what was pending (IPPO.py:144-145); rows the launch left
 * untouched (agent -2 / masked out) or whose step is still in flight (status 4) are skipped -- the library remembers per row what
 * the last environment launch did, so a request is consumed once however often this is called. */
int wrsn_rollout_collect(wrsn_t *h, const wrsn_transition_buffers *buf, const wrsn_step_out *out);

/* Render get_state(agent) for arbitrary agents (DEVICE int32 [B], < 0 = skip) into obs (DEVICE [B,4,G,G] in the handle's
 * observation format, wrsn_set_obs_format). */
int wrsn_render(wrsn_t *h, const int32_t *agent_id, float *obs);

/* ENTITY OBSERVATION: the numbers get_state(agent) rasterises, instead of the 4 x G x G image.  Map 1 of get_state is one separable
 * Gaussian per live node with weight w_n at the node's down-mapped position (WRSN.py:137-147), maps 2..4 are at most M rank-1 terms
 * built from the chargers (WRSN.py:149-185).  With entity buffers registered, every call that renders also writes those terms as
 * float32 rows: per node, per charger and per environment, about 6.6 KB per row at 200 nodes x 3 chargers.
 * With W = xmax - xmin, H = ymax - ymin, a_b2 = alpha / beta^2 and `a` the asking charger of the row:
 *   node n    [0] u = (x - xmin) / W   [1] v = (y - ymin) / H   [2] w_n = (CS / a_b2) / ((E - thr) / (cap - thr))   (WRSN.py:146)
 *             [3] (E - thr) / (cap - thr)   [4] CS / a_b2   [5] RR / a_b2   [6] Node.level as WRSN_PEEK_NODE_LEVEL reports it   [7] 1
 *             a dead node (Node.status == 0) keeps [0], [1] and has 0 in [2..7]; rows n >= n_node of a smaller environment of a
 *             ragged batch are all zero (they are written);
 *   charger o [0], [1] loc, down-mapped   [2] energy / capacity   [3] o == a   [4] status != 0   [5] cur_action_type == "charging"
 *             [6], [7] cur_phy_action x, y, down-mapped   [8] cur_phy_action[2] / charging_time_max
 *             [9] the map-4 amplitude as the reference writes it (WRSN.py:184, mixed index and all):
 *                 euclid(loc_o, (cur_o[0], cur_a[1])) / velocity / moving_time_max; 0 for o == a        [10], [11] 0, reserved
 *   env       [0] hX = charging_range / W   [1] hY = charging_range / H   (bandwidths of maps 1, 3, 4)
 *             [2] 0.5 min(W, H) / W   [3] 0.5 min(W, H) / H   (bandwidths of map 2)   [4] a   [5] n_node   [6], [7] 0
 * Every value is computed in float64 from the fields the render kernel reads and rounded once, to float32, at the store: an image and
 * an entity row written by the same call describe the same instant. */
#define WRSN_ENT_NODE_F 8
#define WRSN_ENT_MC_F  12
#define WRSN_ENT_ENV_F  8
typedef struct wrsn_entity_out {   /* DEVICE, caller-owned, 16-byte aligned, float32 */
    float *node;              /* [B, N, 8]  N = cfg.n_node, node-id order */
    float *mc;                /* [B, M, 12] charger-id order              */
    float *env;               /* [B, 8]                                   */
} wrsn_entity_out;

/* Register (or, with ent == NULL, drop: the default) the entity buffers of the handle.  Once registered, every call that decides which
 * rows to render writes the entity rows of exactly those rows, whether or not out->obs is given: wrsn_reset, wrsn_step in every launch
 * mode (blocking, step budget, two-stage pipeline, time slices), wrsn_load_envs, wrsn_clone_envs (needs out->agent_id, as for obs) and
 * wrsn_pool_reset.  Rows such a call leaves unrendered (terminal, status 4, agent_id -2, masked out, unselected pool rows) are not
 * touched by a single byte.  wrsn_render writes no entity rows.  Independent of wrsn_set_obs_format (always float32) and of
 * wrsn_set_obs_reuse; not part of an environment record; allowed between any two calls, affects the launches enqueued after it.  The
 * memory must stay valid while registered.  A pointer that is NULL or not 16-byte aligned: WRSN_ERR_ARG, handle unchanged. */
int wrsn_set_entity_out(wrsn_t *h, const wrsn_entity_out *ent);

/* Entity rows for arbitrary agents (DEVICE int32 [B], < 0 = skip) into `ent`, like wrsn_render for the image; the registered buffers
 * are neither needed nor touched.  Asynchronous on the handle's stream. */
int wrsn_entities(wrsn_t *h, const int32_t *agent_id, const wrsn_entity_out *ent);

/* Roll-out bookkeeping on ENTITY rows: wrsn_rollout_record / wrsn_rollout_collect with the packed entity row (see
 * wrsn_transition_buffers) in place of the image.  `ent` names the entity buffers the rows are read from; NULL means the buffers
 * registered with wrsn_set_entity_out.  The semantics are those of the image calls, statement for statement: record skips rows with
 * agent_id < 0; collect skips rows the last environment launch left untouched or in flight, discards what is pending for terminal and
 * (auto-)reset rows, appends one transition for a completed WRSN.step whose charger has a pending action; count keeps counting past
 * `capacity` and the excess is not stored; reward is rounded to float32, now and the environment index are stored.
 * out->obs may be NULL (entity-only batches: VecWRSN(render=False, entities=True)).
 * consume != 0: the row's request is consumed, as by wrsn_rollout_collect -- a second collect after the same launch appends nothing.
 * consume == 0: it is left, so that one launch can feed both kinds of buffers: a caller that keeps image AND entity buffers calls
 * wrsn_rollout_collect_entities(consume = 0) FIRST and wrsn_rollout_collect SECOND.
 * WRSN_ERR_ARG, with the handle and every buffer untouched: ent == NULL and nothing registered; node, mc or env NULL or not 16-byte
 * aligned; pend_state, state or next_state NULL or not 16-byte aligned; agent_id, action or logp NULL (record); out->agent_id, reward,
 * terminal, now or status NULL (collect).  Both run on the handle's stream, into which a pipelined step has joined: no extra ordering. */
int wrsn_rollout_record_entities(wrsn_t *h, const wrsn_transition_buffers *buf, const int32_t *agent_id, const float *action,
                                 const float *logp, const wrsn_entity_out *ent);
int wrsn_rollout_collect_entities(wrsn_t *h, const wrsn_transition_buffers *buf, const wrsn_step_out *out,
                                  const wrsn_entity_out *ent, int32_t consume);

/* ACTING FROM ENTITY ROWS.  The actor of build_entity_networks (ippo.py: a set policy over the entity rows, a diagonal Gaussian over
 * the 3-vector action) evaluated and sampled on the device, between the call that wrote the entity rows and
 * wrsn_rollout_record_entities.  `actors` holds one packed float32 block per charger, [n_mc, wrsn_entity_actor_floats()].
 * BLOCK LAYOUT.  Every Linear is stored TRANSPOSED, [in, out] row-major, directly followed by its bias [out], in this order
 * (offsets in floats):
 *     node1    8 ->  64  at     0, bias at   512      node2   64 ->  64  at   576, bias at  4672
 *     mc1     12 ->  32  at  4736, bias at  5120      mc2     32 ->  32  at  5152, bias at  6176
 *     head1  200 -> 128  at  6208, bias at 31808      head2  128 -> 128  at 31936, bias at 48320
 *     mean   128 ->   3  at 48448, bias at 48832      log_std 128 ->  3  at 48835, bias at 49219
 * 49 222 floats, then zeros up to a multiple of 4: wrsn_entity_actor_floats() == 49 224.  The WRSN_ENTPOL_FEAT inputs of head1 are, in
 * this order: the mean of the node embeddings over the alive nodes [64], their maximum [64], the mean of the charger embeddings over
 * the alive chargers [32], the asking charger's own embedding [32], the environment row [8] with slot 4 (the asking charger) scaled by
 * 1 / n_mc and slot 5 (n_node) by 1 / (the handle's node count).  (Stored [in, out], a matrix-core operand W[out = 32 t + (l & 31)]
 * [k = 2 kk + (l >> 5)] of lane l is two runs of 32 consecutive floats.)
 * SEMANTICS.  Row e with a = agent_id[e] in [0, n_mc) is evaluated exactly as EntityActor.forward evaluates it, with block a: a node's
 * eight inputs are replaced by zeros unless its slot 7 (alive) equals 1 -- a select: NaN or inf in a dead or padded node row vanish --;
 * mean and maximum of ReLU(node2(ReLU(node1(x)))) are taken over the alive nodes, the mean divided by max(count, 1), the maximum zero
 * when no node is alive; the charger mean is taken over the chargers whose slot 4 (alive) equals 1, divided by max(count, 1); the own
 * embedding is the sum over the chargers whose slot 3 (is_self) equals 1 -- from the rows themselves, not from agent_id --;
 * (mean, log_std) = the two 3-vectors on ReLU(head2(ReLU(head1(features)))), log_std clamped to [-4, 1].  Then, all in float32,
 *     action[d] = fmaf(exp(log_std[d]), eps[d], mean[d])          logp = sum_d (-eps[d]^2 / 2 - log_std[d]) - 1.5 log(2 pi)
 * with eps == NULL standing for eps = 0 (the mode).  action_f64 holds the same values widened, as wrsn_step takes them.  Rows with
 * agent_id outside [0, n_mc) are skipped: every byte of every output is kept.
 * A row's outputs depend on its own entity rows, its charger's block and its eps only: not on any other row of the batch, not on its
 * position in it, and not on the run -- two calls on equal inputs give equal bytes.  The call needs no scenario: it reads nothing but
 * `ent`, `actors`, `agent_id` and `eps`.
 * WRSN_ERR_ARG, with the handle and every buffer untouched: h, actors, agent_id, out, out->action or out->logp NULL; ent == NULL and
 * nothing registered; node, mc or env NULL or not 16-byte aligned; actors not 16-byte aligned.
 * Asynchronous on the handle's stream, into which a pipelined step has joined.  The first call allocates a scratch of
 * n_env * (WRSN_ENTPOL_FEAT + n_mc) words in the handle; wrsn_destroy frees it. */
#define WRSN_ENTPOL_FEAT 200            /* 64 mean + 64 max + 32 charger mean + 32 own + 8 env */
int32_t wrsn_entity_actor_floats(void); /* floats of one block, a multiple of 4; host only, no handle */

typedef struct wrsn_entity_act_out {    /* DEVICE, caller-owned; written only for the rows that are not skipped */
    float  *action;      /* [B,3] the sample: what wrsn_rollout_record_entities stores */
    double *action_f64;  /* [B,3] the same values widened: what wrsn_step takes; may be NULL */
    float  *logp;        /* [B]   */
    float  *mean;        /* [B,3] may be NULL */
    float  *log_std;     /* [B,3] after the clamp to [-4, 1]; may be NULL */
} wrsn_entity_act_out;

int wrsn_entity_act(wrsn_t *h, const float *actors, const int32_t *agent_id, const float *eps, const wrsn_entity_out *ent,
                    const wrsn_entity_act_out *out);

/* ACTING FROM ENTITY ROWS WITH A NODE POINTER.  The actor of build_entity_pointer_networks (ippo.py) evaluated and sampled on the
 * device: the trunk of the set policy above, a categorical choice of ONE alive node, and a charge head on the chosen node's own
 * features.  The destination is the chosen node's position, so the actor names a node instead of regressing a position from pools,
 * and the third component is a sigmoid raised to at least min_charge, so with min_charge > 0 every decision spends simulated time.
 * `actors` holds one packed float32 block per charger, [n_mc, wrsn_entity_pointer_floats()].
 * BLOCK LAYOUT.  The trunk -- node1, node2, mc1, mc2, head1, head2 -- at the offsets of the block of wrsn_entity_act, 48 448 floats;
 * then, every Linear again TRANSPOSED, [in, out] row-major, directly followed by its bias (offsets in floats):
 *     query  128 ->  64  at 48448, bias at 56640      charge 136 ->   2  at 56704, bias at 56976
 * charge's 136 input rows are z [128] first, then the chosen node's eight features; its outputs are (mean, log_std).  56 978 floats,
 * then zeros up to a multiple of 4: wrsn_entity_pointer_floats() == 56 980.
 * SEMANTICS.  Row e with a = agent_id[e] in [0, n_mc) is evaluated exactly as EntityPointerActor evaluates it, with block a, all in
 * float32.  z = ReLU(head2(ReLU(head1(features)))) as for wrsn_entity_act; q = query(z); h_i = ReLU(node2(ReLU(node1(x_i)))) with x_i
 * the eight inputs of node i (they are used only for alive nodes);
 *     l_i = 0.125 <h_i, q>   for the nodes whose slot 7 (alive) equals 1, -inf for every other -- a select: NaN or inf in a dead or
 *                            padded node row never enter (an alive node whose l_i is not > -inf -- a NaN from weights that are
 *                            not finite -- counts as not alive);
 *     node_logp[i] = l_i - log sum_{j alive} exp(l_j)            (-inf where l_i is)
 *     node = the alive i with the largest l_i + gumbel[e][i], the lowest index among equal scores; a score that is not > -inf
 *            (a NaN) counts as -inf; gumbel == NULL stands for zeros (the mode)
 *     (mean, log_std) = charge([z, x_node]), log_std clamped to [-4, 1];  x = fmaf(exp(log_std), eps[e], mean), eps == NULL: eps = 0
 *     c = min_charge + (1 - min_charge) * (1 / (1 + expf(-x)))
 *     action = (node[node][0], node[node][1], c)        stored = ((float)node, x)
 *     logp = node_logp[node] + (-eps^2 / 2 - log_std - 0.5 log(2 pi))
 * A row with no alive node: node = -1, stored[0] = -1, the node term of logp is 0, x_node is zeros, node_logp is -inf everywhere, and
 * the destination is the asking charger's own position (mc[self][0], mc[self][1]), self being the lowest-index charger row whose slot 3
 * (is_self) equals 1 and row a when there is none: the rule of wrsn_entity_heuristic_act.  No output is a NaN for it.
 * `stored` is what wrsn_rollout_record_entities stores for this policy (action_elems = 2): from it and the stored row, the update
 * recomputes logp.  action_f64 holds `action` widened, as wrsn_step takes it.  Rows with agent_id outside [0, n_mc) are skipped:
 * every byte of every output is kept.
 * A row's outputs depend on its own entity rows, its charger's block, its gumbel row and its eps only: not on any other row of the
 * batch, not on its position in it, and not on the run -- two calls on equal inputs give equal bytes (no float atomics; every sum and
 * every maximum in a fixed order; the bits of l_i do not depend on where node i sits in the row's tiles).  `ent` NULL: the registered
 * buffers.  The call needs no scenario: it reads nothing but `ent`, `actors`, `agent_id`, `gumbel` and `eps`.
 * WRSN_ERR_ARG, with the handle and every buffer untouched: h, actors, agent_id, out, out->node, out->stored, out->action or out->logp
 * NULL; ent == NULL and nothing registered; node, mc or env NULL or not 16-byte aligned; actors not 16-byte aligned; min_charge not
 * finite or outside [0, 1).
 * Asynchronous on the handle's stream, into which a pipelined step has joined.  The scratch -- that of wrsn_entity_act, shared with
 * it, plus n_env * 192 floats for z and q -- lives in the handle, is allocated by the first call and freed by wrsn_destroy. */
int32_t wrsn_entity_pointer_floats(void);            /* 56 980: floats of one block, a multiple of 4; host only, no handle */

typedef struct wrsn_entity_pointer_out {             /* DEVICE, caller-owned; written only for rows that are not skipped */
    int32_t *node;        /* [B]   chosen node, -1: no alive node */
    float   *stored;      /* [B,2] ((float)node, x): what wrsn_rollout_record_entities stores (action_elems = 2) */
    float   *action;      /* [B,3] (u_k, v_k, c) */
    double  *action_f64;  /* [B,3] the same widened; may be NULL */
    float   *logp;        /* [B] */
    float   *node_logp;   /* [B,N] log-softmax over the alive nodes, -inf elsewhere; may be NULL */
    float   *charge_mean, *charge_log_std;   /* [B] each, after the clamp; each may be NULL */
} wrsn_entity_pointer_out;

int wrsn_entity_pointer_act(wrsn_t *h, const float *actors /* [n_mc, floats] */, const int32_t *agent_id,
                            const float *gumbel /* [B,N] or NULL */, const float *eps /* [B] or NULL */,
                            float min_charge, const wrsn_entity_out *ent, const wrsn_entity_pointer_out *out);

/* THE CANDIDATE MASK OF THE NODE POINTER: "not a node another charger serves", the rule of wrsn_entity_heuristic_act below as an
 * opt-in mask on the pointer's choice.  Handle state, WRSN_POINTER_MASK_NONE by default; not part of an environment record.  Allowed
 * between any two calls: it is read when a call enqueues its launches, so the launches enqueued so far keep theirs (as
 * wrsn_set_obs_format).  Read by wrsn_entity_pointer_act, wrsn_entity_pointer_eval, wrsn_entity_pointer_ppo_grad,
 * wrsn_entity_pointer_ppo_grad_multi and wrsn_entity_pointer_ppo_update (once, before its loop), and by the behaviour-cloning calls
 * wrsn_entity_pointer_bc_grad, wrsn_entity_pointer_bc_grad_multi and wrsn_entity_pointer_bc_update (once, before its loop).  With
 * WRSN_POINTER_MASK_NONE every call gives the bytes it gave before the mask existed.
 * WRSN_POINTER_MASK_CLAIMED.  A pure function of the row's content (node, mc, env -- acting rows and stored packed rows alike), in
 * float32, every operation rounded on its own (no contraction into an FMA):
 *     claimer o    : charger row o with mc[o][4] (alive) == 1 and mc[o][3] (is_self) != 1.  No agent_id enters, so the update forms it
 *                    from the stored row alone.  The heuristic excludes `self` (the lowest-index is_self row, else row agent_id)
 *                    instead: the two differ only on rows with no or with several is_self flags -- with none every alive charger
 *                    claims here, with several none of the flagged ones does.
 *     claimed(i)   : for some claimer o,  dx = (node[i][0] - mc[o][6]) / env[0],  dy = (node[i][1] - mc[o][7]) / env[1],
 *                    dx * dx + dy * dy <= 1.  A NaN compares false: it claims nothing.
 *     candidate(i) : alive(i) && !claimed(i) when the row holds at least one such node; else alive(i) -- the heuristic's fallback, so a
 *                    row never loses its last choice.  alive(i) is "l_i > -inf" of the semantics above.
 * "alive" is replaced by "candidate" in exactly two places: the select that writes l_i or -inf -- hence node_logp, the log-sum-exp,
 * the arg-max and the categorical entropy --, and the update's kv = k >= 0 && candidate(k): a stored node that is no candidate
 * contributes no node term to logp, exactly as a stored dead node.  Nothing else moves: the pools behind z run over all alive nodes
 * (a claimed node is still part of the state), x_k is the stored node's eight floats as they stand, a row with no alive node is
 * treated as without the mask, and wrsn_entity_pointer_eval keeps writing the bytes wrsn_entity_pointer_act writes under the same mode.
 * WRSN_ERR_ARG, handle unchanged: h NULL or any other mode. */
#define WRSN_POINTER_MASK_NONE    0
#define WRSN_POINTER_MASK_CLAIMED 1
int wrsn_set_entity_pointer_mask(wrsn_t *h, int32_t mode);

/* A HEURISTIC BASELINE ON THE ENTITY ROWS: "go to the most critical node nobody else is serving".  Deterministic, no parameters but
 * charge_scale; the answer to "better than what?" for a learned entity policy.  For row e with a = agent_id[e] in [0, n_mc), everything
 * in float32, every operation rounded on its own (no contraction into an FMA):
 *   self     the lowest-index charger row whose slot 3 (is_self) equals 1; row a when there is none;
 *   alive    a node whose slot 7 equals 1 -- a select: NaN or inf in a dead or padded node row vanish;
 *   claimed  a node (u, v) for which some charger o != self with slot 4 (alive) == 1 has
 *                dx = (u - mc[o][6]) / env[0],  dy = (v - mc[o][7]) / env[1],  dx * dx + dy * dy <= 1
 *            (the node lies inside the charging disc around that charger's destination; a NaN compares false: not claimed);
 *   pick     among the alive, unclaimed nodes the one with the largest score, the lowest index among equal scores; the score is slot 2
 *            (w_n, the weight of map 1), with anything that is not > -inf (a NaN, -inf) counted as -inf: a NaN never beats a number.
 *            When every alive node is claimed, the same rule over all alive nodes;
 *   action   (u_n, v_n, c) with t = charge_scale * (1 - node[n][3]), c = t > 0 ? (t < 1 ? t : 1) : 0 (selects: a NaN gives 0);
 *            (mc[self][0], mc[self][1], 0) when no node is alive.
 * Node slots 0, 1 and charger slots 0, 1, 6, 7 are positions in the frame wrsn_step maps an action's first two components back from
 * (WRSN.py:95-98), so (u_n, v_n) is the action that sends the charger to node n.  action_f64 holds the same values widened, as
 * wrsn_step takes them.  Rows with agent_id outside [0, n_mc) are skipped: every output byte is kept.  A row's output depends on its
 * own entity rows only; two calls on equal inputs give equal bytes.  `ent` NULL: the registered buffers.  Needs no scenario.
 * WRSN_ERR_ARG, with every buffer untouched: h, agent_id or action NULL; ent == NULL and nothing registered; node, mc or env NULL or
 * not 16-byte aligned.  Asynchronous on the handle's stream. */
int wrsn_entity_heuristic_act(wrsn_t *h, const int32_t *agent_id, const wrsn_entity_out *ent, float charge_scale, float *action,
                              double *action_f64);

/* THE HEURISTIC'S DECISION AS A POINTER LABEL: what wrsn_entity_heuristic_act decides, kept as the node-pointer policy stores a decision
 * (wrsn_entity_pointer_act's `stored`, the [*, 2] pair of EntityTransitionBuffers(action_elems=2)), so that the pointer can be trained on
 * it (wrsn_entity_pointer_bc_grad below).  For row e with a = agent_id[e] in [0, n_mc), in float32, every operation rounded on its own
 * (no contraction into an FMA):
 *     n         = the pick of wrsn_entity_heuristic_act on the row (self, alive, claimed, score, ties and the fallback as stated there)
 *     stored[0] = (float) n;  -1 when no node is alive
 *     c         = the heuristic's charging time: t = charge_scale * (1 - node[n][3]), c = t > 0 ? (t < 1 ? t : 1) : 0
 *     cm        = c > min_charge ? c : min_charge
 *     u         = (cm - min_charge) / (1 - min_charge)
 *     u_lo      = 1 / (1 + expf(x_clip));  u_hi = 1 - u_lo;  u = u < u_lo ? u_lo : (u > u_hi ? u_hi : u)
 *     stored[1] = logf(u / (1 - u))           -x_clip when no node is alive
 * stored[1] is the x for which the pointer's c = min_charge + (1 - min_charge) * sigmoid(x) is the heuristic's c, up to the clamp: it lies
 * in [-x_clip, x_clip] up to rounding, so c == 0, c == 1 and c < min_charge give the ends.
 * action / action_f64, when not NULL, receive THE BYTES wrsn_entity_heuristic_act writes for the row: (u_n, v_n, c) with the heuristic's
 * own c, not the squashed one; (mc[self][0], mc[self][1], 0) when no node is alive.
 * Under WRSN_POINTER_MASK_CLAIMED the label's node is a candidate of the masked pointer on every row that holds exactly one is_self flag
 * (there the mask's claimers are the heuristic's), so the update's kv holds for it; rows with no or several is_self flags are the
 * exception stated with the mask.
 * Rows with agent_id outside [0, n_mc) are skipped: every output byte is kept.  A row's output depends on its own entity rows only; two
 * calls on equal inputs give equal bytes.  `ent` NULL: the registered buffers.  Needs no scenario.  Asynchronous on the handle's stream.
 * WRSN_ERR_ARG, with every buffer untouched: h, agent_id or stored NULL; ent == NULL and nothing registered; node, mc or env NULL or not
 * 16-byte aligned; min_charge not finite or outside [0, 1); x_clip not finite or <= 0. */
int wrsn_entity_heuristic_label(wrsn_t *h, const int32_t *agent_id, const wrsn_entity_out *ent, float charge_scale, float min_charge,
                                float x_clip, float *stored /* [B,2] */, float *action /* [B,3] or NULL */,
                                double *action_f64 /* [B,3] or NULL */);

/* EPISODE LEDGER: whole episodes, per environment, on the device.  wrsn_rollout_table sums over whatever ran; this keeps one entry per
 * finished episode -- lifetime (env.now of the closing return), return and decisions per charger, why it ended, the pool record it ran
 * in -- and tells the caller which rows to restart.  All arrays are caller-owned DEVICE memory; the library keeps no episode state.
 * Call it after every call that wrote `out` (wrsn_step, wrsn_reset, wrsn_pool_reset).  Per row, keyed on what the last environment
 * launch did with it (the row states wrsn_rollout_collect goes by):
 *   untouched / already consumed   nothing is accumulated, next_agent_id[e] keeps its bytes;
 *   step in flight (status 4)      next_agent_id[e] = -1;
 *   reset, auto-reset, pool swap   an episode starts: the running sums of the row are zeroed; next_agent_id[e] = out->agent_id[e];
 *   fresh request                  with a = out->agent_id[e] in [0, n_mc): run_return[e, a] += out->reward[e] (float64, one add) and
 *                                  run_decisions[e, a] += 1.  Then the episode CLOSES with ended = 3 when out->status[e] == 1, else with
 *                                  ended = 2 when time_limit > 0 and out->now[e] >= time_limit; otherwise next_agent_id[e] = a;
 *   terminal return                the episode closes with ended = 1.
 * Closing, with k = finished[e]: k < episodes stores lifetime[k, e] = out->now[e], ep_return[k, e, :], decisions[k, e, :], ended[k, e]
 * and record[k, e]; otherwise dropped[e] += 1.  Then finished[e] = k + 1, the running sums are zeroed, next_agent_id[e] = -2 (the next
 * wrsn_step leaves the row alone) and restart[e] = 1 -- unless quota > 0 and k + 1 >= quota: the row is PARKED, restart[e] = 0.
 * restart[e] is written for every row at every call (0 unless this call closed an episode of a row it did not park): it is the mask
 * for wrsn_reset / wrsn_pool_reset.  A parked row (quota > 0 and finished[e] >= quota at entry) accumulates nothing and gets
 * next_agent_id[e] = -2 at every call, whatever the launch did with it.  An episode that outlives max_time never reports terminal
 * (Network.py:79) and would return at the same instant forever: time_limit closes it.
 * consume != 0: rows with a fresh request, a reset or a terminal return are marked consumed afterwards (a second call after the same
 * launch finds nothing, and so does wrsn_rollout_collect*); consume == 0: they are left, so a training roll-out runs the ledger FIRST
 * and wrsn_rollout_collect_entities SECOND.
 * One thread per environment, no atomics, nothing written outside the stated extents; two calls on equal inputs give equal bytes.
 * Needs no scenario.  next_agent_id and restart may each be NULL; record may be NULL.
 * WRSN_ERR_ARG, with every buffer untouched: h, log or out NULL; run_return, run_decisions, finished, dropped, lifetime, ep_return,
 * decisions or ended NULL; out->agent_id, reward, now or status NULL; episodes < 1; quota < 0 or quota > episodes;
 * next_agent_id == out->agent_id.  Asynchronous on the handle's stream. */
typedef struct wrsn_episode_log {      /* DEVICE, caller-owned */
    int32_t episodes;                  /* E >= 1: finished episodes stored per environment */
    int32_t quota;                     /* 0: never park; 1..E: an environment is parked once it has finished `quota` episodes */
    double  *run_return;               /* [B, M] sum of rewards per charger in the running episode */
    int32_t *run_decisions;            /* [B, M] requests that asked charger m in the running episode */
    int32_t *finished;                 /* [B]    episodes closed since the caller zeroed the log */
    int32_t *dropped;                  /* [B]    of those, the ones with index >= E: counted, not stored */
    double  *lifetime;                 /* [E, B] env.now of the closing return; episode k of environment e at [k, e] */
    double  *ep_return;                /* [E, B, M] */
    int32_t *decisions;                /* [E, B, M] */
    int32_t *ended;                    /* [E, B] 1 terminal return, 2 time limit, 3 fell off the end (status 1) */
    int32_t *record;                   /* [E, B] pool record the episode ran in (WRSN_PEEK_POOL[., 0]); may be NULL */
} wrsn_episode_log;
int wrsn_episodes_collect(wrsn_t *h, const wrsn_episode_log *log, const wrsn_step_out *out, double time_limit,
                          int32_t *next_agent_id, uint8_t *restart, int32_t consume);

/* ONE-STEP LOOKAHEAD OVER THE HEURISTIC: for every request try the heuristic's K best nodes, each on a clone of the environment that is
 * rolled forward under the heuristic for `horizon` simulated seconds, and keep the best.  Two handles: the REAL one (batch B), which is
 * only read, and a SIMULATION handle of K * B environments of the same geometry (auto_reset 0); slot r = k * B + b of every k-major
 * array below is candidate k of real row b, and environment r of the simulation handle.  Per request:
 *     wrsn_lookahead_candidates (real handle)  ->  wrsn_clone_envs_from (src b -> dst k * B + b)  ->  wrsn_step(sim, sim_agent_id, sim_action)
 *     then repeat { wrsn_lookahead_collect (sim) ; wrsn_step(sim, next_agent_id, the heuristic's action for next_agent_id) }
 *     then wrsn_lookahead_collect(close_all = 1) ; wrsn_lookahead_pick (real handle).
 * All state is caller-owned DEVICE memory; all four calls are asynchronous on the handle's stream and read nothing back.
 *
 * wrsn_lookahead_candidates: the heuristic's RANKING, not only its first pick.  For row b with a = agent_id[b] in [0, n_mc), with self,
 * alive, claimed and score as wrsn_entity_heuristic_act states them, float32, every operation rounded on its own: the order is the alive
 * unclaimed nodes by score descending, then index ascending, followed by the alive claimed nodes in the same order; candidate k is its
 * k-th entry (K passes over the row, each leaving out the nodes already taken).  Candidate 0 is the pick of wrsn_entity_heuristic_act.
 * Fewer than K alive nodes: the remaining slots are INVALID.  No alive node: candidate 0 is the heuristic's stand-still action and is
 * valid, the others are invalid.  For slot r = k * B + b:
 *     node[r]         the node; -1 for an invalid slot and for the stand-still action
 *     sim_agent_id[r] a when valid, -2 when not (wrsn_step of the simulation handle then leaves the slot alone)
 *     sim_action[r]   valid slots only: (u_n, v_n, max((double) c, min_charge)), c the heuristic's own charging time for that node -- the
 *                     bytes of wrsn_entity_heuristic_act's action_f64 but for the clamp, which is taken in float64 as
 *                     HeuristicPolicy(min_charge) takes it; ((double) mc[self][0], (double) mc[self][1], min_charge) standing still
 *     stored[r]       valid slots only: the pair wrsn_entity_heuristic_label forms for that node with (float) min_charge and x_clip,
 *                     ((float) n, x); (-1, -x_clip) standing still
 * and the lookahead state of the slot: t0[r] = now[b], t_end[r] = now[b] + horizon, last_now[r] = now[b], ret[r] = 0, died[r] = 0,
 * done[r] = !valid (survived[r] keeps its bytes).  `now` is the real handle's out->now.  Rows with agent_id outside [0, n_mc) are
 * skipped: every output byte and every state element of their K slots is kept.  A row's outputs depend on its own entity rows only;
 * two calls on equal inputs give equal bytes.  K = state->K; state->B must be the handle's batch.  Needs no scenario.
 * WRSN_ERR_ARG, with every buffer untouched: a NULL pointer (ent NULL: the registered buffers, and none registered); K outside
 * [1, WRSN_LOOKAHEAD_MAX_K]; state->B not the batch; an entity buffer not 16-byte aligned, another array not aligned to its element;
 * horizon not finite or <= 0; min_charge not finite or outside [0, 1); x_clip not finite or <= 0.
 *
 * wrsn_lookahead_collect: on the SIMULATION handle after every wrsn_step of it, keyed on what that launch did with the slot exactly as
 * wrsn_episodes_collect is.  Per slot r:
 *   done[r] != 0               next_agent_id[r] = -2, nothing else;
 *   step in flight (status 4)  next_agent_id[r] = -1;
 *   fresh request of charger a ret[r] += out->reward[r] (float64, one add), last_now[r] = out->now[r]; the slot CLOSES when
 *                              out->status[r] == 1 or out->now[r] >= t_end[r]; otherwise next_agent_id[r] = a;
 *   terminal return            died[r] = 1, last_now[r] = out->now[r], and the slot closes; no reward is added, as in the ledger;
 *   untouched, or reset        nothing is written, next_agent_id[r] keeps its bytes.
 * Closing: survived[r] = min(last_now[r], t_end[r]) - t0[r], done[r] = 1, next_agent_id[r] = -2.  close_all != 0 (the call after the last
 * launch): every slot still open after the above is closed the same way, with the last_now it has.  The row state is always consumed
 * (a second call after the same launch finds nothing).  One thread per slot, no atomics, nothing written outside the stated extents.
 * WRSN_ERR_ARG: a NULL pointer; a bad state; K * B of the state is not the handle's batch; out->agent_id, reward, now or status NULL;
 * next_agent_id == out->agent_id.
 *
 * wrsn_lookahead_pick: on the REAL handle.  For each row b with agent_id[b] in [0, n_mc): over the slots k with sim_agent_id[r] >= 0 and
 * done[r] != 0 the lexicographic best by (1) survived descending, (2) ret descending, (3) k ascending; a NaN never beats a number; when
 * no slot qualifies k = 0.  No weight joins the two keys: slots that outlive the horizon have survived = t_end - t0 from the same two
 * doubles for every k of a row, so they tie exactly and ret decides.  Writes choice[b] = k, action_f64[b] = sim_action[r] and action[b]
 * (the same, narrowed) when given, stored[b] = cand_stored[r] when given (ready for the [*, 2] pair of the pointer's transition
 * buffers).  Skipped rows keep every byte.
 * WRSN_ERR_ARG: h, agent_id, sim_agent_id, sim_action or choice NULL; stored without cand_stored; a bad state; state->B not the batch. */
#define WRSN_LOOKAHEAD_MAX_K 8
typedef struct wrsn_lookahead_state {   /* DEVICE, caller-owned; r = k * B + b, B = the REAL handle's batch */
    int32_t K, B;
    double *t0, *t_end, *last_now, *ret, *survived;   /* [K*B] */
    uint8_t *done, *died;                              /* [K*B] */
} wrsn_lookahead_state;
int wrsn_lookahead_candidates(wrsn_t *h, const int32_t *agent_id, const wrsn_entity_out *ent, const double *now /* [B] */,
                              const wrsn_lookahead_state *state, double horizon, float charge_scale, double min_charge, float x_clip,
                              int32_t *node /* [K,B] */, int32_t *sim_agent_id /* [K,B] */, double *sim_action /* [K,B,3] */,
                              float *stored /* [K,B,2] */);
int wrsn_lookahead_collect(wrsn_t *sim_h, const wrsn_lookahead_state *state, const wrsn_step_out *out, int32_t *next_agent_id /* [K*B] */,
                           int32_t close_all);
int wrsn_lookahead_pick(wrsn_t *h, const int32_t *agent_id, const wrsn_lookahead_state *state, const int32_t *sim_agent_id,
                        const double *sim_action, const float *cand_stored /* [K,B,2] or NULL */, int32_t *choice /* [B] */,
                        double *action_f64 /* [B,3] or NULL */, float *action /* [B,3] or NULL */, float *stored /* [B,2] or NULL */);

/* THE PPO UPDATE OF THE ENTITY POLICY.  One minibatch step of PPOLearner.update (ippo.py) for the set networks of build_entity_networks:
 * forward, PPO loss, backward, gradient clipping and Adam as a handful of launches on the handle's stream, nothing read back on the host.
 * None of the three calls needs a scenario: the handle supplies the stream and a scratch area that grows on demand and is freed by
 * wrsn_destroy.  All asynchronous.
 *
 * The CRITIC block: the trunk (node1, node2, mc1, mc2, head1, head2, every Linear [in, out] followed by its bias) at the offsets of the
 * actor block, through head2's bias: 48 448 floats; then value (128 -> 1) [in, out] at 48 448 and its bias at 48 576: 48 577 floats,
 * zeros up to wrsn_entity_critic_floats() == 48 580.
 *
 * ROWS: packed entity rows as the transition buffers store them, R = 8 n_node + 12 n_mc + 8 floats each (node [N][8], mc [M][12], env [8]).
 * Minibatch row i is row index[i] of `rows` (index == NULL: rows 0 .. n - 1; repeats are allowed).  1 <= n_mc <= 8, n_node >= 1, n >= 1.
 *
 * wrsn_entity_eval: EntityActor.forward and EntityCritic.forward on the rows: float32 mean [n,3], log_std [n,3] (after the clamp to
 * [-4, 1]) and value [n].  actor or critic may be NULL; then that net's outputs must be NULL too.  Masks and selects are those of
 * wrsn_entity_act; a row's outputs depend on that row and the block only; for one row content and one block, mean and log_std are
 * bit-equal to what wrsn_entity_act writes.
 *
 * wrsn_entity_ppo_grad: the loss of PPOLearner.minibatch_loss on the n rows and its gradient.  With sigma = exp(log_std), z = (a - mu) / sigma:
 *   newlogp = sum_d(-z^2/2 - log_std_d) - 1.5 log 2 pi, H = sum_d(log_std_d + 1/2 + 1/2 log 2 pi), l = newlogp - logp_old, r = e^l,
 *   approx_kl = mean((r - 1) - l), clipfrac = mean(|r - 1| > clip), A^ = (A - mean A) / (std A + 1e-8) (unbiased std over the n rows) with
 *   norm_adv, else A; pg = mean(max(-A^ r, -A^ clamp(r, 1 - clip, 1 + clip))); v_loss = 1/2 mean(max((v - R)^2, (V + clamp(v - V, -clip,
 *   clip) - R)^2)) with clip_vloss, else 1/2 mean((v - R)^2); loss = pg - ent_coef mean(H) + vf_coef v_loss.
 * batch arrays are float32 and indexed by the same `index` as the rows.  grad_actor [wrsn_entity_actor_floats()] and grad_critic
 * [wrsn_entity_critic_floats()] receive d loss / d block in the block's own layout: overwritten, not accumulated, padding zero.
 * stats: float32 [8] on the device: loss, pg, v_loss, entropy, approx_kl, clipfrac, 0, 0.  Derivatives at the kinks are autograd's: ReLU
 * passes where its output is > 0, a clamp on the closed interval, of two terms under a max the larger (equal terms: their mean), the masked
 * maximum goes to the lowest-index alive node that attains it, nothing flows into the advantages or through the alive / is_self selects.
 * Two calls on equal inputs give equal bytes: every sum has a fixed order, no float atomics.
 *
 * wrsn_entity_adam: clip_grad_norm_ (max_norm) then torch.optim.Adam (no weight decay, no amsgrad) in place on one block of n_floats:
 *   g *= min(1, max_norm / (||g|| + 1e-6)); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).   `grad` itself is left as it is.  norm_out: a device float
 * that receives ||g||, or NULL.
 *
 * WRSN_ERR_ARG, with every buffer untouched: a required pointer NULL (eval: h, rows, rows->rows, one of actor / critic, an output of a net
 * that is given -- at least one; an output of a net that is not given must be NULL); a block, rows->rows or a gradient buffer (adam:
 * param, grad, m, v) not 16-byte aligned; n < 1, or n < 2 with norm_adv; n_mc outside [1, 8]; n_node < 1; n_floats < 1; step < 1. */
int32_t wrsn_entity_critic_floats(void); /* floats of one critic block, a multiple of 4; host only, no handle */

typedef struct wrsn_entity_rows {       /* DEVICE pointers */
    const float *rows;                  /* [*, R] float32, 16-byte aligned */
    const int32_t *index;               /* [n] or NULL */
    int32_t n, n_node, n_mc;
} wrsn_entity_rows;

typedef struct wrsn_ppo_batch {         /* DEVICE, float32, indexed like the rows */
    const float *action;                /* [*, 3] */
    const float *logp_old, *advantage, *ret, *value_old;
} wrsn_ppo_batch;

typedef struct wrsn_ppo_hyper {
    float clip, ent_coef, vf_coef;
    int32_t norm_adv, clip_vloss;
} wrsn_ppo_hyper;

int wrsn_entity_eval(wrsn_t *h, const float *actor, const float *critic, const wrsn_entity_rows *rows, float *mean, float *log_std,
                     float *value);
int wrsn_entity_ppo_grad(wrsn_t *h, const float *actor, const float *critic, const wrsn_entity_rows *rows, const wrsn_ppo_batch *batch,
                         const wrsn_ppo_hyper *hyper, float *grad_actor, float *grad_critic, float *stats);
int wrsn_entity_adam(wrsn_t *h, float *param, const float *grad, float *m, float *v, int32_t n_floats, int32_t step, float lr, float beta1,
                     float beta2, float eps, float max_norm, float *norm_out);

/* ---- the same for the node-pointer policy, one learner per call: EntityPointerActor.forward, EntityCritic.forward and
 * PPOLearner.minibatch_loss of ippo.py, statement for statement, in float32.  `actor` is a pointer block (wrsn_entity_pointer_floats()
 * floats, wrsn_entity_pointer_act's layout), `critic` the block of wrsn_entity_critic_floats() floats, `rows` as above; `stored` [*, 2]
 * holds the decisions as EntityTransitionBuffers(action_elems=2) keeps them, ((float) node, x), indexed like the rows.  Both calls are
 * asynchronous on the handle's stream, need no scenario and use the handle's growing scratch.  For one row with stored (kf, x):
 *   k  = (int) kf when kf is finite and 0 <= k < n_node, else -1 -- a select made before anything is indexed;  kv = k >= 0 and node k is alive
 *   z, q, h_i, l_i, lse, node_logp as under wrsn_entity_pointer_act (-inf for nodes that are not alive);  p_i = exp(l_i - lse)
 *   (mu, s_raw) = charge([z, x_k]), s = clamp(s_raw, -4, 1);  x_k = the eight floats of node row k as they stand (alive or not), zeros for k = -1
 *   t = (x - mu) / exp(s);  logp = (kv ? node_logp[k] : 0) - t^2 / 2 - s - 1/2 log 2 pi
 *   H_cat = -sum_alive p_i (l_i - lse) (0 with no alive node);  entropy = H_cat + s + 1/2 + 1/2 log 2 pi
 * wrsn_entity_pointer_eval writes logp [n], entropy [n], node_logp [n, n_node], charge_mean [n], charge_log_std [n] (after the clamp) and
 * value [n]; any output may be NULL, `actor` or `critic` may be NULL (not both), and the outputs of an absent net must be NULL.  For one row
 * content and one block node_logp, charge_mean and charge_log_std are THE BYTES wrsn_entity_pointer_act writes when stored[0] is that call's
 * node; logp differs from its logp by rounding only (act forms it from its own eps).
 * wrsn_entity_pointer_ppo_grad: loss, statistics, advantage normalisation, value terms and kinks exactly as under wrsn_entity_ppo_grad with
 * this logp and entropy; grad_actor (wrsn_entity_pointer_floats() floats) and grad_critic (wrsn_entity_critic_floats()) are overwritten in
 * block layout, the padding with zeros; stats as there.  Nothing flows into x_k, the advantages or the selects.
 * Two calls on equal inputs give equal bytes; a row's forward outputs depend on that row, its stored pair and the block only.
 * WRSN_ERR_ARG with every buffer untouched: the cases of wrsn_entity_eval / wrsn_entity_ppo_grad carried over, `stored` NULL with an actor, and
 * more nodes than the score block's LDS holds (about 11 000). */
typedef struct wrsn_pointer_batch {      /* DEVICE, float32, indexed like the rows */
    const float *stored;                 /* [*, 2] ((float)node, x), as EntityTransitionBuffers(action_elems=2) keeps it */
    const float *logp_old, *advantage, *ret, *value_old;
} wrsn_pointer_batch;

int wrsn_entity_pointer_eval(wrsn_t *h, const float *actor, const float *critic, const wrsn_entity_rows *rows, const float *stored, float *logp,
                             float *entropy, float *node_logp, float *charge_mean, float *charge_log_std, float *value);
int wrsn_entity_pointer_ppo_grad(wrsn_t *h, const float *actor, const float *critic, const wrsn_entity_rows *rows, const wrsn_pointer_batch *batch,
                                 const wrsn_ppo_hyper *hyper, float *grad_actor, float *grad_critic, float *stats);

/* THE UPDATE OF SEVERAL INDEPENDENT LEARNERS AT ONCE.  The chargers of IPPO share nothing: own nets, own Adam state, own batch.  A GROUP is
 * one (actor, critic) pair with its optimiser state and its data; the three calls below do for G groups (1 <= G <= 8) what the
 * single-group calls above do for one, in the SAME number of launches however large G is (the group is a dimension of every kernel's
 * grid), and run the whole of PPOLearner.update behind one call.  All asynchronous on the handle's stream; none needs a scenario.
 *
 * wrsn_entity_ppo_grad_multi: wrsn_entity_ppo_grad for every group, six launches.  n, n_node, n_mc are common to the groups.  index: DEVICE
 * int32 [G][n], group g's minibatch row i is row index[g * n + i] of ITS rows and batch arrays; NULL: rows 0 .. n - 1 for every group.
 * stats: DEVICE float32 [G][8].  The groups' adam_step and moments are not read (they may be NULL).
 *
 * wrsn_entity_adam_multi: wrsn_entity_adam on the 2 G blocks of the groups, two launches: group g's actor (grad_actor, m_actor, v_actor)
 * and critic (grad_critic, m_critic, v_critic) are stepped at step adam_step + 1, each block clipped by ITS OWN norm (actor and critic
 * separately, as PPOLearner.update clips them).  The bias corrections are formed in double on the host and rounded once, exactly as
 * wrsn_entity_adam forms them.  rows and batch are not read.  The caller advances its step counts.
 *
 * wrsn_entity_ppo_update: `epochs` x ceil(batch_size / minibatch) steps; a step is wrsn_entity_ppo_grad_multi then wrsn_entity_adam_multi.
 * index: DEVICE int32 [G][epochs][batch_size] -- the caller's shuffles; minibatch s of epoch e of group g is entries s * minibatch ..
 * min((s + 1) * minibatch, batch_size) - 1 of index[g][e] (the last one of an epoch may be short).  Step k (counted over epochs and
 * minibatches, from 0) steps group g at adam_step + 1 + k and writes row stats[g][k] of the DEVICE float32 table stats
 * [G][epochs * ceil(batch_size / minibatch)][8].  The host loop only enqueues: nothing is read back, nothing synchronises.  The caller
 * advances its step counts by the number of steps.
 *
 * CONTRACT.  After a multi call, group g's blocks, moments, gradient buffers and statistics hold THE BYTES the single-group calls give
 * on the same inputs in the same order.  They do not depend on G, on the other groups' data or on g's position among the groups.  Two
 * calls on equal inputs give equal bytes (no float atomics, every sum in a fixed order).
 *
 * WRSN_ERR_ARG, with every buffer untouched: every case of the single-group calls, for any group (a required pointer NULL -- of a group:
 * what the call reads or writes; a block, moment, gradient buffer or rows not 16-byte aligned; n < 1; n_mc outside [1, 8]; n_node < 1;
 * adam_step < 0); n_groups outside [1, 8]; two groups naming the same block, moment or gradient buffer; minibatch, epochs or batch_size
 * < 1; norm_adv when any minibatch, the short last one included, has fewer than 2 rows.
 *
 * OUT OF SCOPE: capture of the update as a HIP graph (the launches are simply enqueued); a device-side shuffle or generator (the caller
 * draws the permutations); groups with different n, n_node or n_mc. */
typedef struct wrsn_entity_group {      /* a HOST struct of DEVICE pointers; blocks, moments and gradient buffers 16-byte aligned */
    float *actor, *critic;              /* blocks [wrsn_entity_actor_floats()], [wrsn_entity_critic_floats()]: updated in place by Adam */
    float *m_actor, *v_actor, *m_critic, *v_critic;   /* Adam moments, block layout */
    float *grad_actor, *grad_critic;    /* caller-owned gradient buffers, block layout: overwritten by the gradient, read by Adam */
    const float *rows;                  /* [*, R] packed entity rows, 16-byte aligned */
    wrsn_ppo_batch batch;               /* indexed like the rows */
    int32_t adam_step;                  /* Adam steps taken before the call */
} wrsn_entity_group;

typedef struct wrsn_adam_hyper {
    float lr, beta1, beta2, eps, max_norm;
} wrsn_adam_hyper;

int wrsn_entity_ppo_grad_multi(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                               const int32_t *index, const wrsn_ppo_hyper *hyper, float *stats);
int wrsn_entity_adam_multi(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, const wrsn_adam_hyper *adam);
int wrsn_entity_ppo_update(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n_node, int32_t n_mc, const int32_t *index,
                           int32_t batch_size, int32_t minibatch, int32_t epochs, const wrsn_ppo_hyper *hyper, const wrsn_adam_hyper *adam,
                           float *stats);

/* ---- the same three calls for the node-pointer policy.  They reuse wrsn_entity_group as it stands; for these calls
 *   - actor, m_actor, v_actor and grad_actor hold wrsn_entity_pointer_floats() floats (56 980), critic and its buffers as above;
 *   - batch.action is the [*, 2] stored pair ((float)node, x) of wrsn_pointer_batch, indexed like the rows.
 * The single-group calls they stand for are wrsn_entity_pointer_ppo_grad, and wrsn_entity_adam once on the actor block (56 980 floats)
 * and once on the critic block.  Everything stated above holds with these in place of wrsn_entity_ppo_grad / wrsn_entity_adam:
 *
 * wrsn_entity_pointer_ppo_grad_multi: wrsn_entity_pointer_ppo_grad for every group, ten launches however large G is.  index: DEVICE int32
 * [G][n] or NULL (rows 0 .. n - 1 for every group); stats: DEVICE float32 [G][8].  adam_step and the moments are not read.
 * wrsn_entity_pointer_adam_multi: wrsn_entity_adam on the 2 G blocks, two launches, group g at adam_step + 1, each block clipped by its
 * own norm.  rows and batch are not read.  The caller advances its step counts.
 * wrsn_entity_pointer_ppo_update: `epochs` x ceil(batch_size / minibatch) steps of the two; index: DEVICE int32 [G][epochs][batch_size]
 * (required), stats: DEVICE float32 [G][steps][8]; step k steps group g at adam_step + 1 + k.  The host loop only enqueues on the
 * handle's stream: nothing is read back, nothing synchronises, and the scratch of the largest step is taken before the loop.
 *
 * CONTRACT.  After a multi call, group g's blocks, moments, gradient buffers and statistics row hold THE BYTES the single-group calls
 * give on the same inputs in the same order, whatever G is (1 <= G <= 8), whatever the other groups hold and wherever g stands among
 * them.  Two calls on equal inputs give equal bytes.
 *
 * WRSN_ERR_ARG, with every buffer untouched and everything checked before the first launch: every case listed for the three calls above;
 * norm_adv when any minibatch, the short last one included, has fewer than 2 rows; more nodes than the score block's LDS holds.
 * OUT OF SCOPE, as above: HIP-graph capture, a device-side shuffle, groups of different shape. */
int wrsn_entity_pointer_ppo_grad_multi(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                                       const int32_t *index, const wrsn_ppo_hyper *hyper, float *stats);
int wrsn_entity_pointer_adam_multi(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, const wrsn_adam_hyper *adam);
int wrsn_entity_pointer_ppo_update(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n_node, int32_t n_mc,
                                   const int32_t *index, int32_t batch_size, int32_t minibatch, int32_t epochs, const wrsn_ppo_hyper *hyper,
                                   const wrsn_adam_hyper *adam, float *stats);

/* BEHAVIOUR CLONING OF THE NODE-POINTER ACTOR: supervised training on stored pairs ((float) node, x) -- wrsn_entity_heuristic_label's, or
 * anybody's -- as a warm start that PPO then fine-tunes.  With logp, H, kv and k exactly as wrsn_entity_pointer_eval defines them for a
 * row and its stored pair,
 *     loss = -mean(logp) - ent_coef * mean(H)        over the n rows,
 * so d loss / d logp = -inv_n and d loss / d H = -ent_coef * inv_n with inv_n = 1.f / (float) n.  These are the two floats
 * wrsn_entity_pointer_ppo_grad hands its backward pass when norm_adv = 0, advantage == 1, vf_coef = 0 and logp_old is the logp
 * wrsn_entity_pointer_eval writes (ratio exactly 1, equal terms under the max), and the backward pass is the same kernels: grad_actor
 * holds THE BYTES that call gives under that setting.  No critic is read, written or stepped.
 * stats, float32 [8]: loss; -mean(logp); the node part, -mean over the rows with kv of node_logp[k]; the charge part, -mean over all
 * rows of the Gaussian term -t^2 / 2 - s - 1/2 log 2 pi; mean(H); top-1, the share of the rows with kv whose stored node attains the
 * row's largest node_logp (ties are hits); the share of rows with kv; 0.  The node part and top-1 divide by the number of rows with kv
 * and are 0 when there is none.  Sums in double in a fixed order.
 *
 * wrsn_entity_pointer_bc_grad: one learner; `stored` [*, 2] indexed like the rows; grad_actor (wrsn_entity_pointer_floats() floats) is
 * overwritten in block layout, the padding with zeros.
 * wrsn_entity_pointer_bc_grad_multi: the same for G groups of wrsn_entity_group.  Read of a group: actor, grad_actor, rows and
 * batch.action (the stored pairs).  critic, its moments, grad_critic, batch.logp_old / advantage / ret / value_old may be NULL; where
 * given they keep their bytes.  index: DEVICE int32 [G][n] or NULL; stats: DEVICE float32 [G][8].  7 + 3 G launches: the kernels whose
 * grid carries (group, net) are launched per group on the actor's half.
 * wrsn_entity_pointer_bc_update: `epochs` x ceil(batch_size / minibatch) steps; a step is wrsn_entity_pointer_bc_grad_multi, then the
 * actor half of wrsn_entity_pointer_adam_multi: group g's (actor, grad_actor, m_actor, v_actor) stepped at adam_step + 1 + k, clipped by
 * the actor's own norm, bias corrections formed on the host in double.  index: DEVICE int32 [G][epochs][batch_size] (required); stats:
 * DEVICE float32 [G][steps][8].  The host loop only enqueues: nothing is read back, nothing synchronises, the scratch of the largest step
 * is taken before the loop.  The caller advances its step counts by the number of steps; PPO continues from the same moments.
 * The candidate mask (wrsn_set_entity_pointer_mask) is read when the call enqueues, once before the loop of the update.
 *
 * CONTRACT, as for the multi calls above: group g's block, moments, gradient and statistics hold the bytes the single-group call (and
 * wrsn_entity_adam on the actor block) gives, whatever G is, whatever the other groups hold and wherever g stands.  Two calls on equal
 * inputs give equal bytes.
 * WRSN_ERR_ARG, everything checked before the first launch and every buffer untouched: h NULL; a pointer the call reads or writes NULL
 * (actor, grad_actor, rows, the stored pairs, stats; for the update m_actor, v_actor, index, adam); a block, moment, gradient buffer or
 * rows not 16-byte aligned; n, batch_size, minibatch or epochs < 1; n_mc outside [1, 8]; n_node < 1 or more than the score block's LDS
 * holds; n_groups outside [1, 8]; adam_step < 0; two groups naming the same actor block, moment or gradient buffer; ent_coef not finite.
 * OUT OF SCOPE: per-row loss weights, a device-side shuffle, HIP-graph capture, imitation for the Gaussian set policy. */
int wrsn_entity_pointer_bc_grad(wrsn_t *h, const float *actor, const wrsn_entity_rows *rows, const float *stored, float ent_coef,
                                float *grad_actor, float *stats);
int wrsn_entity_pointer_bc_grad_multi(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                                      const int32_t *index, float ent_coef, float *stats);
int wrsn_entity_pointer_bc_update(wrsn_t *h, const wrsn_entity_group *groups, int32_t n_groups, int32_t n_node, int32_t n_mc,
                                  const int32_t *index, int32_t batch_size, int32_t minibatch, int32_t epochs, float ent_coef,
                                  const wrsn_adam_hyper *adam, float *stats);

/* THE PPO BATCH OF SEVERAL LEARNERS, PREPARED ON THE DEVICE: the critic's values of the selected transitions, PPOLearner.cal_rt_adv
 * (gae=True) over them and the gathers of the batch tensors, for G groups (1 <= G <= 8) in three launches however large G and n are.
 * Asynchronous on the handle's stream, needs no scenario, reads nothing back.
 *
 * For group g and position i let s = index[g * n + i] (index: DEVICE int32 [G][n], repeats allowed; NULL: s = i).
 *   value[i]      the critic's value of state[s]: THE BYTES wrsn_entity_eval writes for that row and block.  The value of next_state[s]
 *                 ("next_value") lives in the handle's scratch area only.
 *   advantage, ret  the reference's recurrence in float32 -- every operation rounded to float32, none contracted into an FMA:
 *                     g = (float)gamma;  c = (float)((double)gamma * (double)gae_lambda);                  formed on the host
 *                     last = 0;  for t = n - 1 .. 0:   tm = terminal ? terminal[s_t] : 0
 *                         delta = (reward[s_t] + (g * next_value[t]) * tm) - value[t];
 *                         last  = delta + ((c * tm) * last);
 *                         advantage[t] = last;   ret[t] = advantage[t] + value[t];
 *                 `terminal` is the reference's FACTOR on the bootstrap term (IPPO.py:71-93), not a done flag.  Non-finite values go
 *                 through the recurrence as they are (0 * inf is NaN): there is no shortcut on tm == 0.
 *   out_state[i] = state[s], out_next_state[i] = next_state[s], out_action[i] = action[s], out_logp[i] = logp[s],
 *   out_reward[i] = reward[s]: plain copies; each output may be NULL (nothing is written for it).
 *
 * CONTRACT.  A group's outputs depend on that group's inputs only: not on G, on the other groups' data or on the group's position.  Two
 * calls on equal inputs give equal bytes.  Nothing outside the stated extents is written.
 *
 * WRSN_ERR_ARG, with every buffer untouched (checked before the first launch): h or groups NULL; n_groups outside [1, 8]; n < 1;
 * n_node < 1; n_mc outside [1, 8]; critic, state, next_state, reward, value, advantage or ret of a group NULL; an output given whose
 * source is NULL (out_action without action, out_logp without logp); critic, state, next_state, out_state or out_next_state not 16-byte
 * aligned; two groups naming the same output buffer; gamma or gae_lambda not finite.
 *
 * OUT OF SCOPE: the batch selection (the caller's: it uploads the index); groups with different n, n_node or n_mc; the gae=False branch. */
typedef struct wrsn_prepare_group {      /* a HOST struct of DEVICE pointers */
    const float *critic;                 /* critic block [wrsn_entity_critic_floats()], 16-byte aligned */
    const float *state, *next_state;     /* [*, R] packed entity rows, 16-byte aligned (a charger's slice of the transition buffers) */
    const float *reward;                 /* [*] */
    const float *terminal;               /* [*] the reference's factor on the bootstrap term, or NULL = all 0 */
    const float *action, *logp;          /* [*, 3], [*]; each may be NULL, then its output must be NULL */
    float *value, *advantage, *ret;      /* [n] required outputs, in selection order */
    float *out_state, *out_next_state;   /* [n, R] gathered rows, 16-byte aligned; each may be NULL */
    float *out_action, *out_logp, *out_reward;   /* [n, 3], [n], [n]; each may be NULL */
} wrsn_prepare_group;

int wrsn_entity_prepare(wrsn_t *h, const wrsn_prepare_group *groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                        const int32_t *index /* DEVICE [G][n] or NULL = rows 0..n-1 */, float gamma, float gae_lambda);

/* Copy internal state to HOST memory (parity tests, `net` / `agents` views).  Synchronises. */
int wrsn_peek(wrsn_t *h, int32_t what, void *dst);

/* Observation reuse.  Map 1 of get_state (WRSN.py:137-147) depends on node state only, maps 2..4 on the asking charger.  With
 * on != 0 the caller promises that an `obs` row the library wrote keeps its content until the library writes it again (same buffer
 * passed call after call, never modified, never re-allocated at the same address with other content); the render pass then leaves map 1
 * of a row alone when no simulated second has passed since it rendered that row at that address (a WRSN.step that returns at the
 * instant it was called) and writes only maps 2..4.  Results are bit-identical; default off. */
int wrsn_set_obs_reuse(wrsn_t *h, int32_t on);

/* Observation format of the handle; default WRSN_OBS_F32.  With WRSN_OBS_BF16 every observation the library writes or copies
 * holds bfloat16 bit patterns, uint16 [.,4,G,G], half the bytes: wrsn_step_out.obs of wrsn_reset, wrsn_step (every launch mode),
 * wrsn_load_envs and wrsn_clone_envs; the obs of wrsn_render and wrsn_rollout_record; pend_state, state and next_state of
 * wrsn_transition_buffers (actions, log-probabilities and rewards stay float32).  The declared pointer types stay `float *`: the
 * pointee type follows the handle's format.  A buffer for B rows is B*4*G*G*2 bytes and no byte beyond it is touched; rows the
 * float32 format leaves untouched stay untouched.  Every cell is the float32 value of the float32 format rounded to nearest even
 * (bit for bit; on the device a float32 subnormal may become a zero of its sign).  Rows of 4-column groups are written with 8-byte
 * stores when map_size is a multiple of 4, with 2-byte stores otherwise.  Allowed between any two calls; affects the launches
 * enqueued after it.  Map-1 reuse (wrsn_set_obs_reuse) does not carry over a change of format at the same address.  Environment
 * records do not depend on the format.  Any other value: WRSN_ERR_ARG, handle unchanged. */
enum wrsn_obs_format { WRSN_OBS_F32 = 0, WRSN_OBS_BF16 = 1 };
int wrsn_set_obs_format(wrsn_t *h, int32_t format);

/* Per-kernel timing of the step path with HIP events recorded on the handle's stream (the stream the kernels are launched on).
 * wrsn_set_timing(h, 1) makes every following wrsn_step record four events; wrsn_kernel_times waits for the last call and
 * returns, in milliseconds: ms[0] launch-order kernels (work estimate + sort), ms[1] step kernel, ms[2] always 0 (the continuation
 * launch it timed no longer exists; the slot stays for the callers that add it to ms[1]), ms[3] observation kernel plus, with entity
 * buffers registered (wrsn_set_entity_out), the entity launch behind it (0 when the call rendered neither).  Measurement only. */
int wrsn_set_timing(wrsn_t *h, int32_t on);
int wrsn_kernel_times(wrsn_t *h, float *ms);

/* Wait for the handle's stream. */
int wrsn_sync(wrsn_t *h);

/* ENVIRONMENT RECORDS: save, load and clone running environments.  A record is the whole state of one environment -- scenario
 * constants, topology, the live state and the post-warm-up snapshot reset() restores (WrsnEnvDyn: a step in flight, a latched
 * action, terminal_pending), the MT19937 generator when the handle keeps one -- plus the row's pending request, behind a header
 * (magic, format version, struct sizes, NP, TP, ECAP, CCAP, M, n_node, n_target, conn_bound, generator block).  After a load or a
 * clone a destination behaves exactly as the source would have: bit-identical requests in blocking mode, the launch-mode contract
 * with a step budget, the pipeline or time slices.  Not carried over: the destination keeps its counters since create (n_steps,
 * wrsn_counters [3..5], the rollout table) and its diagnostic counters; map 1 reuse starts afresh (wrsn_set_obs_reuse); a following
 * wrsn_rollout_collect appends nothing for a replaced row.
 * Index arrays are HOST int32 [n], checked on the host (in range; saved / cloned-from environments hold a scenario; load and clone
 * destinations distinct; no clone destination is also a source).  Records and request rows are DEVICE memory (16-byte aligned). */

/* Bytes of one record of this handle (a multiple of 256; about 220 KB at 200 nodes with the default capacities). */
int wrsn_env_record_bytes(wrsn_t *h, int64_t *bytes);

/* Write n records, record i = environment env[i] with its pending request (req->agent_id, reward, terminal, now, status
 * non-NULL; obs ignored), into dst [n, record bytes].  Asynchronous on the handle's stream. */
int wrsn_save_envs(wrsn_t *h, const int32_t *env, int32_t n, const wrsn_step_out *req, void *dst);

/* Replace environment env[i] by record i of src (n records back to back) and write its saved request into row env[i] of out (NULL
 * fields are skipped; with out->obs, rows with agent_id >= 0 are rendered, the others left untouched).  Validates every header
 * first and changes nothing when one does not fit (WRSN_ERR_ARG naming the field).  A record fits a handle with equal NP, TP, ECAP,
 * CCAP and M, n_node <= N and n_target <= T; map_size, B and the device may differ.  A record with a generator block loads only
 * into a handle that keeps generators or holds no scenario yet (which then gets them, and runs the stochastic kernels when a loaded
 * prob_gp != 1); one without only into a handle without generators.  Synchronous, like wrsn_set_scenario. */
int wrsn_load_envs(wrsn_t *h, const int32_t *env, int32_t n, const void *src, const wrsn_step_out *out);

/* dst[i] becomes a copy of src[i] (device to device), and row src[i] of out is copied to row dst[i] (obs rendered as for a load;
 * needs out->agent_id then).  Asynchronous on the handle's stream. */
int wrsn_clone_envs(wrsn_t *h, const int32_t *src, const int32_t *dst, int32_t n, const wrsn_step_out *out);

/* The clone ACROSS TWO HANDLES: environment dst[i] of dst_h becomes a copy of environment src[i] of src_h, and row src[i] of src_req (the
 * source's request rows: agent_id, reward, terminal, now and status non-NULL, obs ignored) is copied to row dst[i] of dst_out (NULL fields
 * are skipped).  Everything else is the contract of wrsn_clone_envs: what is carried and what is not (the destination keeps its counters
 * since create, map 1 reuse starts afresh, a following collect finds nothing for the row), and the cloned rows are rendered -- dst_out->obs
 * when set, the destination's registered entity rows -- which needs dst_out->agent_id.  The pool record of a destination (WRSN_PEEK_POOL)
 * becomes -1, as after a load: a pool belongs to its handle.  `src` may repeat (fan-out: one source, many destinations); `dst` entries
 * are distinct; both are HOST int32 [n].  The source handle is only read: no byte of its environments or request rows changes.
 * Asynchronous on the handles' common stream, no host read; when the source's connected-node bound or stochastic kernels ask for a new
 * launch configuration of the destination (never between handles created on the same scenarios) that one call synchronises first.
 * Mechanism: the distinct sources are packed into records in an area the destination owns and unpacked from there, so a call moves
 * 2 * (u + n) record sizes for u distinct sources and n pairs.
 * WRSN_ERR_ARG with a message, nothing changed: a NULL pointer or n < 1; the two handles are one; different devices; different streams;
 * NP, TP, ECAP, CCAP or M differ; the source handle's n_node or n_target is larger than the destination's; one handle keeps generators
 * and the other does not; an index out of range; a source that holds no scenario; a destination twice. */
int wrsn_clone_envs_from(wrsn_t *dst_h, wrsn_t *src_h, const int32_t *src, const int32_t *dst, int32_t n,
                         const wrsn_step_out *src_req, const wrsn_step_out *dst_out);

/* SCENARIO POOLS: restart finished episodes in another network, on the device.  A record saved right after wrsn_reset is a prepared
 * scenario (topology, constants, post-warm-up snapshot, reset request); a pool is P of them.
 *
 * wrsn_pool_set registers P records (DEVICE, caller-owned, 16-byte aligned, back to back at this handle's record size) as the handle's
 * pool.  The memory must stay valid and unchanged until the pool is replaced, cleared (records == NULL, n_records == 0) or the handle
 * destroyed.  Every header is validated as by wrsn_load_envs (WRSN_ERR_ARG naming record and field, nothing changed), the generator
 * block rule of wrsn_load_envs applies to the pool as a whole, and the launch configuration is fitted to the pool's largest
 * conn_bound (and to prob_gp != 1 anywhere in it) once, so that no later swap needs a new one.  Zeroes the per-environment swap
 * counters (WRSN_PEEK_POOL).  `seed` seeds the draw below.  Synchronous. */
int wrsn_pool_set(wrsn_t *h, const void *records, int32_t n_records, uint64_t seed);

/* Replace the environments the DEVICE selects by pool records, asynchronously on the handle's stream (no host synchronisation, no
 * host read-back).
 *   env_mask   DEVICE uint8 [B]: rows with a non-zero byte are selected.  NULL: exactly the rows whose last return was terminal, the
 *              rows an auto-reset of the next wrsn_step would take.
 *   pool_index DEVICE int32 [B]: the record for row e, read for selected rows only.  NULL: the handle draws it -- for environment e
 *              with k swaps since wrsn_pool_set:  z = (seed ^ ((uint64)e << 32 | k)) + 0x9E3779B97F4A7C15;
 *              z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31;
 *              index = ((z >> 32) * P) >> 32   (mod 2^64).  Every swap of e increments k, whoever chose the index.
 *   agent_id   NULL, or DEVICE int32 [B], in/out: selected rows are set to -2, so that the wrsn_step the caller issues next with this
 *              array leaves them alone in every launch mode and their rows of `out` carry the request below out of that call.
 *              It must NOT be the same array as out->agent_id (WRSN_ERR_ARG): that row receives the record's charger.
 * A selected row becomes what wrsn_load_envs of that record into that row would make it (the destination keeps its counters since
 * create and the rollout table; a step in flight or a latched action of the old occupant is gone; the generator block is replaced
 * when the handle keeps generators).  Its row of `out` gets the record's saved request (agent_id, reward, now, terminal), status 3
 * when env_mask is NULL (as an auto-reset reports) and 0 with a mask (as wrsn_reset reports); with out->obs (needs out->agent_id) the
 * row is rendered in the handle's observation format.  A following wrsn_rollout_collect discards what was pending for the row, as
 * after a reset.  No byte of state, request row or observation of an unselected row is touched.  A selected row whose pool_index is
 * outside [0, n_records) is left as it was (agent_id too) and gets status WRSN_STATUS_POOL_INDEX.
 * WRSN_ERR_STATE: no pool set; an environment of the handle holds no scenario yet (the host cannot know which rows the device
 * replaces, so every one must be filled); the handle's record layout changed since wrsn_pool_set. */
int wrsn_pool_reset(wrsn_t *h, const uint8_t *env_mask, const int32_t *pool_index, int32_t *agent_id, const wrsn_step_out *out);

/* Device counters, summed over the environments.  HOST pointer to 8 x int64.  Synchronises.
 *   [0] simulated seconds, [1] packet-exact seconds, [2] charger events of the episodes in progress (they restart at
 *       every reset: the warm-up is part of them);
 *   [3] completed WRSN.step calls since create;
 *   [4] simulated seconds executed inside WRSN.step calls since create (warm-up excluded, never reset);
 *   [5] completed WRSN.step calls since create that returned at the instant they were called (the bookkeeping returns
 *       at t = warm_up_time, SURVEY.md A.4, and same-instant completions);  [6], [7] reserved (0). */
int wrsn_counters(wrsn_t *h, int64_t *dst);

/* Seeded synthetic network generator (host code): fills HOST arrays
 * node_xy [n_node,2], target_xy [n_target,2], bs_xy [2].  side <= 0 selects
 * 1000 * max(1, sqrt(n_node / 200)) metres. */
int wrsn_synth_network(uint64_t seed, int32_t n_node, int32_t n_target, double side,
                       double com_range, double sen_range,
                       double *node_xy, double *target_xy, double *bs_xy);

const char *wrsn_last_error(void);
const char *wrsn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WRSN_HIP_H */
