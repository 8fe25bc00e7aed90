/* include/pgtg.h -- C ABI of the MI355X-native batched PGTG environment (libpgtg_hip.so).
 *
 * The reference (Inuri04/pgtg) has no FFI: its hot path sits behind the Gymnasium Env API of
 * `PGTGEnv` (pgtg/environment.py:297-1281, registered as "pgtg-v4" in pgtg/__init__.py:7).  Each
 * entry point below replaces one piece of that surface for a BATCH of independent environments
 * resident in HBM; the Python facade in pgtg_amd/ (PGTGEnv, PGTGVecEnv) binds it with ctypes.
 *
 *   pgtg_create       <- PGTGEnv.__init__(map_path, **kwargs)          environment.py:302-515
 *   pgtg_reset        <- PGTGEnv.reset(seed=...)                        environment.py:581-656
 *   pgtg_step         <- PGTGEnv.step(action) + same-step auto-reset    environment.py:1092-1281
 *   pgtg_set_outputs  <- the obs/reward/terminated/truncated/info return values (device buffers)
 *   pgtg_get_cars / pgtg_get_env_state <- get_info() fields             environment.py:1538-1578
 *   pgtg_set_agent / pgtg_add_car      <- test-style state overrides (env.position = ..., env.cars.append)
 *   pgtg_get_map_plan <- EpisodeMap.map_plan / save_map                 pgtg/map.py:173-184
 *   pgtg_get_squares  <- EpisodeMap.squares feature sets (feature_at)   pgtg/map.py:49-69, parser.py:13-166
 *   pgtg_get_counters <- (new) device-side env-step / episode counters
 *   pgtg_set_episode_stats / pgtg_episode_summary <- (new, no reference function) the VecMonitor
 *                        wrapper the reference's caller puts around the vector env  pgtg/train.py:55
 *   pgtg_gae          <- (new, no reference function) RolloutBuffer.compute_returns_and_advantage of the
 *                        PPO the reference's caller trains                 pgtg/train.py:61-74
 *   pgtg_set_flat_cost / pgtg_cost_scan <- info["cost"] of separate_reward_cost through the rollout, and
 *                        a Lagrange multiplier on it (new past the step)  environment.py:1130-1276
 *   pgtg_reward_norm  <- (new, no reference function) the reward half of the VecNormalize an SB3 user
 *                        wraps the env in, for rewards the size of train.py's   pgtg/train.py:21-38
 *   pgtg_policy / pgtg_policy_pack <- (new, no reference function) the acting forward pass of the
 *                        MlpPolicy that PPO collects with                  pgtg/train.py:61-74
 *   pgtg_eval_step / pgtg_eval_summary <- ModularEvaluator.evaluate for the batch, with the per-env
 *                        episode quotas of SB3's evaluate_policy           pgtg/evaluator.py:284-339
 *   pgtg_flatten      <- (new, test-oriented) the FlattenObservation kernel alone, over the bound outputs
 *   pgtg_snapshot_*   <- copy.deepcopy(env) / env.clone() for single envs of the batch, on the device
 *                        environment.py:1283-1299, pgtg/evaluator.py:98-110
 *
 * Conventions: all pointers named *_dev are device pointers (hipMalloc'd or torch data_ptr) on the
 * handle's device; everything else is host memory.  Calls on one handle are serialised by the
 * caller and enqueued on the handle's HIP stream (pgtg_set_stream); they do not synchronise unless
 * documented.  Every entry point returns PGTG_OK (0) or a negative PGTG_E_* code; the message is
 * available from pgtg_last_error(handle).
 */
#ifndef PGTG_H_
#define PGTG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGTG_ABI_VERSION 9

/* status codes (Python facade maps them to the reference's exception types) */
#define PGTG_OK 0
#define PGTG_E_INVALID -1      /* invalid configuration / argument  -> ValueError            */
#define PGTG_E_DONE -2         /* step on a finished env (no auto-reset) -> RuntimeError       */
#define PGTG_E_DEVICE -3       /* HIP runtime error                  -> RuntimeError           */
#define PGTG_E_UNSUPPORTED -4  /* outside this build's limits        -> ValueError             */
#define PGTG_E_MAP -5          /* map without route / no start square / empty route choice      */

/* limits of this build */
#define PGTG_MAX_TILES 256     /* width*height of the tile map (16 x 16; traffic: squares <= 255 per side) */
#define PGTG_MAX_CHANNELS 128  /* observation keys: distinct feature names (the vocabulary has 51; unknown names give zero channels) */
#define PGTG_MAX_RULES 8       /* traffic rules: the triggered-rule mask output is one byte per env */
#define PGTG_MAX_WINDOW 31     /* observation window side (9 fixed, 2*s+1 sliding, s <= 15) */

/* observation channel codes (one per key of the reference's obs["map"] dict) */
enum {
  PGTG_CH_ZERO = 0,        /* names that never occur on a square: all zeros */
  PGTG_CH_WALL = 1,        /* "walls" / "wall" */
  PGTG_CH_GOALS = 2,       /* "goals": subgoal or final goal */
  PGTG_CH_TRAFFIC = 3,     /* "traffic": a car on the square */
  PGTG_CH_TL_GREEN = 4,    /* "traffic_light" key -> traffic_light_{green,yellow,red} */
  PGTG_CH_TL_YELLOW = 5,
  PGTG_CH_TL_RED = 6,
  PGTG_CH_START = 7,
  PGTG_CH_SUBGOAL = 8,
  PGTG_CH_USED_SUBGOAL = 9,
  PGTG_CH_FINAL_GOAL = 10,
  PGTG_CH_ICE = 11,
  PGTG_CH_BROKEN = 12,
  PGTG_CH_SAND = 13,
  PGTG_CH_SPAWNER = 14,
  PGTG_CH_LANE0 = 32       /* + lane id 0..31, "car_lane <route> <type>" in sorted order */
};

typedef struct {
  int32_t tile_exits;       /* rule tile_type "NESW" bits as mask (bit0 north); -1 = never */
  int32_t speed_sq_min;     /* admissible vx^2+vy^2 interval for velocity_range (fp64 sqrt) */
  int32_t speed_sq_max;
  int32_t min_traffic;
  int32_t min_matching_traffic;
  /* weight[d][r]: maneuvers with agent direction d listing route r;
   * d: 0 south_to_north 1 west_to_east 2 north_to_south 3 east_to_west 4 stationary 5 near_goal */
  uint8_t weight[6][20];
} PgtgRule;

/* Raw constructor kwargs (pgtg/environment.py:302-359) plus the fixed map of map_path. */
typedef struct {
  int32_t abi_version;                 /* = PGTG_ABI_VERSION */
  int32_t width, height;               /* random_map_width / random_map_height */
  double pct_connections;              /* random_map_percentage_of_connections */
  int32_t start_mode, goal_mode;       /* 0 (x,y,dir)  1 (x,y)  2 "random" */
  int32_t start_x, start_y, start_dir; /* dir: 0 north 1 east 2 south 3 west; x/y may be -1 */
  int32_t goal_x, goal_y, goal_dir;
  int32_t min_distance;                /* random_map_minimum_distance_between_start_and_goal, -1 None */
  double obstacle_probability;
  double w_ice, w_broken, w_sand, w_tl;
  int32_t n_channels;
  int32_t channels[PGTG_MAX_CHANNELS];
  int32_t sliding, sliding_size, next_subgoal;
  double sum_subgoals_reward, final_goal_bonus, crash_penalty, tl_violation_penalty;
  double standing_still_penalty, visited_penalty;
  double ice_probability, street_damage_probability, sand_probability, traffic_density;
  int32_t phase_dur[3];
  int32_t ignore_traffic_collisions;
  double profile_pct[5];               /* conservative, normal, aggressive, elderly, reckless */
  int32_t separate_reward_cost;
  int32_t n_rules;
  PgtgRule rules[PGTG_MAX_RULES];
  /* fixed map (map_path): tiles row-major [y*w+x] */
  int32_t fixed_map, fm_w, fm_h;
  uint8_t fm_exits[PGTG_MAX_TILES];
  int8_t fm_obst_type[PGTG_MAX_TILES]; /* -1 none, 0 ice 1 broken road 2 sand 3 traffic_light */
  int8_t fm_obst_mask[PGTG_MAX_TILES]; /* -1 none, 0..13 (tools/gen_tables.py order) */
  int32_t fm_start[3], fm_goal[3];
  /* vector-env options (no reference equivalent; pgtg/train.py:21-41 wraps with TimeLimit) */
  int32_t autoreset;                   /* 1: same-step auto-reset (gymnasium/SB3 vector semantics) */
  int32_t max_episode_steps;           /* TimeLimit truncation, 0 = none */
  int32_t min_car_capacity;            /* car slots per env for pgtg_add_car (tests), 0 = from density */
  /* launch-shape overrides for tests and A/B runs (0 = automatic; the library reads no environment) */
  int32_t tune_envs_per_block;         /* 16, 32, 64, 128 or 256 env lanes per step workgroup */
  int32_t tune_obs_sub;                /* envs per observation sub-batch */
  int32_t tune_kt_grid, tune_kt_cap, tune_kt_wpc; /* k_traffic grid, envs per wave, workgroups per CU */
  int32_t tune_car_slots;              /* car slots per env (>= 3 x capacity + 4; tests of the bound) */
  int32_t tune_kt_serial;              /* 1: initial traffic's per-car draws on one lane per env (the
                                          rejection fallback of the lane-parallel path; tests) */
  int32_t tune_queue_mode;             /* map-queue step kernel: 0 automatic (k_envb for grids of <= 2 rounds
                                          of workgroups, else k_envq), 1 k_envq, 2 k_envb */
  int32_t tune_fault;                  /* tests of the error paths: bit 0 clears the path walk's north
                                          mask on maps whose tile 0 keeps its east exit (inconsistent masks ->
                                          PGTG_E_DEVICE for those envs, the launch finishes) */
  int32_t tune_step_ticks;             /* pgtg_step_many on a k_envq handle: ticks per launch at most (0: 64,
                                          1 a launch per tick) */
  int32_t tune_queue_grid;             /* k_envq's persistent grid at most (tests: more rounds of blocks per
                                          workgroup at small batches) */
} PgtgConfig;

/* Output buffers (device pointers, caller-owned, contiguous).  NULL = not produced. */
typedef struct {
  uint8_t* obs;            /* [N][n_channels][win][win] uint8 one-hot ([c][x][y] like the reference) */
  int32_t* position;       /* [N][2] */
  int32_t* velocity;       /* [N][2] */
  int32_t* next_subgoal;   /* [N] (use_next_subgoal_direction) */
  double* reward;          /* [N] */
  double* cost;            /* [N] (separate_reward_cost) */
  uint8_t* terminated;     /* [N] */
  uint8_t* truncated;      /* [N] */
  uint8_t* final_obs;      /* [N][n_channels][win][win]: terminal observation of envs reset this step */
  int32_t* final_position; /* [N][2] */
  int32_t* final_velocity; /* [N][2] */
  int32_t* final_next_subgoal; /* [N] */
  uint8_t* braking;        /* [N] triggered traffic rules, bit r = PgtgConfig.rules[r] (rule_triggers);
                              nonzero <=> info['traffic_rules']['braking_applied'] */
} PgtgOutputs;

typedef struct {
  int32_t x, y, vx, vy;
  int32_t terminated, flat_tire, phase, elapsed;
  int32_t n_cars, next_car_id, path_len, error;
  uint32_t spawn_counter;
  uint64_t seed;
  uint64_t used_subgoals[4];           /* bit t%64 of word t/64: tile t's subgoal used (all 256 tiles) */
  int32_t n_spawners, car_tail;        /* car slots in use (cars + empty slots before the last car) */
} PgtgEnvState;

typedef struct {
  int32_t id, x, y, route, profile, patience, delay;
} PgtgCar;

/* Episodes finished in a window, over the batch (pgtg_episode_summary). */
typedef struct {
  uint64_t episodes, truncated_only, length_sum;
  int32_t  length_min, length_max;      /* INT32_MAX / 0 when episodes == 0 */
  double   return_sum;                  /* fp64 sum of the episodes' float32 returns */
  float    return_min, return_max;      /* +INFINITY / -INFINITY when episodes == 0 */
} PgtgEpisodeSummary;

typedef struct pgtg_handle pgtg_handle;

int pgtg_create(const PgtgConfig* cfg, uint64_t n_envs, int32_t device, pgtg_handle** out);
int pgtg_destroy(pgtg_handle* h);
/* Queue work on this stream (hipStream_t); NULL = the null stream.  The stream contract of the library:
 *   - every launch, copy and memset of an entry point goes to the stream bound when it is called, and when the
 *     entry point returns, everything it wrote to the handle's device state is ordered before the next launch
 *     on that stream (the allocations of pgtg_create are zeroed before it returns);
 *   - the handle does not order one stream with another: a caller that binds another stream orders it with the
 *     work queued on the last one (an event, a synchronisation), as it would for any buffer it moves between
 *     streams; the same holds for the buffers it binds or passes in;
 *   - the entry points that read or write device state from the host (the getters, pgtg_set_agent,
 *     pgtg_add_car, pgtg_set_to_state, pgtg_set_rules, pgtg_dump_state, pgtg_load_state,
 *     pgtg_set_block_shares with counts) first drain the bound stream themselves;
 *   - a host array passed in (seeds_host, a state blob, rules, cars, counts) is read before the call returns
 *     and may be reused or freed at once. */
int pgtg_set_stream(pgtg_handle* h, void* stream);
/* Bind the output buffers.  Between step launches the bound `obs` buffer belongs to the handle: the persistent
 * map-queue step kernel (k_envq) writes only the observations that changed since the last launch (whole
 * 128-byte lines) and relies on the other bytes being the ones it wrote before.  A caller that wrote into `obs`
 * calls pgtg_observe or binds the outputs again before the next step; reading it is always fine.  Every
 * call that changes an env's state or the binding without rewriting all observations (this one, a masked
 * reset, pgtg_set_agent, pgtg_add_car, pgtg_set_to_state, pgtg_load_state, pgtg_snapshot_load,
 * pgtg_set_rules) makes the next step write every observation, so a step right after one of them returns
 * correct observations without pgtg_observe.  final_obs and every other output are written in full. */
int pgtg_set_outputs(pgtg_handle* h, const PgtgOutputs* out);
/* Seeded reset of env i with seeds_host[i] (NULL: seed_base + global index), only where
 * mask_dev[i] != 0 (NULL: all).  Writes the reset observation to the bound outputs.  seeds_host ([N], pageable
 * or pinned) is copied into a pinned array of the handle before the call returns and uploaded from there on the
 * handle's stream: the caller's array is not read afterwards.  The call does not wait for the device, except
 * that a second seed-list reset waits for the first one's upload before it reuses the pinned array. */
int pgtg_reset(pgtg_handle* h, const uint64_t* seeds_host, uint64_t seed_base, const uint8_t* mask_dev);
/* Unseeded reset (next spawn block of each env's seed sequence) where mask_dev[i] != 0. */
int pgtg_reset_unseeded(pgtg_handle* h, const uint8_t* mask_dev);
/* One tick for every env.  actions_dev: [N] uint8 in [0, 9). */
int pgtg_step(pgtg_handle* h, const uint8_t* actions_dev);
/* `ticks` consecutive pgtg_step calls from a resident rollout action buffer: tick k reads the [N]
 * row at actions_dev + k * row_stride bytes (row_stride >= N).  Identical results to the loop of
 * pgtg_step calls (the outputs hold the last tick's); one host call, so the launches are queued
 * without per-tick host overhead.  Stops at the first launch error. */
int pgtg_step_many(pgtg_handle* h, const uint8_t* actions_dev, uint64_t row_stride, uint64_t ticks);
/* Fill [N] uint8 actions with a counter-based uniform hash of (seed, env_offset + env, t) --
 * synthetic rollouts; env_offset = global index of env 0 so that a sharded run draws the same
 * actions as one GPU running the whole batch. */
int pgtg_random_actions(pgtg_handle* h, uint8_t* actions_dev, uint64_t seed, uint64_t t, uint64_t env_offset);
/* Host-synchronising introspection (copies device state). */
int pgtg_get_env_state(pgtg_handle* h, uint64_t env, PgtgEnvState* st);
int pgtg_get_cars(pgtg_handle* h, uint64_t env, PgtgCar* cars, int32_t cap, int32_t* n);
int pgtg_get_map_plan(pgtg_handle* h, uint64_t env, int32_t* w, int32_t* h_, uint8_t* exits, int8_t* otype,
                      int8_t* omask, int32_t* start3, int32_t* goal3);
/* The episode map's squares as feature words, x-major (index x * height + y), height = 9 * tile rows:
 * bits 0-31 the car lanes (lane ids of the tables), then the PGTG_SQ_* flags below. */
#define PGTG_SQ_WALL (1ull << 32)
#define PGTG_SQ_SPAWNER (1ull << 37)
#define PGTG_SQ_START (1ull << 38)
#define PGTG_SQ_SUBGOAL (1ull << 39)
#define PGTG_SQ_USED_SUBGOAL (1ull << 40)
#define PGTG_SQ_FINAL_GOAL (1ull << 41)
#define PGTG_SQ_ICE (1ull << 42)
#define PGTG_SQ_BROKEN_ROAD (1ull << 43)
#define PGTG_SQ_SAND (1ull << 44)
#define PGTG_SQ_TRAFFIC_LIGHT (1ull << 45)
int pgtg_get_squares(pgtg_handle* h, uint64_t env, uint64_t* words, int32_t cap, int32_t* width, int32_t* height);
int pgtg_set_agent(pgtg_handle* h, uint64_t env, int32_t x, int32_t y, int32_t vx, int32_t vy);
/* Append a car (env.cars.append(Car(...)) in the reference tests); car_id < 0 takes the env's next id. */
int pgtg_add_car(pgtg_handle* h, uint64_t env, int32_t x, int32_t y, int32_t route, int32_t profile, int32_t car_id);
/* Whole-batch state for bit-exact replay: every device array that carries env state
 * between launches (agent records, seeds, tile plans, all RNG streams with their buffered halves,
 * visited bitsets, the car slots, traffic records with the persisted lane-square occupancy counters,
 * spawner lists, map queue, counters) as one host
 * blob.  pgtg_state_size gives the blob size; pgtg_load_state accepts only a blob dumped from a handle
 * of the same config (checked by a hash of every configuration field) and batch size.  Outputs are not state: call pgtg_observe after a load to
 * re-emit the observations.  Both synchronise.  (No reference equivalent: PGTGEnv deep-copies
 * itself in light_step, environment.py:1283-1299.) */
int pgtg_state_size(pgtg_handle* h, uint64_t* bytes);
int pgtg_dump_state(pgtg_handle* h, void* buf, uint64_t bytes);
int pgtg_load_state(pgtg_handle* h, const void* buf, uint64_t bytes);
/* Device-resident snapshots: single envs saved, restored and forked without leaving the GPU (the
 * deepcopy of PGTGEnv.light_step, environment.py:1283-1299, and the env.clone() of Evaluator.evaluate,
 * pgtg/evaluator.py:98-110, for any subset of a batch).  A snapshot owns device arrays with the layouts
 * of the handle's per-env state sections (everything in the state blob but the batch-wide counters),
 * allocated zeroed for `slots` envs; `slots` need not be the handle's batch size.  It records the
 * handle's configuration hash, the shape fields of the blob header (tile count, car capacity and slots,
 * plan stride, spawner capacity, visited words, ring entry words), the map ring's layout and the device:
 * pgtg_snapshot_save / _load accept ANY handle on that device for which all of these are equal -- a
 * snapshot saved from one handle loads into another handle of another batch size -- and refuse every
 * other handle with PGTG_E_INVALID and a message on that handle, launching nothing.  (The ring layout
 * follows the map-queue step kernel, which tune_queue_mode 0 picks from the batch size: k_envq keeps three
 * 128-byte-aligned slots per env (one more than before), the live episode's tile plan in one of them, and
 * no separate plan row (device memory per env: one slot more, the row less.  A slot is the plan's 16-byte
 * quads plus 16 bytes in whole 128-byte lines, a row the plan in whole lines, or 32 bytes below 16 tiles:
 * equal for 16 to 56 tiles (5x5: 128 and 128) and for 9x9 (256 and 256), +96 bytes below 16 tiles, +128
 * bytes where the 16 bytes open another line, e.g. 57 to 64 tiles),
 * k_envb three queued maps beside the plan row; state blobs of one are refused by the other in the same
 * way.  Fix it with tune_queue_mode to share snapshots between batches of very different sizes.  k_envq
 * handles hold at most 2^30 envs: PGTG_E_UNSUPPORTED from pgtg_create beyond.)
 *   save: env env_idx_dev[k] of h -> slot slot_idx_dev[k];   load: slot slot_idx_dev[k] -> env
 *   env_idx_dev[k] of h, for k < count.  Index arrays are uint32 device arrays; NULL = the identity k.
 * One launch of k_state_copy (after the pending map-ring refills, as before pgtg_dump_state) on the
 * handle's stream: neither call synchronises, and the snapshot's contents are ordered with that stream --
 * a save on one handle's stream and a load on another's need the caller's event between them, or one
 * stream for both handles.  A pair with an index outside its side is skipped.  A slot may be loaded into
 * many envs in one call (fork); two pairs with the same DESTINATION in one call are the caller's error:
 * that env or slot ends up with an unspecified mix of the two sources (nothing outside it is touched).
 * Loading a slot that was never saved gives an env of zero bytes, not a valid episode.  Outputs are not
 * state: call pgtg_observe after a load.  The TimeLimit step count is in the agent record and travels
 * with the env; the episode accumulators of pgtg_set_episode_stats are not state: a load zeroes them for
 * the envs it wrote and leaves the summary as it is.  count = 0 is a no-op.  pgtg_snapshot_destroy waits
 * for the device.  pgtg_snapshot_bytes: the device memory the snapshot holds and the state bytes of one
 * env (what a save or a load reads and writes per pair). */
typedef struct pgtg_snapshot pgtg_snapshot;
int pgtg_snapshot_create(pgtg_handle* h, uint64_t slots, pgtg_snapshot** out);
int pgtg_snapshot_destroy(pgtg_snapshot* s);
int pgtg_snapshot_bytes(const pgtg_snapshot* s, uint64_t* device_bytes, uint64_t* bytes_per_env);
int pgtg_snapshot_save(pgtg_handle* h, pgtg_snapshot* s, const uint32_t* env_idx_dev, const uint32_t* slot_idx_dev,
                       uint64_t count);
int pgtg_snapshot_load(pgtg_handle* h, const pgtg_snapshot* s, const uint32_t* slot_idx_dev, const uint32_t* env_idx_dev,
                       uint64_t count);
/* PGTGEnv.set_to_state(state) (environment.py:1301-1342) for one env: position, velocity, flat tire
 * and the car list (patience/delay 0; next car id = last id + 1 if any cars).  Synchronises. */
int pgtg_set_to_state(pgtg_handle* h, uint64_t env, int32_t x, int32_t y, int32_t vx, int32_t vy, int32_t flat_tire,
                      const PgtgCar* cars, int32_t n_cars);
/* Replace the traffic rules of every env (add_traffic_rule / remove_traffic_rule,
 * environment.py:569-575); takes effect from the next step.  n_rules <= PGTG_MAX_RULES. */
int pgtg_set_rules(pgtg_handle* h, const PgtgRule* rules, int32_t n_rules);
/* FlattenObservation rows (pgtg/train.py:40; gymnasium's flatten of the Dict observation space of
 * environment.py:415-441, keys in name order), written by k_flatten after every launch that writes the
 * bound observation (step, reset, observe): per env, D = n_channels*win*win (+ 9) + 18 + 2 values
 *   map channels in `order` (order[k] = channel of the k-th name-sorted key), win*win each, [x][y] |
 *   next-subgoal one-hot at direction + 1 (9, only with use_next_subgoal_direction) |
 *   position one-hot of x (9), of y (9) | velocity (2)
 * as float32 (dtype 0) or int8 (dtype 1: exact, every value being 0/1 or a velocity) into flat_dev
 * [N][D]; final_flat_dev [N][D] receives the terminal observations of the envs that finished in a step
 * (their rows only; the other rows are left as they are).  Buffers 16-byte aligned; NULL, NULL = off.
 * Needs the corresponding PgtgOutputs bound first; a sliding window of size >= 9 is refused
 * (PGTG_E_UNSUPPORTED) as gymnasium's flatten raises for it.  No reference function: it replaces the
 * FlattenObservation wrapper the reference's caller puts around each env. */
int pgtg_set_flat_outputs(pgtg_handle* h, const int32_t* order, int32_t n_order, int32_t dtype, void* flat_dev,
                          void* final_flat_dev);
/* With flat rows bound, the observation pass of k_flatten also writes, per env, the reward as float32,
 * done = terminated | truncated and truncated-and-not-terminated (uint8 0/1) -- what an SB3-style
 * vector env returns -- into these [N] device buffers (all three or none; needs the reward, terminated
 * and truncated outputs bound).  No reference function: it replaces per-step tensor arithmetic. */
int pgtg_set_flat_scalars(pgtg_handle* h, float* reward_f32_dev, uint8_t* dones_dev, uint8_t* truncated_only_dev);
/* With the flat scalars bound, the same pass also writes the cost of separate_reward_cost (info["cost"],
 * environment.py:1130-1276) as float32, (float)cost[e], into this [N] device buffer.  NULL unbinds.  Valid only
 * on a handle created with separate_reward_cost whose cost output is bound, and only while the scalars of
 * pgtg_set_flat_scalars are bound: PGTG_E_INVALID with a message otherwise, and nothing changes.
 * pgtg_set_flat_scalars(NULL, NULL, NULL) unbinds the cost too; rebinding the three scalars keeps it. */
int pgtg_set_flat_cost(pgtg_handle* h, float* cost_f32_dev);
/* k_flatten alone, over the bound outputs as they are now (tests: rows from chosen inputs, without a
 * step, reset or observe launch rewriting the observation first).  mode: 0 the observation rows and
 * the scalars of pgtg_set_flat_scalars, 1 the terminal rows of the envs whose terminated | truncated
 * is set, 2 both -- the launch a step makes.  grid: 0 the grid a step uses, else that many workgroups,
 * each taking ceil(N / grid) consecutive envs.  PGTG_E_INVALID with a message, nothing launched: a
 * grid below ceil(N / 256) (the kernel lists at most 256 envs per workgroup) or above N, or a mode
 * whose destination is not bound.  The same launch site as the step path's.  Asynchronous on the
 * handle's stream. */
int pgtg_flatten(pgtg_handle* h, int32_t mode, int32_t grid);
/* Episode return and length per env (new; no reference function: it replaces SB3's VecMonitor wrapper of
 * pgtg/train.py:55, whose info["episode"] = {"r", "l"} feeds ep_rew_mean / ep_len_mean).  The handle
 * keeps per env a float32 return and an int32 length; with the two [N] buffers bound, every pgtg_step
 * (each tick of pgtg_step_many) ends with the kernel k_episode, which per env e does
 *   ret[e] += (float)reward[e];  len[e] += 1;  ep_return[e] = ret[e];  ep_length[e] = len[e]
 *   if (terminated[e] | truncated[e]) { the episode joins the summary;  ret[e] = 0;  len[e] = 0 }
 * so a finished env's row holds its episode's totals, the others their running values (the reward output
 * only, also with separate_reward_cost; the same rule with autoreset = 0, the accumulators restarting at
 * the env's next reset).  Both buffers or neither (NULL, NULL = off; frees nothing).  The accumulators are
 * allocated, zeroed, at the first binding and kept when other buffers are bound; pgtg_reset and
 * pgtg_reset_unseeded zero them for the envs they reset.  They are NOT part of the state blob:
 * pgtg_load_state zeroes them for every env and leaves the summary as it is.  Needs the reward, terminated
 * and truncated outputs bound (PGTG_E_INVALID otherwise); while statistics are bound, pgtg_set_outputs
 * refuses a set without one of the three (PGTG_E_INVALID, the previous outputs stay bound). */
int pgtg_set_episode_stats(pgtg_handle* h, float* ep_return_dev, int32_t* ep_length_dev);
/* Episodes finished since create or since the last call with reset != 0 (one row per 256 envs, updated
 * without atomics and combined here in row order: the same bits on any device and for any step kernel).
 * Synchronises.  PGTG_E_INVALID if statistics were never bound. */
int pgtg_episode_summary(pgtg_handle* h, PgtgEpisodeSummary* out, int32_t reset);
/* Generalised advantage estimation over a device-resident rollout of N envs and T steps (new; no
 * reference function: it replaces RolloutBuffer.compute_returns_and_advantage of the PPO of
 * pgtg/train.py:61-74, and the time-limit bootstrap reward += gamma * V(terminal_observation) that its
 * collect_rollouts applies to truncated envs).  One launch of k_gae, one lane per env, float32 and
 * without fused multiply-add, operation for operation what SB3 computes in numpy:
 *   g = (float)gamma;  gl = (float)(gamma * gae_lambda)  (the product in double);  last = 0;  t = T-1 .. 0:
 *   r     = truncated_only[t][e] ? rewards[t][e] + g * terminal_values[t][e] : rewards[t][e]
 *   nnt   = 1.0f - (float)(dones[t+1][e] != 0)
 *   nv    = t == T-1 ? last_values[e] : values[t+1][e]
 *   delta = (r + (g * nv) * nnt) - values[t][e]
 *   last  = delta + (gl * nnt) * last
 *   advantages[t][e] = last;  returns[t][e] = last + values[t][e]
 * All pointers are device pointers.  The handle is used for its device, stream and error string only: n
 * need not be its batch size.  steps == 0, a NULL required pointer, only one of truncated_only /
 * terminal_values, or a non-finite gamma or gae_lambda: PGTG_E_INVALID with a message, nothing is
 * launched.  n == 0 is a no-op.  Asynchronous on the handle's stream. */
typedef struct {
  uint64_t n, steps;              /* N envs, T >= 1 rows; every [T][N] array row-contiguous with pitch N */
  double gamma, gae_lambda;
  const float*   rewards;         /* [T][N] raw float32 rewards (k_flatten's scalar) */
  const float*   values;          /* [T][N] */
  const uint8_t* dones;           /* [T+1][N]: row t = episode_starts of step t, row T = dones after the last step */
  const uint8_t* truncated_only;  /* [T][N]; NULL together with terminal_values = no bootstrap */
  const float*   terminal_values; /* [T][N]; read ONLY where truncated_only != 0 */
  const float*   last_values;     /* [N] */
  float* advantages; float* returns;   /* [T][N] */
} PgtgGae;
int pgtg_gae(pgtg_handle* h, const PgtgGae* a);
/* The safety cost of a device-resident rollout of N envs and T steps (new; no reference function: the
 * reference returns info["cost"] per step and leaves the rest to its caller): per-episode cost sums, the
 * Lagrangian penalty on the reward (RCPO, Tessler et al. 2018) and the dual ascent of the multiplier on the mean
 * episode cost against a budget.  Two launches.  k_cost_scan, one lane per env, no fused multiply-add, with
 * lam = *lambda as it stood before the call, acc = ep_cost[e], t = 0 .. T-1:
 *   penalised[t][e] = rewards[t][e] - lam * costs[t][e]      (float32: the product rounds, then the difference)
 *   acc += (double)costs[t][e]
 *   dones[t+1][e] != 0:  the episode joins the summary with cost acc;  acc = 0
 *   ep_cost[e] = acc  (after row T-1: the cost of the episode under way, carried into the next rollout)
 * then k_cost_dual, one workgroup, which writes *summary and, with episodes > 0, in fp64
 *   cost_mean = cost_sum / episodes;  l = (double)lam + lambda_lr * (cost_mean - cost_limit)
 *   *lambda = (float)min(max(l, 0), lambda_max)
 * (episodes == 0: cost_mean = cost_max = 0 and the word is left as it is).  cost_sum runs in one order, a
 * function of N alone (per env in step order, 256 envs per workgroup by a shuffle tree and wave order, the
 * workgroups' rows in row order; no atomics): the same arrays give the same bits on any device.  penalised is
 * what pgtg_gae then takes as its rewards.  All pointers are device pointers; ep_cost, summary and workspace
 * (pgtg_cost_workspace_bytes(n) bytes, contents irrelevant) 8-byte aligned.  The handle is used for its device,
 * stream and error string only.  steps == 0, a NULL or misaligned pointer, a non-finite cost_limit or
 * lambda_lr, lambda_max < 0 or NaN: PGTG_E_INVALID; a rollout beyond one launch (pgtg_gae's limits):
 * PGTG_E_UNSUPPORTED; each with a message, nothing launched.  n == 0 is a no-op.  Asynchronous on the
 * handle's stream. */
typedef struct {
  uint64_t episodes;                       /* episodes that ended inside the rollout */
  double cost_sum, cost_mean, cost_max;    /* of their costs */
  float lambda_before, lambda_after;       /* the multiplier the rollout was penalised with, and the next */
} PgtgCostSummary;
typedef struct {
  uint64_t n, steps;
  const float*   rewards;     /* [T][N] */
  const float*   costs;       /* [T][N] (k_flatten's scalar of pgtg_set_flat_cost) */
  const uint8_t* dones;       /* [T+1][N]: row t+1 = the episode ended in step t */
  double* ep_cost;            /* [N] carry: cost of the episode under way (in/out) */
  float*  penalised;          /* [T][N] out */
  float*  lambda;             /* device word, in/out */
  double cost_limit, lambda_lr, lambda_max;
  PgtgCostSummary* summary;   /* device, out */
  void* workspace;
} PgtgCost;
int pgtg_cost_workspace_bytes(uint64_t n, uint64_t* bytes);
int pgtg_cost_scan(pgtg_handle* h, const PgtgCost* a);
/* Running return normalisation of the reward of a device-resident rollout of N envs and T steps (new; no
 * reference function: SB3's VecNormalize(norm_reward=True), reward half, which a user of the reference wraps the
 * env in).  In fp64, no fused multiply-add, per step t = 0 .. T-1 in order, ret = returns, (mean, var, count) = rms:
 *   ret[e] = ret[e] * gamma + (double)rewards[t][e]
 *   (nb, mb, vb) = the count, mean and population variance of ret over the N envs
 *   delta = mb - mean;  tot = count + nb;  mean' = mean + delta * nb / tot
 *   var' = (var * count + vb * nb + delta * delta * count * nb / tot) / tot;  count' = tot
 *   row_var[t] = var';  normalised[t][e] = (float)min(max((double)rewards[t][e] / sqrt(var' + epsilon), -clip), clip)
 *   dones[t+1][e] != 0:  ret[e] = 0
 * (RunningMeanStd.update_from_moments; step t is normalised with statistics that include step t, as SB3 does).
 * Four launches: k_ret_scan (one lane per env; each wave of 64 envs writes the (n, mean, M2) of its returns per
 * step into the workspace), k_ret_stats twice (one workgroup per step merges that step's partials; then one lane
 * walks the steps) and k_ret_apply (elementwise).  The moments are merged pairwise and count-aware (Chan et al.:
 * n = na + nb; d = mb - ma; mean = ma + d * (nb / n); M2 = M2a + M2b + d * d * (na * nb / n); an empty operand
 * returns the other), each wave by a shuffle tree, a step's waves by lane l taking partials l, l + 256, ... and the
 * same tree: every order is a function of N and T alone, so the same arrays give the same bits on any device.
 * training == 0: returns, rms and row_var are left as they are, and k_ret_apply alone runs, every row divided
 * by sqrt(rms[1] + epsilon).  All pointers are device pointers; returns, rms, row_var and workspace
 * (pgtg_reward_norm_workspace_bytes(n, steps) bytes, contents irrelevant) 8-byte aligned.  The handle is used
 * for its device, stream and error string only.  steps == 0, a NULL or misaligned pointer, a negative or
 * non-finite epsilon or clip, gamma outside [0, 1] or NaN: PGTG_E_INVALID; a rollout beyond one launch
 * (pgtg_gae's limits): PGTG_E_UNSUPPORTED; each with a message, nothing launched.  n == 0 is a no-op.
 * Asynchronous on the handle's stream. */
typedef struct {
  uint64_t n, steps;
  double gamma, epsilon, clip;
  int32_t training;           /* 0: the statistics and returns are frozen */
  const float*   rewards;     /* [T][N] */
  const uint8_t* dones;       /* [T+1][N]: row t+1 = the episode ended in step t */
  double* returns;            /* [N] the discounted return of the episode under way (in/out) */
  double* rms;                /* [3] mean, var, count of the returns seen so far (in/out) */
  double* row_var;            /* [T] out: var after step t */
  float*  normalised;         /* [T][N] out */
  void* workspace;
} PgtgRewardNorm;
int pgtg_reward_norm_workspace_bytes(uint64_t n, uint64_t steps, uint64_t* bytes);
int pgtg_reward_norm(pgtg_handle* h, const PgtgRewardNorm* a);
/* The acting forward pass of SB3's MlpPolicy over int8 flat rows (new; no reference function: it replaces
 * ActorCriticPolicy.forward / predict_values of the PPO("MlpPolicy") of pgtg/train.py:61-74 inside
 * collect_rollouts).  Separate pi / vf towers, 64-64, tanh, 9 actions; float32 throughout.  Per env e,
 * x = the obs_dim signed bytes of its row (row e starts at byte e * obs_dim of obs; any base alignment):
 *   h1p = tanh(W1p x + b1p)   h2p = tanh(W2p h1p + b2p)   logits = Wa h2p + ba   (9)
 *   h1v = tanh(W1v x + b1v)   h2v = tanh(W2v h1v + b2v)   value  = Wv h2v + bv
 *   log_prob = logits[a] - (max + log(sum exp(logits - max)))
 * mode PGTG_POLICY_SAMPLE: p = exp(logits - max) / sum in float32, c_a its running sum in action order,
 *   a = the least a with u < c_a, 8 if there is none; u = uniforms[e] if uniforms is given, otherwise the
 *   counter-based hash of (seed, counter, env_offset + e) (pgtg_amd.policy.policy_uniform: 24 bits in [0, 1)).
 * mode PGTG_POLICY_ARGMAX: a = the least index among the maxima (predict(deterministic=True)).
 * mode PGTG_POLICY_VALUE_ONLY: the vf tower alone; only values is written (and is required).
 * actions, values, log_probs: [n] each, NULL = not written.  No load touches a byte outside
 * [obs, obs + n * obs_dim).  One launch of k_policy, asynchronous on the handle's stream; the handle gives
 * the device, the stream and the error string only (n and obs_dim need not be its own).  obs_dim == 0 or
 * beyond PGTG_POLICY_MAX_OBS_DIM, obs or packed NULL (packed: 16-byte aligned), an unknown mode or
 * n * obs_dim overflowing: PGTG_E_INVALID with a message, nothing is launched.  n == 0 is a no-op.
 *
 * packed is the kernel's own weight layout, written by pgtg_policy_pack (one launch of k_policy_pack on the
 * handle's stream, no host copy; once per PPO update) from twelve device pointers in SB3's nn.Linear
 * layouts, float32, contiguous: w1* [64][obs_dim], w2* [64][64], wa [9][64], wv [1][64] and their biases.
 * pgtg_policy_packed_bytes gives the buffer's size for an obs_dim; pgtg_policy_chunk the observation
 * bytes of a row the kernel stages at a time (tests place obs_dim around it). */
#define PGTG_POLICY_SAMPLE 0
#define PGTG_POLICY_ARGMAX 1
#define PGTG_POLICY_VALUE_ONLY 2
#define PGTG_POLICY_MAX_OBS_DIM 1048576
typedef struct {
  const float *w1p, *b1p, *w2p, *b2p, *wa, *ba;   /* mlp_extractor.policy_net.{0,2}, action_net */
  const float *w1v, *b1v, *w2v, *b2v, *wv, *bv;   /* mlp_extractor.value_net.{0,2}, value_net */
  uint64_t obs_dim;
} PgtgPolicyWeights;
typedef struct { uint64_t n, obs_dim; const int8_t* obs; const void* packed;
                 int32_t mode; uint64_t seed, counter, env_offset;
                 const float* uniforms; uint8_t* actions; float* values; float* log_probs; } PgtgPolicy;
int pgtg_policy_packed_bytes(uint64_t obs_dim, uint64_t* bytes);
int pgtg_policy_pack(pgtg_handle* h, const PgtgPolicyWeights* raw, void* packed);
int pgtg_policy(pgtg_handle* h, const PgtgPolicy* a);
int pgtg_policy_chunk(void);
/* One minibatch of SB3's PPO.train (defaults; clip_range_vf = None) over a finished rollout of int8 rows
 * (new; no reference function: it replaces the forward, the loss and loss.backward() of the PPO("MlpPolicy")
 * of pgtg/train.py:61-74).  Sample s = 0 .. batch-1 is (env, step) = (indices[s] / steps, indices[s] % steps),
 * SB3's swap_and_flatten order; its row starts at byte step * obs_pitch + env * obs_dim of obs (any base
 * alignment; no load touches a byte outside [obs, obs + (steps-1) * obs_pitch + n * obs_dim)); repeats are
 * allowed; the [batch, obs_dim] matrix is never materialised.  With logits, value the forward of pgtg_policy
 * (the same tiling and order of operations) under `packed`, a = actions[step][env], and every mean over batch:
 *   adv   = adv_stats ? (advantages - adv_stats[0]) * adv_stats[1] : advantages
 *   ratio = exp(log_prob(a) - log_probs[step][env])
 *   policy_loss  = mean(-min(adv ratio, adv clamp(ratio, 1 - clip_range, 1 + clip_range)))
 *   value_loss   = mean((returns - value)^2)        entropy_loss = -mean(-sum_c p_c log p_c)
 *   loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 * and d loss / d(every one of the twelve tensors) is written (not accumulated) into grads, float32 in SB3's
 * nn.Linear layouts (PgtgPolicyWeights); the min passes adv where its unclipped branch is the smaller or the
 * ratio lies inside the clip interval, and 0 otherwise.  stats[8] (device): loss, policy_loss, value_loss,
 * entropy_loss, approx_kl = mean((ratio - 1) - log ratio), clip fraction = mean(|ratio - 1| > clip_range), 0, 0.
 * An index outside [0, steps * n), or a sample whose action is above 8, is not dereferenced: the sample adds
 * nothing to any sum (the means stay over batch) and sets the handle's error byte s mod its batch size to
 * -PGTG_E_INVALID (pgtg_error_count).  Three launches (k_ppo_loss, k_ppo_dw1, k_ppo_reduce), asynchronous on
 * the handle's stream, no atomics: the partition of the work is a function of (batch, obs_dim) alone and every
 * sum runs in a fixed order, so the same call gives the same bits.  workspace: pgtg_ppo_workspace_bytes bytes,
 * 16-byte aligned, contents irrelevant.  A NULL required pointer (adv_stats alone may be NULL), obs_dim outside
 * [1, PGTG_POLICY_MAX_OBS_DIM], steps or n of 0, obs_pitch < n * obs_dim, packed or workspace not 16-byte
 * aligned, products that overflow, a non-finite coefficient: PGTG_E_INVALID with a message, nothing launched.
 * batch == 0 is a no-op. */
typedef struct {
  float *w1p, *b1p, *w2p, *b2p, *wa, *ba;
  float *w1v, *b1v, *w2v, *b2v, *wv, *bv;
} PgtgPpoGrads;
typedef struct {
  uint64_t batch, obs_dim, steps, n, obs_pitch;   /* B, D, T, N, bytes from obs[t] to obs[t+1] */
  const int8_t* obs; const int64_t* indices;      /* indices [batch] */
  const uint8_t* actions;                         /* [steps][n], as log_probs, advantages, returns */
  const float *log_probs, *advantages, *returns;
  const void* packed;                             /* pgtg_policy_pack's buffer */
  const float* adv_stats;                         /* {mean, 1 / (std + 1e-8)} or NULL */
  double clip_range, ent_coef, vf_coef;
  void* workspace;
  PgtgPpoGrads grads;
  float* stats;                                   /* [8] */
} PgtgPpoGrad;
int pgtg_ppo_workspace_bytes(uint64_t obs_dim, uint64_t batch, uint64_t* bytes);
int pgtg_ppo_grad(pgtg_handle* h, const PgtgPpoGrad* a);
/* The optimiser step that follows pgtg_ppo_grad (new; no reference function: it replaces
 * torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step with weight_decay = 0, amsgrad = False, maximize =
 * False, and the repack of pgtg_policy_pack).  Over all twelve tensors, float32:
 *   total = sqrt(sum g^2)        coef = min(1, max_grad_norm / (total + 1e-6))        g <- coef g  (not stored)
 *   m <- m + (1 - beta1) (g - m)        v <- beta2 v + (1 - beta2) g^2
 *   p <- p - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with lr / (1 - beta1^step) and sqrt(1 - beta2^step) computed in double on the host and rounded once, as torch
 * computes them in Python floats; lr, beta1 and beta2 enter those as the shortest decimals that round to the
 * float32 given (0.999f stands for 0.999), so that 1 - beta2 is torch's.  params, exp_avg and exp_avg_sq are updated in place in SB3's nn.Linear
 * layouts, grads is only read, and every word of packed (pgtg_policy_packed_bytes) is rewritten with the new
 * weights in k_policy's layout, its padding words with 0: the bits pgtg_policy_pack would write from the new
 * params.  grad_norm (device, optional) receives total.  Two launches (k_ppo_gnorm, k_ppo_adam), asynchronous on
 * the handle's stream, no atomics: the partition is a function of obs_dim alone and every sum runs in a fixed
 * order, so the same call from the same state gives the same bits.  workspace: pgtg_ppo_step_workspace_bytes
 * bytes, 8-byte aligned, contents irrelevant (the sums of squares are taken in double).  Non-finite gradients are not detected: the result is what the arithmetic above
 * gives (clip_grad_norm_ with error_if_nonfinite = False).  Any of the 48 tensor pointers, packed or workspace
 * NULL, packed not 16-byte or workspace not 8-byte aligned, obs_dim outside [1, PGTG_POLICY_MAX_OBS_DIM], step == 0, a non-finite lr,
 * eps or beta, a beta outside [0, 1), max_grad_norm NaN or <= 0 (+inf: no clip): PGTG_E_INVALID with a
 * message, nothing is launched. */
typedef struct {
  const float *w1p, *b1p, *w2p, *b2p, *wa, *ba;
  const float *w1v, *b1v, *w2v, *b2v, *wv, *bv;
} PgtgPpoConstGrads;                 /* PgtgPpoGrads, read only */
typedef struct {
  uint64_t obs_dim;
  PgtgPpoGrads params;               /* twelve float32 tensors, nn.Linear layout, updated in place */
  PgtgPpoConstGrads grads;           /* read only (pgtg_ppo_grad's output) */
  PgtgPpoGrads exp_avg, exp_avg_sq;  /* Adam's moments, same shapes, updated in place */
  void* packed;                      /* pgtg_policy_pack's buffer: every word rewritten */
  void* workspace;                   /* pgtg_ppo_step_workspace_bytes(obs_dim) bytes */
  uint64_t step;                     /* 1 for the first step */
  float lr, beta1, beta2, eps, max_grad_norm;   /* max_grad_norm = +inf: no clip */
  float* grad_norm;                  /* optional: the total norm before clipping */
} PgtgPpoStep;
int pgtg_ppo_step_workspace_bytes(uint64_t obs_dim, uint64_t* bytes);
int pgtg_ppo_step(pgtg_handle* h, const PgtgPpoStep* a);
/* out = {mean, 1 / (std + 1e-8)} (device, float32) of the batch advantages[indices[s] % steps][indices[s] / steps],
 * s = 0 .. batch-1: pgtg_ppo_grad's adv_stats.  The unbiased std in two passes (the mean, then the squared
 * deviations); an index outside [0, steps * n) stands as an advantage of 0 (pgtg_ppo_grad still skips and counts
 * that sample).  One launch of one workgroup (k_ppo_adv_stats), asynchronous on the handle's stream; the
 * partition is a function of batch alone and the order is fixed.  A NULL pointer, batch < 2 (SB3 does not
 * normalise a batch of one), steps or n of 0, steps * n overflowing: PGTG_E_INVALID, nothing is launched. */
int pgtg_ppo_adv_stats(pgtg_handle* h, const void* advantages, const void* indices, uint64_t batch, uint64_t steps,
                       uint64_t n, float* out);
/* The rest of SB3's PPO.train (new): value-function clipping, target_kl without a host synchronisation per
 * minibatch, the train log and the epoch's permutation.  The three _ex entry points take the call they extend
 * and a PgtgPpoExtra; extra == NULL is exactly that call (pgtg_ppo_grad, pgtg_ppo_step and pgtg_ppo_adv_stats
 * call them so), and so is an extra of zeros.
 *   PGTG_PPO_CLIP_VF (pgtg_ppo_grad_ex): with v0 = old_values[step][env] (required; the rollout's values) and
 *     c = clip_range_vf, value_loss = mean((returns - (v0 + clamp(value - v0, -c, c)))^2), whose derivative with
 *     respect to value is that of the unclipped term where -c <= value - v0 <= c (boundaries included, as
 *     torch.clamp's) and 0 elsewhere.  Only the value tower's gradients, value_loss and loss change.
 *   stop_at (device uint32, the update's stop word: 0 when the update starts) with ordinal = m, the place
 *     1, 2, ... of the minibatch within the update, is the gate: a kernel of pgtg_ppo_adv_stats_ex or
 *     pgtg_ppo_grad_ex returns at once when stop_at != 0 && stop_at < m, one of pgtg_ppo_step_ex when
 *     stop_at != 0 && stop_at <= m, having written nothing (gradients, stats, parameters, moments, packed and
 *     grad_norm keep their contents).  The host launches every minibatch and reads stop_at once, at the end.
 *   PGTG_PPO_TARGET_KL (pgtg_ppo_grad_ex; stop_at required): the thread that writes stats stores stop_at = m
 *     when stop_at == 0 and approx_kl > 1.5f * (float)target_kl (a float32 compare; NaN compares false).  That
 *     minibatch has written its gradients and stats and takes no step: SB3's break before optimizer.step().
 *     No kernel is gated by a value its own launch writes, so the outcome does not depend on the order in
 *     which workgroups run.
 * clip_range_vf or target_kl negative or non-finite, PGTG_PPO_CLIP_VF without old_values, PGTG_PPO_TARGET_KL
 * without stop_at, stop_at with ordinal == 0 or not 4-byte aligned, unknown flags: PGTG_E_INVALID, nothing launched. */
#define PGTG_PPO_CLIP_VF 1u
#define PGTG_PPO_TARGET_KL 2u
typedef struct {
  uint32_t flags;            /* PGTG_PPO_CLIP_VF | PGTG_PPO_TARGET_KL */
  uint32_t ordinal;          /* m = 1, 2, ...; read when stop_at is set */
  const float* old_values;   /* [steps][n] */
  double clip_range_vf, target_kl;
  uint32_t* stop_at;         /* device; NULL: no gate */
} PgtgPpoExtra;
int pgtg_ppo_grad_ex(pgtg_handle* h, const PgtgPpoGrad* a, const PgtgPpoExtra* extra);
int pgtg_ppo_step_ex(pgtg_handle* h, const PgtgPpoStep* a, const PgtgPpoExtra* extra);
int pgtg_ppo_adv_stats_ex(pgtg_handle* h, const void* advantages, const void* indices, uint64_t batch, uint64_t steps,
                          uint64_t n, float* out, const PgtgPpoExtra* extra);
/* out[2] (device, float32) = {1 - r, r} with r = var(returns - values) / var(returns) over count float32 values
 * each (a rollout's [steps][n] arrays, contiguous): SB3's explained_variance(values.flatten(),
 * returns.flatten()) and the ratio it is one minus (which keeps its relative precision when the value function
 * is good).  Population variances in two passes (the means, then the squared deviations), in fp64; both NaN
 * when var(returns) == 0.  Three launches (k_ppo_expl_var), asynchronous on the handle's stream; the partition
 * depends on count alone and every sum runs in a fixed order: two calls give the same bits.  workspace:
 * pgtg_ppo_expl_var_workspace_bytes() bytes, 8-byte aligned, contents irrelevant.  A NULL pointer, count == 0 or
 * above 2^40, a workspace not 8-byte or out not 4-byte aligned: PGTG_E_INVALID, nothing launched. */
int pgtg_ppo_expl_var_workspace_bytes(uint64_t* bytes);
int pgtg_ppo_expl_var(pgtg_handle* h, const float* values, const float* returns, uint64_t count, void* workspace,
                      float* out);
/* The train log of one update from the [minibatches][8] statistics rows its pgtg_ppo_grad calls wrote (one
 * launch, k_ppo_log, asynchronous on the handle's stream).  With run = stop_at's value where stop_at is given
 * and non-zero, else minibatches: the means over rows [0, run) of entropy, policy and value loss and of the clip
 * fraction; approx_kl's mean over the rows of the last run epoch only, [(run - 1) / per_epoch * per_epoch, run)
 * (SB3 resets that list per epoch); loss of row run - 1; epochs = (run - 1) / per_epoch + 1, SB3's _n_updates
 * increment; every mean an fp64 sum in row order, rounded to float32 once.  expl_var: pgtg_ppo_expl_var's out or
 * NULL (NaN).  minibatches == 0 gives NaNs and zeros.  stats or out NULL, stats not 16-byte aligned, out,
 * stop_at or expl_var not 4-byte aligned, per_epoch == 0, minibatches above 2^31: PGTG_E_INVALID, nothing
 * launched. */
typedef struct {
  uint32_t minibatches;      /* run */
  uint32_t epochs;
  uint32_t early_stop;       /* stop_at was set */
  uint32_t reserved;
  float entropy_loss, policy_gradient_loss, value_loss, clip_fraction, approx_kl, loss;
  float explained_variance, variance_ratio;
} PgtgPpoLog;
int pgtg_ppo_log(pgtg_handle* h, const float* stats, uint64_t minibatches, uint64_t per_epoch, const uint32_t* stop_at,
                 const float* expl_var, PgtgPpoLog* out);
/* perm[total] (device, int64) = a permutation of [0, total) that is a function of (total, seed, counter) alone
 * (one launch, k_ppo_perm, asynchronous on the handle's stream): an alternating Feistel network of six rounds
 * over ceil(log2 total) bits, round function the splitmix64 finaliser of pgtg_policy's uniform draw in a domain
 * of its own, cycle-walked into [0, total).  Every element is computed on its own: no sort, no atomics, no
 * dependence on the grid.  An element whose walk exceeds 64 steps (probability below 2^-64) is written as its own
 * index and sets the handle's error byte (element mod batch size) to -PGTG_E_DEVICE (pgtg_error_count).
 * pgtg_amd.rollout.permutation_reference restates it.  perm NULL or not 8-byte aligned, total == 0 or above
 * 2^38: PGTG_E_INVALID, nothing launched. */
int pgtg_ppo_perm(pgtg_handle* h, uint64_t total, uint64_t seed, uint64_t counter, int64_t* perm);
/* Policy evaluation with per-env episode quotas (new; ModularEvaluator.evaluate of pgtg/evaluator.py:284-339
 * for the batch, counted as SB3's evaluate_policy counts a vector env: env e contributes its first
 * quota_e = (n_episodes + e) / n episodes (integer division; the quotas sum to n_episodes), so short episodes
 * are not over-represented).  pgtg_eval_step is one launch of k_eval after a tick: per env e, in fp64 without
 * fused multiply-add,
 *   if cnt[e] < quota_e:
 *     ret[e] += r;  disc[e] += r * g[e];  g[e] *= gamma;  len[e] += 1            (r = reward[e])
 *     if terminated[e] | truncated[e]:
 *       k = cnt[e];  row k * n + e of the record arrays = {ret, disc, len, r, step, flags};  cnt[e] = k + 1
 *       ret[e] = disc[e] = 0;  g[e] = 1;  len[e] = 0
 * and open_rows[b] = the number of envs e in [256 b, 256 b + 256) with cnt[e] < quota_e afterwards (a plain
 * store per workgroup; no atomics).  An env at its quota is not touched again.  The caller owns every array
 * and starts an evaluation with ret = disc = 0, g = 1, len = cnt = 0; the record arrays are [Q][n] with
 * Q = ceil(n_episodes / n), episode slot major, and hold rows k < cnt[e] only.  flags: bit 0 terminated,
 * bit 1 truncated.  pgtg_eval_summary reduces the recorded episodes (rows k < cnt[e]) into *out_dev in four
 * launches (k_eval_reduce and k_eval_final, twice: the means first, then the squared deviations about them)
 * whose partition depends on n alone and whose sums run in a fixed order: the same records give the same bits
 * on any device.  workspace: pgtg_eval_workspace_bytes(n, n_episodes) bytes, 8-byte aligned, contents
 * irrelevant.  Both calls are asynchronous on the handle's stream.  A NULL pointer (pgtg_eval_summary does not
 * read reward, terminated, truncated, ret, disc, g, len or open_rows), n different from the handle's batch
 * size, n_episodes == 0, gamma outside [0, 1], or step, Q or Q * n beyond INT32_MAX, INT32_MAX and 2^60:
 * PGTG_E_INVALID with a message, nothing is launched. */
typedef struct {
  uint64_t n, n_episodes;          /* N envs (the handle's), episodes wanted over the batch */
  uint64_t step;                   /* s: the evaluation step this launch records as end_step */
  double gamma;
  const double*  reward;           /* [N] the step's outputs (PgtgOutputs.reward, terminated, truncated) */
  const uint8_t* terminated;
  const uint8_t* truncated;
  double* ret; double* disc; double* g;     /* [N] running undiscounted and discounted return, discount */
  int32_t* len; int32_t* cnt;               /* [N] running length, episodes recorded */
  double* rec_return; double* rec_discounted; int32_t* rec_length;        /* [Q][N] */
  double* rec_last_reward; int32_t* rec_end_step; uint8_t* rec_flags;     /* [Q][N] */
  int32_t* open_rows;              /* [ceil(N / 256)] */
} PgtgEval;
/* The recorded episodes.  std: the population standard deviation (numpy's std, ddof 0). */
typedef struct {
  uint64_t episodes, open_envs;                          /* open_envs: envs with cnt < quota */
  uint64_t terminated, truncated_only;                   /* counters 0 and 1 of ModularEvaluator */
  uint64_t last_reward_positive, last_reward_negative;   /* the win and loss of Evaluator.evaluate */
  uint64_t negative_discounted;                          /* counter 3 of ModularEvaluator */
  uint64_t length_sum;
  int32_t  length_min, length_max;                       /* INT32_MAX / 0 when episodes == 0 */
  double   return_mean, return_std;                      /* 0 when episodes == 0 */
  double   return_min, return_max;                       /* +INFINITY / -INFINITY when episodes == 0 */
  double   discounted_mean, discounted_std;
} PgtgEvalSummary;
int pgtg_eval_step(pgtg_handle* h, const PgtgEval* a);
int pgtg_eval_summary(pgtg_handle* h, const PgtgEval* a, PgtgEvalSummary* out_dev, void* workspace);
int pgtg_eval_workspace_bytes(uint64_t n, uint64_t n_episodes, uint64_t* bytes);
/* Re-emit the observation of every env into the bound outputs (after set_agent/add_car). */
int pgtg_observe(pgtg_handle* h);
/* Per-env uint64 digest of the car list into out_dev[N] (device; parity tests: the car term of
 * pgtg_amd/digest.py).  Traffic handles only.  Asynchronous on the handle's stream. */
int pgtg_car_digest(pgtg_handle* h, uint64_t* out_dev);
/* steps (env-steps executed) and episodes (resets) since create, summed over envs; synchronises. */
int pgtg_get_counters(pgtg_handle* h, uint64_t* env_steps, uint64_t* episodes);
/* Map-queue ring entries generated since create (k_qfill after resets + the step launches' helper
 * waves; 0 for handles without the queue): a window's delta beside its episode delta shows that the
 * maps the episodes consumed were generated in the window.  Synchronises. */
int pgtg_get_queue_maps(pgtg_handle* h, uint64_t* maps);
/* Step-kernel launches since create: one per pgtg_step, and per pgtg_step_many one per tick or, where it runs
 * several ticks in a launch, one per such launch.  Host counter, no synchronisation. */
int pgtg_get_step_launches(pgtg_handle* h, uint64_t* launches);
/* Tuning and testing, beside PgtgConfig.tune_queue_grid: the block shares of the multi-tick step launches of a
 * k_envq handle.  Workgroup w of the queue grid owns counts[w] consecutive blocks (of envs-per-workgroup envs
 * each), workgroup 0 from block 0 on.  By default every such launch of two ticks or more re-derives the counts
 * on the device from the workgroups' measured time per block; results never depend on them.
 * pgtg_set_block_shares: counts == NULL keeps the table; otherwise n must be the queue grid, the counts must sum
 * to the handle's blocks and none may exceed what a workgroup's request list holds (three times the equal
 * share, rounded up), else PGTG_E_INVALID.  freeze != 0 stops the device from updating them, 0 resumes it.
 * pgtg_get_block_shares: the queue grid into *grid (if not NULL) and, if counts is not NULL, the current counts
 * (n must be the queue grid).  Both synchronise. */
int pgtg_set_block_shares(pgtg_handle* h, const uint32_t* counts, uint32_t n, int32_t freeze);
int pgtg_get_block_shares(pgtg_handle* h, uint32_t* counts, uint32_t n, uint32_t* grid);
/* Map-queue refill requests served from the overflow lists since create (step launches of one round
 * of workgroups list at most 64 requests per workgroup; the rest go to lists shared by residue mod 8
 * and are served by other workgroups' helper waves in the next launch).  Synchronises. */
int pgtg_get_queue_overflow(pgtg_handle* h, uint64_t* served);
/* Number of envs whose last step reported an error (PGTG_E_DONE / PGTG_E_MAP); synchronises. */
int pgtg_error_count(pgtg_handle* h, uint64_t* n_errors, int32_t* first_code);
/* Measured HBM denominator of the roofline: a 16-B/lane stream copy of `bytes` between two device
 * buffers on `device`, `reps` timed passes; *copy_gbs = (read + write bytes) / s / 1e9.  Synchronises. */
int pgtg_measure_hbm(int32_t device, uint64_t bytes, int32_t reps, double* copy_gbs);
int pgtg_window(const pgtg_handle* h);
uint64_t pgtg_num_envs(const pgtg_handle* h);
/* Launch geometry of the step kernel: envs per 256-lane workgroup and dynamic LDS bytes. */
int pgtg_launch_info(const pgtg_handle* h, int32_t* envs_per_block, int32_t* lds_bytes);
/* Resident workgroups per CU of the step kernel this handle launches (HIP occupancy query). */
int pgtg_occupancy(const pgtg_handle* h, int32_t* step_blocks_per_cu);
/* Name of the kernel(s) one pgtg_step launches for this handle (measurement labels). */
const char* pgtg_step_kernel(const pgtg_handle* h);
const char* pgtg_last_error(const pgtg_handle* h);
/* Per-launch device timing of the step kernels with HIP events on the handle's stream.  every > 0:
 * every every-th pgtg_step brackets its kernels with an event pair (1: all; 0: off);
 * pgtg_timing_read synchronises and returns the summed milliseconds of the bracketed launches and
 * their number (reset=1 clears the tally). */
int pgtg_enable_timing(pgtg_handle* h, int32_t every);
int pgtg_timing_read(pgtg_handle* h, double* total_ms, uint64_t* launches, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* PGTG_H_ */
