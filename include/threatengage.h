/*
 * threatengage.h — C ABI of the batched threat-engagement drone environment
 * (MI355X / gfx950 HIP implementation: dronechase_amd/libthreatengage.so).
 *
 * The reference (DaviGuanabara/dronechase) has no FFI: every environment is a
 * Python gymnasium.Env driven one-process-per-env through SB3's SubprocVecEnv
 * (src/core/rl_framework/utils/pipeline.py:31-61).  This header CREATES the
 * seam: one `te_env` replaces N reference environments
 * (src/threatengage/environments/level4/exp03_vFinal_environment.py:42-171 and
 * siblings) and each entry point names the reference interface it stands for.
 *
 * Conventions
 *   - plain C, no torch/HIP types in signatures; every I/O pointer is a DEVICE
 *     pointer (hipMalloc'ed or a PyTorch-ROCm tensor's data_ptr()) unless the
 *     name ends in `_host`.
 *   - all functions return 0 on success, non-zero on failure; the message is
 *     available from te_last_error() (thread-local, never NULL).
 *   - work is enqueued on `stream` (a hipStream_t passed as void*, NULL = the
 *     null stream) and is asynchronous; the caller synchronises.
 *   - a te_env is not thread-safe; distinct te_envs (e.g. one per GPU) are
 *     independent (mirrors the thread-local singletons of the reference,
 *     level4/components/entities_management/entities_manager.py:24-30).
 */
#ifndef THREATENGAGE_H
#define THREATENGAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TE_ABI_VERSION 5   /* layout of te_config / the state blob.  Added since without a layout change: the task presets 10-12, TE_REWARD_L5_C1,
                              bit 1 of te_config.evaluation (TE_EVAL_ORIGIN_RULE), te_drive_wingman_bf16, te_policy_adam_step_bf16, te_policy_ppo_epoch */

/* ---- tasks (reference env class each one mirrors) ----------------------- */
enum {
  TE_TASK_STAGE01 = 1, /* level2/pyflyt_level2_environment_modified_v2.py (apps stage01) */
  TE_TASK_STAGE02 = 2, /* level3/pyflyt_level3_environment_v2.py + components/stages.py (apps stage02) */
  TE_TASK_EXP02 = 3,   /* level4/exp02_vFinal_environment.py + tasks/exp02_vFinal_task.py */
  TE_TASK_EXP03 = 4,   /* level4/exp03_vFinal_environment.py + tasks/exp03_vFinal_task.py (apps stage03) */
  TE_TASK_EXP04 = 5,   /* level4/exp04_vFinal_environment.py (ally frozen, x10 approach bonus) */
  TE_TASK_LEVEL5 = 6,  /* threatsense/level5/level5_envrionment.py + tasks/level5_task.py: the exp03 task with 6 pursuers,
                          12 invaders and the FusedLIDAR stacked-sphere observation (te_step_stacked) */
  TE_TASK_EXP05 = 7,   /* level4/exp05_vFinal_environment.py + tasks/exp05_vFinal_task.py: exp03 with the ally driven by a
                          second policy (drive_lw_rl_agent, :252-260): te_observe_ally / te_set_ally_actions */
  TE_TASK_LEVEL5_DUMB = 9, /* threatsense/level5/level5_dumb_multiobs.py + tasks/level5_dumb_multiobject_task.py: the imitation-data
                          collector's environment — 7 wingmen ALL flown by the behaviour tree (the agent too, :256-266), 30 invader slots
                          of which min(4 + round, 30) are armed in a round (:173-184), 26 rounds, its own reward (:452-553) and
                          termination (:555-612); the observation is the stacked one of EVERY armed wingman (te_step_students) */
  TE_TASK_LEVEL5_2BT = 10, /* threatsense/level5/level5_eval_2bt_environment.py + tasks/level5_2bt_evaluation_task.py: two wingmen, both flown by
                          the behaviour tree (:256-261), against the 30-slot invader table of the level5 fusion tasks (5 in round 1, one more
                          per round, 26 rounds); Evaluation_Task-style rules (cfg.evaluation = TE_EVAL_ON | TE_EVAL_ORIGIN_RULE): reward 0
                          (:421-428), a fixed limit of 1 300 steps (:111), kills counted per wingman (:127-134,408-409; te_wingman_info);
                          the environment returns no observation (level5_eval_2bt_environment.py:27-33,53-56) */
  TE_TASK_LEVEL5_C1 = 11, /* threatsense/level5/level5_c1_fusion_environment.py + tasks/level5_c1_fusion_task.py: the RL agent and ONE scripted wingman
                          against 10 invader slots (4 in round 1, one more per round, 7 rounds; munition 49), the stacked observation of level5
                          (te_step_stacked) and the task's minimal reward (cfg.reward_model = TE_REWARD_L5_C1) */
  TE_TASK_LEVEL5_FUSION = 12, /* threatsense/level5/level5_fusion_environment.py + tasks/level5_fusion_task.py: the RL agent + 5 scripted wingmen
                          against 30 invader slots, FIVE more per round (5, 10, ... 30: 6 rounds; munition 105), Level5DumbMultiObjectTask's reward
                          (the two compute_reward bodies are the same text) with the agent's death ending the episode; 36 drones per env: the
                          stacked observation through te_step_stacked / te_observe_stacked (te_observe serves at most 32) */
  TE_TASK_EVALUATION = 8 /* level4/evaluation_environment.py + tasks/evaluation_task.py with behaviour-tree drivers only
                          (apps/threatengage_runner/stage03/experiments/01/evaluation_exp01_1bt_app_ready.py): cfg.evaluation = 1,
                          n_pursuers = number of drivers (default 1) */
};

/* ally (pursuer slots >= 1) policy: nobody (the set-point persists), LoyalWingmanBehaviorTree, drive([0,0,0,1]) every
 * step (exp04), or the caller through te_set_ally_actions (exp05; n_pursuers must be 2, exp05_vFinal_task.py:103) */
enum { TE_ALLY_NONE = 0, TE_ALLY_BT = 1, TE_ALLY_FROZEN = 2, TE_ALLY_EXTERNAL = 3 };
enum { TE_EVAL_ON = 1, TE_EVAL_ORIGIN_RULE = 2 };   /* te_config.evaluation, bits 0 and 1 */

/* kamikaze FSM states (core/entities/navigators/loitering_munition_navigator_air_combat_only.py:138-246) */
enum { TE_NAV_WAIT = 0, TE_NAV_COLLIDE_WINGMAN = 1, TE_NAV_COLLIDE_BUILDING = 2 };

/* entity types; LIDAR flag = type / 5 (core/entities/entity_type.py:4-14, lidar_math.py:305) */
enum { TE_TYPE_LOITERINGMUNITION = 1, TE_TYPE_QUADCOPTER = 2, TE_TYPE_LOYALWINGMAN = 3,
       TE_TYPE_PROTECTED_BUILDING = 4, TE_TYPE_GROUND = 5 };

/* ---- LIDAR grid (core/dataclasses/angle_grid.py:28-37, resolution 16) --- */
#define TE_LIDAR_NTHETA 13
#define TE_LIDAR_NPHI 26
#define TE_LIDAR_CELLS (TE_LIDAR_NTHETA * TE_LIDAR_NPHI) /* 338 */
#define TE_LIDAR_CHANNELS 3                              /* distance, flag, time (core/enums/channel_index.py:7-9) */
#define TE_OBS_LIDAR_WORDS (TE_LIDAR_CHANNELS * TE_LIDAR_CELLS) /* 1014 */
#define TE_OBS_INERTIAL_WORDS 15 /* pos3 vel3 att3 rate3 gun3 (exp03_vFinal_environment.py:200-228) */
#define TE_OBS_ACTION_WORDS 4
#define TE_INFO_WORDS 4 /* agent_kills, allies_kills, deads, current_wave (exp03_vFinal_task.py:571-578) */

/* ---- FusedLIDAR stacked observation (level5; fused_lidar.py:73-109,223-326, lidar_buffer.py:10-157) ----
 * own sphere + up to n_neighbors_max re-projected neighbour spheres, padded to TE_STACK_SPHERES, shuffled. */
#define TE_RING_DEPTH 10        /* snapshots kept per wingman (base_lidar.py:40: max_buffer_size=10) */
#define TE_STACK_NEIGHBORS_MIN 1
#define TE_STACK_NEIGHBORS_MAX 5 /* n ~ random.choice(range(1, 5)) = 1..4 neighbours (fused_lidar.py:77) */
#define TE_STACK_SPHERES 6      /* n_neighbors_max + 1 (fused_lidar.py:305) */
#define TE_OBS_STACKED_WORDS (TE_STACK_SPHERES * TE_OBS_LIDAR_WORDS) /* 6084 floats = 24 336 B per env */
/* one ring entry = one wingman's PerceptionSnapshot of one step: 12 header words + 4 per kept feature */
#define TE_RING_HEADER_WORDS 12 /* [0] i32 step stamp (0 = empty)  [1] i32 n_features  [2..4] position  [5..8] quaternion xyzw  [9..11] 0 */
#define TE_RING_FEATURE_WORDS 4 /* r_hat, theta, phi (own frame of the publisher), i32 entity type | publisher slot << 8 */
#define TE_RING_ENTRY_WORDS(D) (TE_RING_HEADER_WORDS + TE_RING_FEATURE_WORDS * ((D) - 1))

/* ---- quadrotor model: PyFlyt 0.11.1 QuadX "cf2x" + Bullet free body ------
 * The sources of these numbers (pyflyt 0.11.1, pybullet 3.2.7; poetry.lock:1412-1440)
 * are NOT in the reference tree; te_config_default() fills the table recorded in
 * SURVEY.md Appendix B (UNVERIFIED) so it can be corrected in one place. */
typedef struct te_quad_params {
  float mass;          /* kg */
  float inertia[3];    /* diag(Ixx, Iyy, Izz) kg m^2 */
  float arm;           /* |x| = |y| of each propeller, m */
  float total_thrust;  /* N at throttle 1 on all four motors */
  float thrust_coef;   /* N / rpm^2 */
  float torque_coef;   /* N m / rpm^2 */
  float motor_tau;     /* s, first-order lag */
  float noise_ratio;   /* multiplicative Gaussian throttle noise */
  float drag_coef_xyz, drag_area_xyz, drag_coef_pqr;
  float air_density;
  float gravity;       /* m/s^2, applied along -z (level4_simulation.py:69-70) */
  float ang_vel_kp[3], ang_vel_ki[3], ang_vel_kd[3], ang_vel_lim[3];
  float ang_pos_kp[3], ang_pos_lim[3];   /* ki = kd = 0 in cf2x: loop is memory-less */
  float lin_vel_kp[2], lin_vel_ki[2], lin_vel_kd[2], lin_vel_lim[2];
  float lin_pos_kp[2], lin_pos_lim[2];   /* mode 7 only; ki = kd = 0 */
  float z_pos_kp, z_pos_lim;             /* mode 7 only; ki = kd = 0 */
  float z_vel_kp, z_vel_ki, z_vel_kd, z_vel_lim;
  float pwm_floor;     /* 0.05: minimum pwm after saturation handling */
} te_quad_params;

/* ---- configuration ----------------------------- */
typedef struct te_config {
  uint32_t struct_size;   /* = sizeof(te_config); checked by te_create */
  int32_t task;           /* TE_TASK_* */
  int32_t n_envs;         /* environments owned by this te_env (this GPU's shard) */
  int32_t n_pursuers;     /* P; slot 0 is the RL agent */
  int32_t n_invaders;     /* I */
  int64_t env_index_base; /* global index of local env 0: RNG is keyed on the GLOBAL env index, so
                             results do not depend on how envs are sharded over GPUs */
  uint64_t seed;

  float dome_radius;      /* 20 (level4), 10 (stage01), 8 (stage02) */
  float lidar_radius;     /* 2 * dome_radius */
  float max_speed;        /* 10 km/h = 2.7778 m/s: observation normaliser only (quadcopter.py:590-600) */

  int32_t substeps;       /* physics sub-steps per env.step: 8 sim steps x 2 (level4_simulation.py:84-98) = 16.
                             0 (with observe_lag = 0) = no physics: the step's task logic alone, on the state as loaded */
  float physics_dt;       /* 1/240 */
  float control_dt;       /* 1/120: PID period, although update_control runs every sub-step (reference quirk) */
  int32_t observe_lag;    /* 1: IMU is read before the last integration */

  float shoot_range, explosion_range, origin_range, hit_prob;
  int32_t cooldown_steps; /* 4 s / (1/15 s) = 60 (gun.py:25) */
  int32_t munition;       /* per pursuer (20 in exp02/03; 4 for the stage02 agent; 0 in stage01) */
  int32_t max_step;       /* 300 (level4, stage01), 600 (stage02) */
  int32_t step_increment; /* +100 per step with >= 1 successful shot (exp03_vFinal_task.py:150-153) */
  int32_t n_rounds;       /* waves; = calculate_rounds(P, munition) (exp03_vFinal_task.py:198-226) */
  float born_radius;      /* 6 */
  float born_min_z;       /* 4 */
  float pursuer_spawn_radius; /* 2 (level4), 1 (stage02) */
  float invader_speed;    /* 0.4 kamikaze (…air_combat_only.py:58); 0.5 hover magnitude in stage02 */
  float ally_speed;       /* 0.6 (loyalwingman_navigator.py:37) */
  int32_t ally_policy;    /* TE_ALLY_* */
  float approach_bonus_gain; /* 1 (exp02/03), 10 (exp04, stage01, stage02) */
  float catch_distance;   /* stage01: 0.4 */
  float building_position[3]; /* (0,0,0.1) */

  int32_t motor_noise;    /* 0/1 */
  int32_t auto_reset;     /* 1: VecEnv semantics (reset inside step when done) */
  int32_t kamikaze_cone_check; /* 0: air-combat-only navigator (_is_building_path_clear == False, used by every
                                  vFinal task); 1: cone test of loitering_munition_navigator.py:78-87 */
  int32_t stacked_obs;    /* 1: keep the per-wingman snapshot ring and serve te_step_stacked (level5) */
  int32_t evaluation;     /* bit 0 (TE_EVAL_ON) = 1: Evaluation_Task rules (tasks/evaluation_task.py): EVERY pursuer is flown by the behaviour tree
                             (drivers of type "bt", :257-275,655-668; te_step's actions are ignored), reward 0 (:508-515), no
                             invaders-in-origin rule (:397), termination = time limit only if max_step > 0 (TIME_IS_LIMITED,
                             :519-524), all rounds over, anybody outside the dome, all pursuers destroyed (:526-551); kills are
                             counted per wingman (TE_D_KILLS) for te_wingman_info.  Bits 8.. : mask of the pursuers whose driver
                             is the CALLER's instead of the behaviour tree (drivers of type "nn", :264-268): bit 8 + p set =
                             pursuer p is observed with te_observe_wingman and commanded with te_set_wingman_actions 
                             Bit 1 (TE_EVAL_ORIGIN_RULE): invaders that reach the origin are still removed (Level52BTEvaluationTask.on_step_middle,
                             level5_2bt_evaluation_task.py:328; Evaluation_Task has that call commented out). */
  int32_t ground_contact; /* 1: ground plane (OPT-IN, off in every preset; parity unpinned): the reference loads plane.urdf at
                             z = -6 (entities_manager.py:120-124, immovable_structures.py:123-135); a drone whose hull bottom
                             reaches it stops there: inelastic normal contact (Bullet's default restitution 0) and Coulomb
                             friction 0.5 on the tangential velocity; no contact torque, no drone-drone contact */
  float ground_z;         /* -6 */
  float hull_half_height; /* 0.0125: half of the cf2x collision cylinder's height (unverified) */

  /* ---- SURVEY.md Appendix A.7 switches (ABI 4) ---- */
  int32_t control_every_substep; /* 1 (every preset): QuadX.update_control runs on EVERY physics sub-step, as the reference's
                             simulation loop calls it (level4_simulation.py:92-94), with the PID period still control_dt;
                             0: PyFlyt-native, update_control on every (physics_hz / ctrl_hz)-th sub-step only (120 Hz), the
                             motors keep the last pwm in between */
  int32_t lidar_channels; /* 3 (distance, flag, time: FusedLIDAR own sphere); 2 = the legacy LIDAR's layout
                             (distance, flag) that the level2-4 docs and the level5 teacher space quote
                             (sensors/lidar.py:137-145, level5_envrionment.py:79-84): obs_lidar is [N,2,13,26] */
  int32_t io_location;    /* TE_IO_DEVICE (0): every I/O pointer is a device pointer.  TE_IO_HOST (1): the actions, observation,
                             reward, done, info and terminal pointers of te_step / te_observe and te_reset's mask are HOST
                             pointers (what a SubprocVecEnv caller holds); the library stages them through device buffers of
                             its own with hipMemcpyAsync on the call's stream and the call returns when they have landed */
  int32_t drone_contact;  /* 1: drone-drone contact (OPT-IN, off in every preset; parity unpinned): armed drones collide as
                             spheres of contact_radius (Bullet narrow phase with the cf2x collision shapes; group/mask 1/1
                             for armed drones only, quadcopter.py:484-496): inelastic impulse along the line of centres at
                             the end of each sub-step, equal masses, no friction, no contact torque */
  float contact_radius;   /* 0.06: radius of the cf2x collision cylinder (unverified) */
  /* ---- round rule and the switches Level5DumbMultiObjectTask needs (ABI 5) ---- */
  int32_t initial_invaders;   /* 1: invaders armed in round r = min((r - 1) * invaders_per_round + initial_invaders, n_invaders): */
  int32_t invaders_per_round; /* 1:   Task.setup_round arms `round` of them (exp03_vFinal_task.py:180-196); the dumb multi-object task
                                 starts with 5 (level5_dumb_multiobject_task.py:87-90,173-184) */
  int32_t agent_scripted;     /* 1: pursuer 0 obeys the behaviour tree like the other wingmen and te_step's actions are ignored
                                 (level5_dumb_multiobject_task.py:256-266; implied by cfg.evaluation) */
  int32_t reward_model;       /* TE_REWARD_EXP03 (0): exp03_vFinal_task.py:423-515; TE_REWARD_L5_DUMB (1): level5_dumb_multiobject_task.py:452-553
                                 (reload-distance shaping, weighted kills / deaths, bounded border term, clipped to +-3000) 
                                 TE_REWARD_L5_C1 (2): Level5C1FusionTask.compute_reward (level5_c1_fusion_task.py:448-485): 10 |v| while the agent is closer to
                                 ITS closest invader than at the FIRST reward of this te_env's env (`self.last_distance` is set once and never
                                 again, not even by a reset: TE_E_LAST_DIST holds it, 0 = not measured yet), + 1000 per agent kill, - 2000 for
                                 the agent's suicide, clipped to +-3000 */
  int32_t agent_death_terminates; /* 1: the episode ends when pursuer 0 is disarmed (training tasks, exp03_vFinal_task.py:556-561);
                                 0: it goes on (level5_dumb_multiobject_task.py:600-606 has the test commented out) */
  int32_t quad_preset;    /* which table te_config_default / te_quad_preset filled `quad` with: TE_QUAD_CF2X_RECALLED (0) or
                             TE_QUAD_CF2X_RECORDED_FIT (1).  Informational: the kernels read `quad` only */

  te_quad_params quad;
} te_config;

enum { TE_IO_DEVICE = 0, TE_IO_HOST = 1 };
enum { TE_REWARD_EXP03 = 0, TE_REWARD_L5_DUMB = 1, TE_REWARD_L5_C1 = 2 };
/* quadrotor parameter presets (te_quad_preset).  RECALLED = PyFlyt 0.11.1's cf2x.yaml / cf2x.urdf as recalled in SURVEY.md
 * Appendix B (the default until round 2; chi^2 / dof 5.3 against the recording below); RECORDED_FIT = the same table with the
 * fewest changed entries (ang_vel_kp roll / pitch x 6, motor_tau x 0.4) that reproduce the only PyBullet-made numbers in the
 * reference tree (io_data0.h5: seven wingmen, two steps after a respawn) within their motor-noise scatter (chi^2 / dof 0.29) —
 * THE DEFAULT OF EVERY TASK since round 3; see DESIGN.md 5 and tools/physics_fit.py.  Neither is verified against the PyFlyt sources, and
 * the recording does not single the fit out: scored in units of its own (smaller) motor-noise scatter it reaches chi^2 / dof 2.8, and other
 * candidates (e.g. 120 Hz control with ang_pos_kp x 2 and total_thrust x 2) fit the 147 numbers as well or better.  One of several tables
 * the data support; parity with PyBullet is unpinned under either preset. */
enum { TE_QUAD_CF2X_RECALLED = 0, TE_QUAD_CF2X_RECORDED_FIT = 1 };

/* ---- state blob (te_get_state / te_set_state) ----------------------------
 * Env-major array of 4-byte words: for env e,
 *   drone d (0..D-1, pursuers first): TE_DRONE_WORDS words at (e*D + d)*TE_DRONE_WORDS
 *   then, after all N*D drone records, env record e: TE_ENV_WORDS words.
 * Words are float32 unless marked i32 (raw two's complement int32). */
enum {
  TE_D_POS = 0,        /* 3  world position */
  TE_D_QUAT = 3,       /* 4  x,y,z,w (Bullet convention) */
  TE_D_VEL = 7,        /* 3  world linear velocity */
  TE_D_OMEGA = 10,     /* 3  world angular velocity */
  TE_D_THROTTLE = 13,  /* 4  motor throttles */
  TE_D_PID_AV_I = 17,  /* 3  angular-velocity PID integral */
  TE_D_PID_AV_E = 20,  /* 3  angular-velocity PID previous error */
  TE_D_PID_LV_I = 23,  /* 2  linear-velocity PID integral */
  TE_D_PID_LV_E = 25,  /* 2  linear-velocity PID previous error */
  TE_D_PID_ZV_I = 27,  /* 1 */
  TE_D_PID_ZV_E = 28,  /* 1 */
  TE_D_SETPOINT = 29,  /* 4  [vx, vy, vr, vz] (mode 6) or [x, y, r, z] (mode 7) */
  TE_D_OBS_POS = 33,   /* 3  last IMU read: position (imu.py:27-41) */
  TE_D_OBS_EULER = 36, /* 3  roll, pitch, yaw */
  TE_D_OBS_VEL = 39,   /* 3  body-frame linear velocity */
  TE_D_OBS_RATE = 42,  /* 3  body-frame angular velocity */
  TE_D_FORMATION = 45, /* 3  last replace() position (quadcopter.py:437) */
  TE_D_PENDING = 48,   /* 6  world force(3)+torque(3) applied outside the loop, consumed by the next
                             integration (stage01 replace_invader, level2/components/quadcopter_manager.py:166-179) */
  TE_D_ALLY_ACTION = 48, /* 4  the same words of a CALLER-DRIVEN pursuer (pursuer 1 under TE_ALLY_EXTERNAL, the pursuers of
                             cfg.evaluation's driver mask; no level4 drone has a pending wrench):
                             the ally policy's previous action, Exp05_vFinal_Task.last_action (exp05_vFinal_task.py:139,259) */
  TE_D_ARMED = 54,     /* i32 */
  TE_D_MUNITION = 55,  /* i32 */
  TE_D_LAST_FIRED = 56,/* i32 */
  TE_D_NAV_STATE = 57, /* i32 TE_NAV_* (invaders) */
  TE_D_KILLS = 57,     /* i32 the same word of a PURSUER under cfg.evaluation: Evaluation_Task.lw_kills of this episode
                             (evaluation_task.py:498-499); 0 otherwise */
  TE_DRONE_WORDS = 58
};
enum {
  TE_E_STEP = 0,         /* i32 RL step counter of the episode */
  TE_E_MAX_STEP = 1,     /* i32 */
  TE_E_ROUND = 2,        /* i32 current wave */
  TE_E_LAST_DIST = 3,    /* f32 last_closest_distance (level4) / last_distance (stage01) */
  TE_E_AGENT_KILLS = 4,  /* i32 */
  TE_E_ALLIES_KILLS = 5, /* i32 */
  TE_E_DEADS = 6,        /* i32 */
  TE_E_SNAP_MASK = 7,    /* i32 bit d = drone d was armed when the offsets were last computed
                                (level4/components/entities_management/offsets_handler.py:68-95) */
  TE_E_EPISODE = 8,      /* i32 episode counter (RNG stream selector) */
  TE_E_LAST_ACTION = 9,  /* 4 f32 */
  TE_E_PREV_SNAP_MIN = 13, /* f32 stage02: last_closest_pursuer_to_invader_distance */
  TE_E_INFO_WAVE = 15,   /* i32 the wave as the step's compute_info saw it: BEFORE on_step_end may have started the next one (the environments read
                            info between on_step_middle and on_step_end, evaluation_environment.py:178-186); te_wingman_info reports this */
  TE_E_SNAP_MASK_HI = 14,/* i32 bits 32..63 of the snapshot mask (more than 32 drones per env: TE_TASK_LEVEL5_DUMB has 37) */
  TE_ENV_WORDS = 16
};

typedef struct te_env te_env; /* opaque */

/* Fill `cfg` with the reference constants of `task` (n_envs = 1, seed = 0).
 * Mirrors Task.init_constants (exp03_vFinal_task.py:88-112, level3/components/stages.py:65-83,
 * level2/pyflyt_level2_environment_modified_v2.py:27-47). */
int te_config_default(te_config* cfg, int32_t task);

/* Overwrite cfg->quad (and cfg->quad_preset) with one of the TE_QUAD_* tables. */
int te_quad_preset(te_config* cfg, int32_t preset);

/* Task.calculate_rounds (exp03_vFinal_task.py:198-226): the number of waves (= invader slots) `defenders` pursuers with
 * `munition` rounds each can clear; what te_config_default puts into n_rounds / n_invaders. */
int te_calculate_rounds(int32_t defenders, int32_t munition);

/* Replaces N x `Env.__init__` (exp03_vFinal_environment.py:42-63): allocates HBM state for
 * cfg->n_envs environments on `device_id` and runs on_env_init + on_episode_start. */
int te_create(const te_config* cfg, int32_t device_id, te_env** out);
void te_destroy(te_env* env);

/* Replaces `Env.reset` (exp03_vFinal_environment.py:128-146) for every env whose
 * env_mask byte is non-zero (NULL = all).  env_mask is a device pointer of n_envs bytes. */
int te_reset(te_env* env, const uint8_t* env_mask, void* stream);

/* Replaces `Env.compute_observation` (exp03_vFinal_environment.py:200-228) without stepping:
 * obs_lidar [N,3,13,26], obs_inertial [N,15], obs_last_action [N,4] (float32, device).
 * Immediately after te_create/te_reset the LIDAR plane is the empty sphere (all ones). */
int te_observe(te_env* env, float* obs_lidar, float* obs_inertial, float* obs_last_action, void* stream);

/* Replaces `VecEnv.step_async + step_wait` over N x `Env.step`
 * (exp03_vFinal_environment.py:150-171; SB3 auto-reset when cfg.auto_reset).
 *   actions        [N,4] float32 (direction xyz in [-1,1], magnitude in [0,1])
 *   reward [N] f32, done [N] u8, info [N,4] i32
 *   terminal_*     may be NULL; rows are written ONLY for envs with done != 0
 *                  (SB3 infos[i]["terminal_observation"]). */
int te_step(te_env* env, const float* actions, float* obs_lidar, float* obs_inertial,
            float* obs_last_action, float* reward, uint8_t* done, int32_t* info,
            float* terminal_lidar, float* terminal_inertial, float* terminal_last_action,
            void* stream);

/* Level5 (cfg.stacked_obs = 1): the same step with the FusedLIDAR stacked observation of the agent instead of
 * its own sphere (threatsense/level5/level5_envrionment.py:312-351; fused_lidar.py:73-109,223-326):
 *   obs_stacked [N,6,3,13,26] f32 — own sphere, 1..4 re-projected neighbour snapshots of random age (farther
 *                wins), padded with empty spheres, then shuffled;   obs_mask [N,6] u8 — 1 = a valid sphere.
 * Every armed wingman's snapshot (pose + the features of its own sphere) is pushed into a 10-deep ring per step;
 * the ring is part of the state blob.  terminal_* as in te_step.  te_observe_stacked is te_observe's counterpart
 * (after a reset every sphere is empty and every mask byte 0: there is no snapshot yet).  Both serve up to 37 drones per env (P <= 7;
 * TE_TASK_LEVEL5_FUSION has 36); te_observe, the own-sphere observation, stops at 32.  Three launches after the sub-step kernel: the engage
 * kernel, then one wave per (64-env chunk, wingman) pushing this step's ring entries, then one 5-wave workgroup per chunk for the
 * observer's view (te_stackview.hpp). */
int te_step_stacked(te_env* env, const float* actions, float* obs_stacked, uint8_t* obs_mask, float* obs_inertial,
                    float* obs_last_action, float* reward, uint8_t* done, int32_t* info, float* terminal_stacked,
                    uint8_t* terminal_mask, float* terminal_inertial, float* terminal_last_action, void* stream);
int te_observe_stacked(te_env* env, float* obs_stacked, uint8_t* obs_mask, float* obs_inertial, float* obs_last_action,
                       void* stream);

/* Level5DumbMultiObs.step + compute_info (threatsense/level5/level5_dumb_multiobs.py:116-150): one env.step in which every wingman is
 * scripted, returning the STUDENT observation of every pursuer and the teacher's action for it (the collector keeps the rows of the armed
 * ones, apps/threatsense_runner/collect_and_save.py:99-127):
 *   stacked [N,P,6,3,13,26] f32, mask [N,P,6] u8, inertial [N,P,15] f32 (normalised IMU + gun state of pursuer p),
 *   last_action [N,P,4] f32 = the behaviour tree's command of this step (direction, magnitude: pursuer.last_action = the teacher's
 *   action), active [N,P] u8 = pursuer p is armed after the step (its row is one the reference emits); reward / done / info as te_step.
 * Needs cfg.stacked_obs and cfg.agent_scripted (or cfg.evaluation).  Envs that auto-reset come back with the reset observation (empty
 * spheres, zero masks); there are no terminal buffers (the collector has no use for them). */
int te_step_students(te_env* env, float* stacked, uint8_t* mask, float* inertial, float* last_action, uint8_t* active, float* reward,
                     uint8_t* done, int32_t* info, void* stream);

/* exp05 (cfg.ally_policy == TE_ALLY_EXTERNAL): the two halves of Exp05_vFinal_Task.drive_lw_rl_agent
 * (exp05_vFinal_task.py:252-260), which the reference runs in on_step_start, i.e. BEFORE the physics of a step:
 *   te_observe_ally      = compute_lw_observation (:265-292) of pursuer 1 on the CURRENT state: its own LIDAR sphere
 *                          ally_lidar [N,3,13,26], normalised inertial data + gun state ally_inertial [N,15], the ally
 *                          policy's previous action ally_last_action [N,4] (zeros after a reset); ally_active [N] u8 = 1
 *                          where the reference would call driver.predict (the ally is armed).  Any pointer may be NULL.
 *   te_set_ally_actions  = pursuer.drive(action) for every env whose ally is armed: ally_actions [N,4] f32 as te_step's
 *                          actions; remembered as the ally's last action.  Rows of envs with a dead ally are ignored.
 * One env.step of exp05 is therefore te_observe_ally -> (the caller's policy) -> te_set_ally_actions -> te_step. */
int te_observe_ally(te_env* env, float* ally_lidar, float* ally_inertial, float* ally_last_action, uint8_t* ally_active,
                    void* stream);
int te_set_ally_actions(te_env* env, const float* ally_actions, void* stream);
/* The same pair for ANY caller-driven pursuer `wingman`: pursuer 1 of exp05 (= the two calls above), or a pursuer whose bit
 * is set in cfg.evaluation's driver mask (Evaluation_Task.drive_lw with a driver that has `predict`,
 * evaluation_task.py:257-268, compute_lw_observation :281-310).  The last action is kept per wingman (the reference shares
 * one `self.last_action` between all "nn" drivers of an env, i.e. a wingman sees its predecessor's action: not restated). */
int te_observe_wingman(te_env* env, int32_t wingman, float* lidar, float* inertial, float* last_action, uint8_t* active, void* stream);
int te_set_wingman_actions(te_env* env, int32_t wingman, const float* actions, void* stream);
/* Exp05_vFinal_Task.drive_lw_rl_agent for caller-driven pursuer `wingman`, with the packed LidarInertialActionPolicy `params`
 * (te_policy_act's layout below, lidar_channels == cfg.lidar_channels) as the driver, deterministic:
 *   te_observe_wingman(wingman) into lidar [N][C][13][26] / inertial [N][15] / last_action [N][4] (caller-owned scratch, same
 *   alignment rules: lidar and last_action 16-byte aligned), then for every env whose pursuer `wingman` is armed:
 *   action = clamp(mu, [-1,1]^3 x [0,1]) and exactly what te_set_wingman_actions does with it (velocity command, set-point,
 *   remembered last action).  The env state afterwards is bitwise the one of te_observe_wingman -> te_policy_act (eps NULL)
 *   -> clamp -> te_set_wingman_actions.
 * mu (optional, [N][4], 4-byte aligned) receives the unclamped mean of every row, bitwise te_policy_act's.  params is 16-byte
 * aligned.  Enqueues on `stream` only (no allocation, no host synchronisation: a HIP graph can capture it); every argument
 * error returns before anything is launched. */
int te_drive_wingman(te_env* env, int32_t wingman, const float* params, int32_t lidar_channels, float* lidar, float* inertial,
                     float* last_action, float* mu, void* stream);
/* The same for a policy of any served shape (te_policy_shape below; shape->lidar_channels == cfg.lidar_channels, params in that
 * shape's packed layout).  te_drive_wingman is this call with the default shape. */
struct te_policy_shape;
int te_drive_wingman_shaped(te_env* env, int32_t wingman, const float* params, const struct te_policy_shape* shape, float* lidar,
                            float* inertial, float* last_action, float* mu, void* stream);

/* Evaluation_Task.compute_info (evaluation_task.py:553-574), cfg.evaluation only: wingman_info [N,P,5] i32 with the rows
 * (lw_kills, lw_alive, lw_munitions, current_wave, step) of every pursuer AFTER the last te_step (the reference lists the
 * armed pursuers only: a row with lw_alive == 0 is one it would omit).  For envs that auto-reset in that step the rows
 * describe the fresh episode; callers that want an episode's final rows read them with cfg.auto_reset = 0, as the
 * reference's evaluation loop does (evaluation_exp01_1bt_app_ready.py:80-96). */
int te_wingman_info(te_env* env, int32_t* wingman_info, void* stream);

/* Persistent observation (opt-in; no counterpart in the reference, whose sensors build a fresh numpy array every call,
 * fused_lidar.py:143-262).  on != 0: the caller promises that nobody but this library writes the LIDAR observation buffer it passes
 * (obs_lidar of te_step; obs_stacked of te_step_stacked / te_step_students / te_observe_stacked).  While the SAME pointer keeps coming, a
 * call rewrites only the cells that change (the cells the previous observation patched go back to 1, the new ones are patched) instead of
 * streaming the whole background; the buffer ends up bit for bit as the dense path leaves it.  A different pointer (e.g. the slots of a
 * rollout buffer) takes the dense path for that call.  Terminal buffers are always dense.  on == 0 (the default): every call is dense.
 * The algorithmic bytes of such a step are the cells it touches, not the background: bench.py keeps the dense path as its headline.
 * "The same buffer" is recognised by its ADDRESS alone: the caller must keep the allocation alive for as long as it passes it — a buffer
 * that is freed and whose memory is handed to a NEW allocation at the same address (a caching allocator does that) would be taken for the old
 * one and its background never written.  te_set_persistent_obs(env, 0) followed by (env, 1) forgets the remembered buffer: call it whenever
 * the buffer's identity changes.  Under cfg.io_location == TE_IO_HOST the persistent buffer is the library's own staging (the caller's host
 * array is filled from it every call); the terminal rows of done envs are compacted in a staging of their own. */
int te_set_persistent_obs(te_env* env, int32_t on);

/* Synthetic random-action generator of the throughput harness
 * (apps/threatengage_runner/interactive/analyse.py:55-59): dir ~ U(-1,1)^3, mag ~ U(0,1),
 * Philox4x32-10 keyed on (seed, global env index, step_index). */
int te_random_actions(te_env* env, float* actions, uint64_t seed, uint64_t step_index, void* stream);

/* Checkpoint / parity hooks (the reference never checkpoints env state). */
int te_state_words(const te_env* env, size_t* out_words);
int te_get_state(te_env* env, void* dst_device, size_t words, void* stream);
int te_set_state(te_env* env, const void* src_device, size_t words, void* stream);

/* Algorithmic HBM bytes one te_step moves per environment (SURVEY.md 8(d) formula). */
int te_algorithmic_bytes_per_env_step(const te_config* cfg, size_t* out_bytes);

/* The kernels te_create would choose for `cfg` under the current environment knobs, one "role=kernel" line each:
 * substeps, substeps_nofill (the sub-step kernel with and without the background's fill waves), engage, and for cfg.stacked_obs
 * ring_push (absent when stacked_kernel serves the observation) and stack_view.  Kernel names as rocprofv3 prints them, without
 * the namespace and the signature.  Needs no device; an invalid config fails with te_create's message.  (On a device that refuses
 * a multi-slot engage kernel more than 64 KB of LDS, te_create falls back to the form without it.)  out holds out_bytes bytes. */
int te_kernel_plan(const te_config* cfg, char* out, size_t out_bytes);

/* Kernel timing with HIP events on the stream te_step launches on.  After te_profile_begin the next
 * `max_steps` te_step calls launch their kernels with start / stop events (hipExtLaunchKernelGGL: the
 * dispatch's own begin / end timestamps, the quantity rocprofv3 --kernel-trace reports; TE_PROF=markers
 * in the environment selects marker packets between the launches instead); te_profile_end blocks until
 * they have finished and returns the average duration of the sub-step kernel and of the rest of the
 * step (engage kernel start to the end of the step's last kernel) in milliseconds, and how many steps
 * were recorded. */
int te_profile_begin(te_env* env, int32_t max_steps);
int te_profile_end(te_env* env, float* substeps_ms, float* engage_observe_ms, int32_t* n_steps);

/* Diagnostic builds only (-DTE_DEBUG_STAMPS): 100 MHz phase stamps of one workgroup of the last te_step;
 * zeros otherwise.  out_host is HOST memory. */
int te_debug_stamps(te_env* env, uint64_t* out_host, int32_t n);

/* Inference of the PPO policy (dronechase_amd/ppo.py LidarInertialActionPolicy; the reference's SB3 MultiInputPolicy with
 * LidarInertialActionExtractor, src/core/rl_framework/agents/policies/ppo_policies.py:234-341) in one launch, fp32.
 *
 * `params` is ONE packed device buffer of te_policy_param_words(lidar_channels) floats, 16-byte aligned: the module's parameters
 * in the registration order of its submodules, each flattened row-major as PyTorch stores it, then log_std:
 *   lidar.0.weight [32][C][4][4], lidar.0.bias [32], lidar.2.weight [64][32][2][2], lidar.2.bias [64],
 *   inertial.{0,2,4}.{weight,bias} ([128][15], [128], [128][128], [128], [128][128], [128]),
 *   action.{0,2,4}.{weight,bias} ([128][4], [128], then as inertial), final.0.weight [256][448], final.0.bias [256],
 *   pi.{0,2}.{weight,bias} ([64][256], [64], [64][64], [64]), vf.{0,2}.{weight,bias} (as pi),
 *   mu.weight [4][64], mu.bias [4], value.weight [1][64], value.bias [1], log_std [4].
 * C = lidar_channels (3, or 2 for the legacy LIDAR layout): 235 049 words for C = 3, 512 fewer for C = 2.
 *
 * te_policy_act: n rows of lidar [n][C][13][26] (8-byte aligned), inertial [n][15], last_action [n][4] -> mu [n][4], value [n].
 * With eps [n][4] (a standard-normal draw) it also samples: action = mu + exp(log_std) * eps (unclamped, what PPO stores),
 * logp [n] = sum_j (-eps_j^2 / 2 - log_std_j - log(2 pi) / 2), action_env = action clamped to [-1, 1]^3 x [0, 1] (what te_step
 * takes).  action, logp and action_env may be NULL when eps is NULL.  Rows are independent: a row's outputs do not depend on n
 * or on the other rows.  Enqueues on `stream` only (no allocation, no host synchronisation: a HIP graph can capture it); runs on
 * the current device. */
int te_policy_param_words(int32_t lidar_channels, size_t* out_words);
int te_policy_act(const float* params, int32_t lidar_channels, int32_t n, const float* lidar, const float* inertial,
                  const float* last_action, const float* eps, float* mu, float* value, float* action, float* logp,
                  float* action_env, void* stream);

/* The policy's shape: the trunk's width (final.0: Linear(448, features_dim)) and the widths of the heads' hidden layers,
 * hidden[0 .. n_hidden - 1], the same for pi and vf (the reference's net_arch = dict(pi = hiddens, vf = hiddens)); hidden[n_hidden ..]
 * is ignored.  The extractor below the trunk is fixed.  The kernels serve a closed list, for lidar_channels 2 and 3:
 *   features_dim 256, hidden 64, 64           SB3's defaults: the shape of te_policy_param_words / te_policy_act / te_drive_wingman
 *   features_dim 512, hidden 128, 256, 512    the reference's stage03 experiment apps (checkpoints named h[128, 256, 512])
 *   features_dim 512, hidden 512, 128, 256    the reference's stage03/auxiliary/learn.py
 * Any other shape is refused, never approximated: te_policy_shape_check returns non-zero and te_last_error names the offending
 * field and the served shapes (no device call).
 *
 * The packed layout of a shape is the rule above applied to its layers: for every layer in the module's registration order
 * (lidar.0, lidar.2, inertial.{0,2,4}, action.{0,2,4}, final.0, pi.{0,2,..}, vf.{0,2,..}, mu, value) the weight [N][K] row-major,
 * then the bias [N]; log_std [4] last.  final.0 is [features_dim][448]; pi.0 and vf.0 are [hidden[0]][features_dim], pi.(2 i) and
 * vf.(2 i) are [hidden[i]][hidden[i - 1]]; mu is [4][hidden[n_hidden - 1]] and value [1][hidden[n_hidden - 1]].
 * te_policy_param_words_shaped counts it: 771 561 words for the second shape and 1 032 425 for the third at lidar_channels 3.
 *
 * te_policy_act_shaped and te_drive_wingman_shaped are te_policy_act and te_drive_wingman for such a buffer: the same arguments,
 * checks, outputs and guarantees (rows independent, bitwise repeatable); with the default shape they are bitwise the unshaped calls. */
typedef struct te_policy_shape {
  int32_t lidar_channels, features_dim, n_hidden, hidden[4];
} te_policy_shape;
int te_policy_shape_check(const te_policy_shape* shape);
int te_policy_param_words_shaped(const te_policy_shape* shape, size_t* out_words);
int te_policy_act_shaped(const float* params, const te_policy_shape* shape, int32_t n, const float* lidar, const float* inertial,
                         const float* last_action, const float* eps, float* mu, float* value, float* action, float* logp,
                         float* action_env, void* stream);

/* te_policy_act_shaped with bf16 operands on the bf16 MFMA (v_mfma_f32_16x16x32_bf16), opt-in, for every served shape and
 * lidar_channels 2 and 3 (dronechase_amd/csrc/te_policy_bf16.hpp).  Numerics contract:
 *   - weights are rounded once to bf16, round-to-nearest-even, by te_policy_pack_bf16; the fp32 packed buffer stays the master copy;
 *   - the input of every weight layer is rounded to bf16 (round-to-nearest-even) where it is stored for the MFMA: the LIDAR patch,
 *     inertial_data, last_action, every hidden activation, the concat, the trunk, the head tiles and each head's last hidden tile;
 *   - products are accumulated in fp32 by the MFMA, the accumulator starting from the fp32 bias; ReLU and tanhf run in fp32 on the
 *     accumulator and the result is rounded when it is stored;
 *   - mu and value are fp32 fmaf sums, one thread per row, of the fp32 weights and bias over the bf16 last hidden tile;
 *   - log_std, the sample, logp and the clamp are te_policy_act's, in fp32;
 *   - a row's outputs do not depend on n or on the other rows, and repeated calls are bitwise equal.
 * The outputs therefore differ from te_policy_act_shaped's by bf16 rounding (measured: README).
 *
 * weights_bf16 is ONE device buffer of te_policy_bf16_words(shape) uint16 elements, 16-byte aligned: for every weight layer below mu
 * and value, in the order of the fp32 buffer (lidar.0, lidar.2, inertial.{0,2,4}, action.{0,2,4}, final.0, pi.{0,2,..},
 * vf.{0,2,..}), the weight [N][Kp] row-major as bf16 bit patterns, Kp = K rounded up to a multiple of 32, columns K .. Kp - 1 zero
 * (every row starts on a 64-byte boundary of the buffer).  Biases, mu, value and log_std are not in it: the call reads them from
 * `params`.  te_policy_pack_bf16 fills it from `params` (the fp32 packed buffer of the same shape) in one launch on `stream`, no host
 * synchronisation; call it again after every change of `params`.
 *
 * te_policy_act_bf16: the arguments, optional pointers, alignment rules and checks of te_policy_act_shaped, plus weights_bf16.  Every
 * argument error returns non-zero before any launch with te_last_error set; an unserved shape is refused with the served list.
 * Enqueues on `stream` only: a HIP graph can capture it. */
int te_policy_bf16_words(const te_policy_shape* shape, size_t* out_halfwords);
int te_policy_pack_bf16(const float* params, const te_policy_shape* shape, uint16_t* out, void* stream);
int te_policy_act_bf16(const float* params, const uint16_t* weights_bf16, const te_policy_shape* shape, int32_t n, const float* lidar,
                       const float* inertial, const float* last_action, const float* eps, float* mu, float* value, float* action,
                       float* logp, float* action_env, void* stream);

/* te_drive_wingman_shaped with te_policy_act_bf16's numerics, opt-in, for every served shape and lidar_channels 2 and 3: the contract,
 * arguments and checks of te_drive_wingman_shaped (above), plus weights_bf16, te_policy_pack_bf16's buffer for `params` (non-null, 16-byte
 * aligned).  The forward is te_policy_act_bf16's on its own tile, so mu (optional, every row) is bitwise te_policy_act_bf16's, and the env
 * state afterwards is bitwise the one of te_observe_wingman -> te_policy_act_bf16 (eps NULL) -> clamp -> te_set_wingman_actions.  The
 * clamp and the drive are te_drive_wingman's, in fp32.  Every argument error returns non-zero before any launch with te_last_error
 * starting "te_drive_wingman_bf16"; an unserved shape is refused with the served list.  Enqueues on `stream` only (no allocation, no
 * host synchronisation): a HIP graph can capture it. */
int te_drive_wingman_bf16(te_env* env, int32_t wingman, const float* params, const uint16_t* weights_bf16,
                          const struct te_policy_shape* shape, float* lidar, float* inertial, float* last_action,
                          float* mu, void* stream);

/* te_policy_ppo_grad_bf16: te_policy_ppo_grad_shaped (below) with bf16 operands on v_mfma_f32_16x16x32_bf16 and fp32 accumulation, for
 * every served shape and lidar_channels 2 and 3; opt-in, the fp32 calls are unchanged.  The loss, the arguments, grad (fp32, packed),
 * stats [4] = pg, vl, ent, clip_frac, the rows read through `index`, no host synchronisation, no float atomics, fixed sum orders and
 * graph capture are te_policy_ppo_grad_shaped's.  The numerics contract extends te_policy_act_bf16's:
 *   1. forward: bitwise te_policy_act_bf16's on the same row and weights (weights rounded once; every layer input rounded to bf16
 *      where it is stored; fp32 accumulation from the fp32 bias; mu and value fp32 fmaf sums over the bf16 last hidden tile).
 *   2. saved activations: the workspace holds every layer's input as the bf16 values the MFMA consumed.  ReLU's mask is y > 0 on the
 *      stored bf16 output y; tanh' is 1 - y^2 with that y, computed in fp32.
 *   3. loss: the per-row loss and its derivatives are te_policy_ppo_grad's, in fp32 (the tie split of min, the closed clamp
 *      interval, adv_mean_std).
 *   4. dZ: every pre-activation gradient is computed in fp32 from the MFMA accumulator and rounded ONCE to bf16 (nearest-even) where
 *      it is stored; the next dX, dW, db and the vector-ALU step from dmu / dv into the last hidden layer read the rounded value.
 *      dmu and dv count as dZ.  The trunk's dZ is one accumulator over both heads.  log_std's per-row gradient and the four
 *      statistics are not dZ of a GEMM: fp32 end to end.
 *   5. dX = dZ W with the bf16 weights (weights_bf16_t); into the last hidden layer of a head with the fp32 mu / value weights.
 *   6. dW = dZ^T [X | 1]: bf16 operands, fp32 accumulation, split-K slices of 2 048 reduction rows, fp32 partials summed slice by
 *      slice in order.  The gradient is with respect to the fp32 master weights: the weight rounding is straight-through.
 *   7. repeated calls are bitwise equal; `index` equals pre-gathered rows bitwise; rows past n contribute exactly 0, whatever the
 *      workspace held.
 * weights_bf16: te_policy_pack_bf16's buffer.  weights_bf16_t: a second uint16 buffer of te_policy_bf16_grad_words(shape) elements,
 * 16-byte aligned, filled by te_policy_pack_bf16_grad from `params` in one launch (again after every change of `params`): per layer
 * whose input needs a gradient (every layer of te_policy_pack_bf16's buffer except conv1, inertial.0 and action.0), in the same
 * order, the transposed weight W^T [K][Np], Np = roundup(N, 32), columns N .. Np - 1 zero.
 * workspace: 256-byte aligned, at least te_policy_grad_bf16_workspace_bytes(shape, n) bytes (about half the fp32 call's).  n <= 2^27.
 * Null pointers, alignment (params, grad and both bf16 buffers 16 bytes; lidar and index 8; workspace 256; float arrays 4), a short
 * workspace, clip_range and an unserved shape are refused before any launch, with te_last_error set. */
int te_policy_bf16_grad_words(const te_policy_shape* shape, size_t* out_halfwords);
int te_policy_pack_bf16_grad(const float* params, const te_policy_shape* shape, uint16_t* out, void* stream);
int te_policy_grad_bf16_workspace_bytes(const te_policy_shape* shape, int32_t n, size_t* out_bytes);
int te_policy_ppo_grad_bf16(const float* params, const uint16_t* weights_bf16, const uint16_t* weights_bf16_t, const te_policy_shape* shape,
                            int32_t n, const int64_t* index, const float* lidar, const float* inertial, const float* last_action,
                            const float* action, const float* old_logp, const float* adv, const float* ret, const float* adv_mean_std,
                            float clip_range, float vf_coef, float ent_coef, float* grad, float* stats, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The gradient of PPO's loss (dronechase_amd/ppo.py PPO.update) for one minibatch of n rows, in fp32:
 *   mu, v  = the policy of te_policy_act on row i;  sigma = exp(log_std)
 *   logp   = sum_j (-(action_j - mu_j)^2 / (2 sigma_j^2) - log_std_j - log(2 pi) / 2)
 *   A      = (adv - adv_mean_std[0]) / (adv_mean_std[1] + 1e-8)   (A = adv when adv_mean_std is NULL; the caller passes the
 *            minibatch's mean and unbiased std, a device pointer so the call needs no host value)
 *   ratio  = exp(logp - old_logp);  pg = -mean(min(A ratio, A clamp(ratio, 1 - clip_range, 1 + clip_range)))
 *   vl     = mean((v - ret)^2);  ent = mean over rows of sum_j (0.5 + log(2 pi) / 2 + log_std_j)
 *   loss   = pg + vf_coef vl - ent_coef ent
 * grad (te_policy_param_words words, 16-byte aligned) = d loss / d params in the packed layout above, with autograd's conventions
 * (min splits a tie evenly, clamp passes the gradient on the closed interval, ReLU's gradient at 0 is 0).  stats [4] = pg, vl,
 * ent, clip_frac = mean(|ratio - 1| > clip_range).  Both are overwritten.
 * Row i of the minibatch is read at row index[i] (int64, device) of lidar [*][C][13][26], inertial [*][15], last_action [*][4],
 * action [*][4], old_logp, adv and ret [*]; index == NULL reads row i.  workspace: device memory, 256-byte aligned, of at
 * least te_policy_grad_workspace_bytes(lidar_channels, n) bytes (about 17.5 KB per row).  n <= 2^27.
 * The result depends only on the inputs: every sum has a fixed order (no atomics), so repeated calls are bitwise equal.
 * Three launches on `stream` (no allocation, no host synchronisation: a HIP graph can capture the call); runs on the current
 * device.  Every argument error returns before anything is launched. */
int te_policy_grad_workspace_bytes(int32_t lidar_channels, int32_t n, size_t* out_bytes);
int te_policy_ppo_grad(const float* params, int32_t lidar_channels, int32_t n, const int64_t* index, const float* lidar,
                       const float* inertial, const float* last_action, const float* action, const float* old_logp, const float* adv,
                       const float* ret, const float* adv_mean_std, float clip_range, float vf_coef, float ent_coef, float* grad,
                       float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* te_policy_ppo_grad for a packed buffer of any served te_policy_shape: the same loss, arguments, checks (null, alignment, workspace
 * size, clip_range, n <= 2^27; an unserved shape fails as in te_policy_shape_check, before any launch), outputs and guarantees
 * (fixed sum orders, bitwise repeatable, three launches, capturable); grad has te_policy_param_words_shaped(shape) words.  With the
 * default shape both calls are the unshaped ones: the same size, and bitwise the same grad and stats.
 * workspace: at least te_policy_grad_workspace_bytes_shaped(shape, n) bytes.  Per row it holds every layer's input and
 * pre-activation gradient: 4 320 floats = 17 280 B for the default shape, 7 904 floats = 31 616 B for either features_dim 512 shape
 * (lidar_channels 3; 192 floats fewer for 2), for n rounded up to 32 rows whatever the shape, each array rounded up to 256 B; then
 * the split-K partials, one copy of the gradient and the statistics per 2 048 rows of a layer's reduction (conv1 has 12 n rows, conv2
 * 3 n).  At lidar_channels 3 the function returns 4 099 328 / 5 142 784 B for n <= 32 and 2 175 067 904 / 2 208 458 496 B
 * (33 189 / 33 698 B per row) for n = 65 536 with hidden 128, 256, 512 / 512, 128, 256; 1 166 870 272 B (17 805 B per row) there for
 * the default shape. */
int te_policy_grad_workspace_bytes_shaped(const te_policy_shape* shape, int32_t n, size_t* out_bytes);
int te_policy_ppo_grad_shaped(const float* params, const te_policy_shape* shape, int32_t n, const int64_t* index, const float* lidar,
                              const float* inertial, const float* last_action, const float* action, const float* old_logp,
                              const float* adv, const float* ret, const float* adv_mean_std, float clip_range, float vf_coef,
                              float ent_coef, float* grad, float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* The optimiser step of the PPO learner: clip_grad_norm_ followed by torch.optim.Adam (the non-fused form; no weight decay, no
 * amsgrad: SB3's optimiser) over ONE flat buffer of `words` fp32 parameters, e.g. the packed buffer of te_policy_act with the
 * gradient of te_policy_ppo_grad.  The call knows nothing of the policy's layers: any words in [1, 2^40] is served.
 *   s      = grad_scale * grad                      (a data-parallel caller passes 1 / world_size after its all-reduce)
 *   norm   = ||s||_2;  coef = min(1, max_grad_norm / (norm + 1e-6));  g = coef * s
 *   t      = step + 1;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   params -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)      (fp32; the two bias corrections in fp64)
 * max_grad_norm must be > 0; INFINITY means no clipping.  Non-finite gradients propagate as they do in torch.
 *
 * `state` is ONE caller-owned device buffer of te_policy_opt_state_bytes(words) bytes, 16-byte aligned; a zero-filled state is a
 * fresh optimiser, and the buffer is saved and restored with a plain device copy.  Layout, with A = 4 * words rounded up to 16:
 *   byte 0: step (i32, the number of calls so far);  byte 4: norm of the last call (f32, before clipping);  byte 8: coef of the last
 *   call (f32);  bytes 12..63 reserved, zero;  byte 64: m [words] f32;  byte 64 + A: v [words] f32;  byte 64 + 2 A: the gradient
 *   norm's partial sums, one f32 per 4 096 words, rounded up to 16 bytes (scratch: overwritten by every call).
 * params and grad are 16-byte aligned.  Every sum has a fixed order and there are no atomics: a step depends on its inputs only, and
 * repeated runs are bitwise equal.
 * Two launches on `stream` (no allocation, no host synchronisation: a HIP graph can capture the call); runs on the current device.
 * The step counter lives in the state, so every replay of a captured call advances it; lr and the other scalars are captured by
 * value.  Every argument error (null pointer, misalignment, words == 0, state_bytes too small, lr < 0, a beta outside [0, 1),
 * eps <= 0, max_grad_norm <= 0 or NaN, a non-finite grad_scale) returns before anything is launched. */
int te_policy_opt_state_bytes(size_t words, size_t* out_bytes);
int te_policy_adam_step(float* params, const float* grad, void* state, size_t state_bytes, size_t words, double lr, double beta1,
                        double beta2, double eps, float max_grad_norm, float grad_scale, void* stream);

/* The PPO learner's advantage arithmetic between the rollout and the gradient call (dronechase_amd/ppo.py RolloutBuffer.finish and
 * the minibatch's advantage normalisation).  Neither call knows the policy or the environments.
 *
 * te_rollout_gae: GAE(lambda) over a rollout of n_steps x n_envs.  rewards, values, dones (1.0 where the env finished AFTER the step,
 * else 0.0), adv and ret are contiguous [n_steps][n_envs] f32, last_value [n_envs] is the value of the state after the last step;
 * 4-byte alignment is all that is asked (n_envs may be odd).  For every env, with nxt = last_value, gae = 0 and t = n_steps - 1 ... 0:
 *   nt    = 1 - dones[t]
 *   delta = (rewards[t] + (fl32(gamma) nxt) nt) - values[t]
 *   gae   = delta + (fl32(gamma gae_lambda) nt) gae           (the product gamma gae_lambda is formed in double on the host)
 *   adv[t] = gae;  ret[t] = gae + values[t];  nxt = values[t]
 * Every operation is rounded to fp32 on its own (no fused multiply-add), in this order: the result is bitwise what the same
 * recurrence gives as one PyTorch op per operation.  adv and ret must not overlap the inputs or each other (refused).
 * n_steps, n_envs >= 1, n_steps n_envs <= 2^31 - 1, gamma and gae_lambda in [0, 1].  One launch on `stream`, one thread per env.
 *
 * te_adv_stats: out_mean_std[0] = the mean and out_mean_std[1] = the unbiased standard deviation (torch.std's default; NaN for
 * n = 1) of the n elements x[index[i]] (index: int64, device, not range-checked; NULL reads x[i]): the adv_mean_std of
 * te_policy_ppo_grad.  The sums are fp64, of x - x[index[0]] and its square, over fixed slices of 4 096 elements with a fixed tree
 * inside a slice and the slices in index order: no atomics, repeated calls are bitwise equal, an indexed call equals the call on the
 * gathered elements, and a constant input has a std of exactly 0.  workspace: device memory, 8-byte aligned, of at least
 * te_adv_stats_workspace_bytes(n) bytes (16 per slice, a multiple of 16; overwritten by every call).  1 <= n <= 2^40.  Two launches
 * on `stream`.
 *
 * Both calls allocate nothing and do not synchronise with the host (a HIP graph can capture them) and run on the current device.
 * Every argument error (null pointer, misalignment, a size out of range, gamma or gae_lambda outside [0, 1] or not finite,
 * overlapping outputs, a workspace too small) returns before anything is launched. */
int te_rollout_gae(int32_t n_steps, int32_t n_envs, const float* rewards, const float* values, const float* dones,
                   const float* last_value, double gamma, double gae_lambda, float* adv, float* ret, void* stream);
int te_adv_stats_workspace_bytes(int64_t n, size_t* out_bytes);
int te_adv_stats(const float* x, const int64_t* index, int64_t n, float* out_mean_std, void* workspace, size_t workspace_bytes,
                 void* stream);

/* The optimiser step that leaves the bf16 copies of the weights current: the step above on the packed buffer of a served
 * te_policy_shape (words is that shape's parameter count), where the thread that has just computed a word of a weight layer also stores
 * its bf16 rounding (nearest-even, the conversion of the pack calls) at its place in weights_bf16 ([n][Kp], the layout of the bf16 pack
 * call) and, when weights_bf16_t is not NULL and the layer has a block there, in weights_bf16_t ([k][Np], the layout of the transposed
 * pack call).  Biases, mu, value and log_std have no bf16 copy.  The arithmetic of the step is the same code: params and state end up
 * bitwise as the plain step leaves them, and afterwards both bf16 buffers are bitwise what the two pack calls give on the stepped
 * params, so no repack launch follows a step.
 * REQUIREMENT: the pad columns of the bf16 buffers are never written here.  Both buffers must have been packed once by their pack call
 * (any params of this shape) before the first step; the pad columns keep the zeros of that pack.
 * Still two launches on `stream`, no atomics, no allocation, no host synchronisation; a HIP graph can capture the call; bitwise
 * repeatable.  Checks: the plain step's, plus: the shape is served (as in the shape check), weights_bf16 is not NULL and 16-byte
 * aligned, weights_bf16_t is 16-byte aligned when given.  Every refusal returns before anything is launched. */
int te_policy_adam_step_bf16(float* params, const float* grad, void* state, size_t state_bytes, const te_policy_shape* shape,
                             uint16_t* weights_bf16, uint16_t* weights_bf16_t, double lr, double beta1, double beta2, double eps,
                             float max_grad_norm, float grad_scale, void* stream);

/* One epoch of the PPO update enqueued by one call: the four calls of a minibatch (advantage statistics, gradient, optimiser step, the
 * log's running sums), for every minibatch of a permutation, without a return to the caller in between.
 * For k = 0, 1, ... with s = k * batch < n_perm and b = min(batch, n_perm - s), in this order on `stream`:
 *   1. the statistics call on (adv, perm + s, b) into adv_mean_std (adv_workspace: at least the statistics workspace of
 *      min(batch, n_perm) elements);
 *   2. the gradient call over the rows index = perm + s, b of them, with adv_mean_std, into grad and stats (workspace: at least the
 *      gradient workspace of min(batch, n_perm) rows, of the precision chosen below);
 *   3. the optimiser step on params with grad;
 *   4. one single-thread launch: sums[0..3] += stats[0..3] (pg, vl, ent, clip_frac), sums[4] += the state's norm word (the gradient's
 *      norm before clipping), in fp32.  sums is added to, never cleared: the caller zeroes it when its log starts.
 * weights_bf16 and weights_bf16_t both NULL: the fp32 shaped gradient call and the plain step.  Both given: the bf16 gradient call and
 * the step that keeps them current (above; its requirement holds here: both packed once, and current with params when the call
 * starts).  Exactly one given is refused.
 * Everything the calls would write is bitwise what the same calls give when made one by one.  perm is int64 on the device, not
 * range-checked, and required.  The call allocates nothing and never synchronises with the host.  EVERY check is made before the
 * first launch: struct_size == sizeof(te_ppo_epoch_args), a served shape, batch >= 1, 1 <= n_perm <= 2^40, and every check of the four inner
 * calls for the first and for the last (shortest) minibatch; a refusal leaves every buffer as it was, with te_last_error set. */
typedef struct te_ppo_epoch_args {
  size_t struct_size;                       /* sizeof(te_ppo_epoch_args), set by the caller */
  te_policy_shape shape;
  float* params;                            /* the packed fp32 buffer, stepped in place */
  uint16_t* weights_bf16;                   /* both NULL: fp32; both given: bf16, kept current by the step */
  uint16_t* weights_bf16_t;
  const float* lidar;                       /* the rollout's row arrays, as the gradient call reads them */
  const float* inertial;
  const float* last_action;
  const float* action;
  const float* old_logp;
  const float* adv;
  const float* ret;
  const int64_t* perm;                      /* device, n_perm row numbers */
  int64_t n_perm;
  int32_t batch;                            /* rows per minibatch; the last one may be shorter */
  float clip_range, vf_coef, ent_coef;
  float* grad;                              /* the packed gradient: the last minibatch's when the call ends */
  void* state;                              /* the optimiser's state buffer */
  size_t state_bytes;
  double lr, beta1, beta2, eps;
  float max_grad_norm, grad_scale;
  void* workspace;                          /* the gradient workspace, 256-byte aligned */
  size_t workspace_bytes;
  void* adv_workspace;                      /* the statistics workspace */
  size_t adv_workspace_bytes;
  float* adv_mean_std;                      /* device scratch [2] */
  float* stats;                             /* device scratch [4] */
  float* sums;                              /* device [5]: pg, vl, ent, clip_frac, grad_norm; added to */
} te_ppo_epoch_args;
int te_policy_ppo_epoch(const te_ppo_epoch_args* args, void* stream);

/* Episode monitor: the bookkeeping of SB3's VecMonitor.step_wait (episode return and length per env, `infos[i]["episode"]`), of
 * its logger's ep_rew_mean / ep_len_mean window, and of evaluate_policy's per-env episode quotas (what the reference's
 * ReinforcementLearningPipeline.evaluate rests on, src/core/rl_framework/utils/pipeline.py:374-414), next to the step on the
 * device instead of in Python on the host.
 *
 * A monitor is ONE caller-owned device buffer of te_monitor_bytes(n_envs, n_records) bytes, 16-byte aligned.  The calls take no
 * te_env, allocate nothing, enqueue on `stream` only (no host synchronisation: a HIP graph can capture them) and run on the
 * current device; the buffer is cloned and restored with a plain device copy.  Every call takes the same (mon, bytes, n_envs,
 * n_records) the buffer was initialised with; every argument error (null pointer, n_envs <= 0, n_records < 0, bytes too small,
 * misalignment) returns before anything is launched.
 *
 * te_monitor_step, after every te_step, with that step's reward [N] f32, done [N] u8 and info [N][4] i32 (16-byte aligned).
 * For env e:  ret_e = ret_e + reward_e (one fp32 add per step, in step order: a host loop in float32 reproduces it bit for bit);
 * len_e += 1; if done_e, the episode (ret_e, len_e, info_e) is complete (te_step computes info before the auto-reset, so the row
 * of a done step is the ended episode's): it is added to the window accumulators, written to record slot offset_e + k_e if
 * k_e < quota_e, k_e += 1, last_ret_e / last_len_e = (ret_e, len_e), and ret_e = len_e = 0.
 * Quotas are evaluate_policy's: quota_e = (n_records + e) / N, i.e. with q = n_records / N and r = n_records % N,
 * quota_e = q + (e >= N - r) and offset_e = e q + max(0, e - (N - r)): records are env-major, then by episode ordinal, and an env
 * with short episodes contributes no more than its share.  n_records = 0 records nothing.
 *
 * Window accumulators (count, sum of len, sum of info[0..3] as int64; sum of ret and of ret^2 as double; min / max ret as float)
 * are kept per wave of 64 envs, reduced in a fixed order: no float atomics, repeated runs are bitwise equal.  te_monitor_stats
 * sums the waves' rows in a fixed order into *out (DEVICE memory, 8-byte aligned) and, with reset_window != 0, clears them; partial
 * episodes, k_e and the records are kept.  min_ret / max_ret are 0 when count == 0.
 *
 * Buffer layout (byte offsets from te_monitor_layout; all arrays 16-byte aligned): word 0 = recorded (i32, the number of record
 * slots written so far); rows [n_rows][72 bytes]; ret [N] f32, len [N] i32, episodes [N] i32 (k_e), last_ret [N] f32, last_len [N]
 * i32; rec_info [R][4] i32, rec_ret [R] f32, rec_len [R] i32.  te_monitor_init zeroes the whole buffer. */
typedef struct te_monitor_summary {
  int64_t count, sum_len, sum_info[4];
  double sum_ret, sum_ret2;
  float min_ret, max_ret;
  int32_t recorded, reserved;
} te_monitor_summary;

typedef struct te_monitor_offsets {
  size_t bytes, n_rows, rows, ret, len, episodes, last_ret, last_len, rec_info, rec_ret, rec_len;
} te_monitor_offsets;

int te_monitor_bytes(int32_t n_envs, int32_t n_records, size_t* out_bytes);
int te_monitor_layout(int32_t n_envs, int32_t n_records, te_monitor_offsets* out);
int te_monitor_init(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, void* stream);
int te_monitor_step(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, const float* reward, const uint8_t* done,
                    const int32_t* info, void* stream);
int te_monitor_stats(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, te_monitor_summary* out, int32_t reset_window,
                     void* stream);

/* Sphere encoder of the level5 student (dronechase_amd/student.py): the two convolution blocks of the reference's SphereCNN
 * (fused_lidar_extractor.py:653-720) over the stacked observation, skipping the spheres the network never looks at.  fp32 on
 * v_mfma_f32_16x16x4_f32 (dronechase_amd/csrc/te_sphere.hpp).  te_sphere_encode is the forward; te_sphere_encode_grad, below, is the
 * gradient of its parameters.
 *
 * params (16-byte aligned, te_sphere_encode_param_words(channels) floats) holds the reference's four tensors, each flattened, in this
 * order: conv1 w[32][C][5][5], b[32], conv2 w[64][32][3][3], b[64].
 *
 * Per sphere x [C][13][26]:  block1 = circular padding by 2 in W, constant padding by 2 in H with the value 1.0 (the LIDAR's "no
 * data"), conv 5x5 stride 2, ReLU -> [32][7][13];  block2 = circular padding by 1 in W, constant 1.0 padding by 1 in H (on the feature
 * map too), conv 3x3 stride 2, ReLU -> [64][4][7];  out = its 1792 values in (co, oh, ow) order.  The Linear(1792, 512) behind them
 * is not part of the call.
 *
 * stacked [n_rows][n_spheres][C][13][26] f32, mask [n_rows][n_spheres] u8 or NULL, out [n_rows][n_spheres][1792] f32, stacked and out
 * 16-byte aligned.  Sphere s of row r COUNTS iff mask == NULL, or mask[r][s] != 0, or s == 0 and the row's mask is all zero (the
 * attention gives every other sphere the weight 0, and MLPomega._grant_at_least_one_valid turns sphere 0 of an all-zero row on).  A
 * sphere that counts gets its features; one that does not gets exact zeros and its input is never read (it may hold anything, NaN
 * included).
 *
 * Served: channels == 3, 1 <= n_spheres <= 8, n_rows >= 1, n_rows * n_spheres <= 2^31 - 1.  Any other value, a NULL pointer other
 * than mask, or a misaligned pointer is refused with te_last_error text that names the argument, before anything is launched.  The
 * call enqueues one launch on `stream` of the current device: no allocation and no host synchronisation, so a HIP graph can capture
 * it.  An element's sum order is fixed (bias first, then k): a sphere's features are bitwise the same whatever its row, its slot,
 * n_rows or the mask of other spheres. */
int te_sphere_encode_param_words(int32_t channels, size_t* out_words);
int te_sphere_encode(const float* params, int32_t channels, int32_t n_rows, int32_t n_spheres, const float* stacked,
                     const uint8_t* mask, float* out, void* stream);

/* te_sphere_encode with bf16 operands on the bf16 MFMA (v_mfma_f32_16x16x32_bf16), opt-in, inference only
 * (dronechase_amd/csrc/te_sphere_bf16.hpp).  The same function, arguments, counting rule, output type and layout.  Numerics contract:
 *   - both conv weights are rounded once to bf16, round-to-nearest-even, by te_sphere_pack_bf16; the fp32 parameter buffer stays the
 *     master copy, and both biases are read from it in fp32;
 *   - a sphere's cells are rounded to bf16 (round-to-nearest-even) when they are staged for the MFMA; the padding constant 1.0 is exact;
 *   - products are accumulated in fp32 by the MFMA, the accumulator starting from the fp32 bias; ReLU runs in fp32;
 *   - block1's post-ReLU output is rounded to bf16 (round-to-nearest-even) where it is stored for block2;
 *   - block2's output is stored as fp32: out is te_sphere_encode's buffer, so everything behind the encoder is unchanged;
 *   - an element's sum order is over k only (k-blocks of 32 in order, within a block the MFMA's own order): a sphere's features are
 *     bitwise the same in any row, slot, batch, grid or mask of other spheres, and repeated calls are bitwise equal;
 *   - a sphere that does not count gets 1792 zeros and its input is never read.
 * The output therefore differs from te_sphere_encode's by bf16 rounding (measured: README).
 *
 * weights_bf16 is ONE device buffer of te_sphere_bf16_words(channels) = 22 528 uint16 elements, 16-byte aligned, bf16 bit patterns,
 * two tensors [N][Kp] row-major, each 16-byte aligned:
 *   element 0:     conv1 [32][128], column k = (ci * 5 + kh) * 8 + kw holds w[n][ci][kh][kw]; the columns with kw >= 5 and the
 *                  columns k >= 120 are zero (the kernel width is padded from 5 to 8);
 *   element 4096:  conv2 [64][288], column k = (kh * 3 + kw) * 32 + ci holds w[n][ci][kh][kw].
 * Biases are not in it.  te_sphere_pack_bf16 fills it from `params` (te_sphere_encode's buffer) in one launch on `stream`, no host
 * synchronisation; call it again after every change of `params`.
 *
 * Served: te_sphere_encode's domain.  A value outside it, a NULL pointer other than mask, or params / weights_bf16 / out / stacked not
 * 16-byte aligned is refused with te_last_error text that names the call and the argument, before anything is launched.  One launch
 * on `stream` of the current device, no allocation and no host synchronisation.  There is no bf16 backward: train through
 * te_sphere_encode and te_sphere_encode_grad. */
int te_sphere_bf16_words(int32_t channels, size_t* out_halfwords);
int te_sphere_pack_bf16(const float* params, int32_t channels, uint16_t* out, void* stream);
int te_sphere_encode_bf16(const float* params, const uint16_t* weights_bf16, int32_t channels, int32_t n_rows, int32_t n_spheres,
                          const float* stacked, const uint8_t* mask, float* out, void* stream);

/* The backward of te_sphere_encode with respect to its parameters: grad (te_sphere_encode_param_words(channels) floats, in params'
 * layout) = sum over the counting spheres of d(out) / d(params) applied to d_out.  No gradient with respect to `stacked` exists: it is
 * an observation.
 *
 * params, channels, n_rows, n_spheres, stacked and mask as te_sphere_encode took them; out [n_rows][n_spheres][1792] is what that call
 * wrote (its sign pattern is block2's ReLU mask, so the mask is the forward's own decision); d_out, of out's shape, is the upstream
 * gradient.  Block1's activations are recomputed from `stacked` by the forward's own code, bitwise as the forward had them.  A sphere
 * that does not count contributes nothing, and its stacked, out and d_out entries are never read (they may hold NaN).
 *
 * workspace: 256-byte aligned, at least te_sphere_encode_grad_workspace_bytes(channels, n_rows, n_spheres) bytes, its content
 * irrelevant; each workgroup leaves one partial gradient there and a second launch sums the partials in workgroup order into grad,
 * which is overwritten, not accumulated into.  There are no float atomics: the same arguments on the same device give the same bits
 * on every call.  Against a float64 reference the result differs as float32 sums of up to n_rows * n_spheres * 91 terms do.
 *
 * Served: te_sphere_encode's domain.  A value outside it, a NULL pointer other than mask, params / stacked / out / d_out / grad not
 * 16-byte aligned, or a workspace that is misaligned or too short is refused with te_last_error text that names the argument, before
 * anything is launched.  Two launches on `stream` of the current device, no allocation and no host synchronisation. */
int te_sphere_encode_grad_workspace_bytes(int32_t channels, int32_t n_rows, int32_t n_spheres, size_t* out_bytes);
int te_sphere_encode_grad(const float* params, int32_t channels, int32_t n_rows, int32_t n_spheres, const float* stacked,
                          const uint8_t* mask, const float* out, const float* d_out, float* grad, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Imitation dataset: the middle of the reference's student line, between its collector (apps/threatsense_runner/collect_and_save.py:
 * step Level5DumbMultiObs, drop the rows whose validity mask is all false, keep the rest) and its trainer
 * (SupervisedImitationTrainer._train_ppo, core/rl_framework/utils/sl_pipeline.py:172-207, which perturbs last_action with
 * kill_high_correlation before every batch).  A ring of student rows in device memory: te_dataset_append takes te_step_students'
 * outputs as they are, te_dataset_gather writes the contiguous batch tensors te_sphere_encode and the student read.  A row
 * (24 434 bytes at 6 spheres) never leaves HBM.  dronechase_amd/csrc/te_dataset.hpp.
 *
 * A dataset is ONE caller-owned device buffer of te_dataset_layout(geom)->bytes bytes, 16-byte aligned.  The calls take no te_env,
 * allocate nothing, enqueue on `stream` of the current device only (no host synchronisation: a HIP graph can capture them), and
 * every call takes the (ds, bytes, geom) the buffer was initialised with.  Served: channels == 3, 1 <= n_spheres <= 8,
 * 1 <= max_append_rows <= capacity <= 2^31 - 1.  Any other value, a NULL, misaligned or short buffer, and the argument errors named
 * below are refused with te_last_error text that names the argument, before anything is launched.
 *
 * Buffer layout (byte offsets from te_dataset_layout, a host-only call; every array 16-byte aligned, in this order, nothing
 * overlaps): header (64 bytes; word 0 = total, i64, the number of rows ever appended; the rest reserved and zero);
 * dst [max_append_rows] i32 (scratch of one append); the rings stacked [capacity][S][3][13][26] f32, mask [capacity][S] u8,
 * inertial [capacity][15] f32, last_action [capacity][4] f32, teacher [capacity][4] f32.  size = min(total, capacity); the k-th kept
 * row of an append that found total = T lands in slot (T + k) mod capacity.  te_dataset_init zeroes the whole buffer.
 *
 * te_dataset_append: stacked [n_rows][S][3][13][26] f32 (16-byte aligned), mask [n_rows][S] u8, inertial [n_rows][15] f32,
 * last_action and teacher [n_rows][4] f32 (teacher may alias last_action), active [n_rows] u8 or NULL (every row active): exactly
 * te_step_students' outputs with n_rows = N * P.  1 <= n_rows <= max_append_rows.  A row is KEPT iff it is active and any of its mask
 * bytes is non-zero (the collector's armed rows behind drop_invalid_student_obs).  Kept rows are appended in source-row order and
 * total advances by their count, on the device.  Of a row that is not kept only active and mask are read: the rest may hold NaN.  The
 * inputs must not overlap the dataset.  Two launches: a scan (one workgroup; keep flags and their exclusive prefix sum in row order
 * -> dst[row] = slot or -1, and the new total) and a copy (one workgroup per source row, 16-byte loads and stores).  No workgroup
 * waits on another.
 *
 * te_dataset_gather: one launch, one workgroup per output row, into out_stacked [batch][S][3][13][26] f32 (16-byte aligned),
 * out_mask [batch][S] u8, out_inertial [batch][15] f32, out_last_action and out_teacher [batch][4] f32, and, when not NULL,
 * out_index [batch] i64 (the slots used).  batch >= 1.  index (i64 [batch], DEVICE memory, 8-byte aligned, or NULL) names the slots; a
 * value outside [0, capacity) is clamped into it, so the call is memory-safe whatever index holds; staying below size is the
 * caller's contract (a slot never written holds te_dataset_init's zeros).  With index == NULL row j draws its slot from the size the
 * kernel reads on the device: slot_j = mulhi32(w.x, size), w = philox4x32_10(counter (j, draw_lo, draw_hi, 1), key (seed_lo, seed_hi));
 * at size == 0 every output row is zeros and out_index is -1.
 * last_action_mode is the branch of the reference's kill_high_correlation for this batch (the reference draws the branch once per
 * batch, on the host).  With w = philox4x32_10((j, draw_lo, draw_hi, 2), key) and u(x) = x >> 8:
 *   TE_DATASET_LA_KEEP    out_last_action = the stored row
 *   TE_DATASET_LA_RANDOM  la[k] = (float)u(w[k]) * 2^-23 - 1: exact in fp32, in [-1, 1)
 *   TE_DATASET_LA_NOISE   la[k] = clamp(la[k] + noise_std * z[k], -1, 1), z from two Box-Muller pairs: u1 = (u(w.x) + 1) * 2^-24,
 *                         u2 = u(w.y) * 2^-24, r = sqrtf(-2 logf(u1)), z0 = r cosf(2 pi u2), z1 = r sinf(2 pi u2); z2, z3 the same from
 *                         (w.z, w.w).  noise_std >= 0; the reference's alpha = 0.1 is noise_std = 0.2.
 * stacked, mask, inertial and teacher are never perturbed.  The same arguments give the same bits on every call. */
typedef struct te_dataset_geom {
  int32_t capacity, max_append_rows, n_spheres, channels;
} te_dataset_geom;

typedef struct te_dataset_offsets {
  size_t bytes, header, dst, stacked, mask, inertial, last_action, teacher;
} te_dataset_offsets;

enum { TE_DATASET_LA_KEEP = 0, TE_DATASET_LA_RANDOM = 1, TE_DATASET_LA_NOISE = 2 };

int te_dataset_layout(const te_dataset_geom* geom, te_dataset_offsets* out);
int te_dataset_init(void* ds, size_t bytes, const te_dataset_geom* geom, void* stream);
int te_dataset_append(void* ds, size_t bytes, const te_dataset_geom* geom, int32_t n_rows, const float* stacked, const uint8_t* mask,
                      const float* inertial, const float* last_action, const float* teacher, const uint8_t* active, void* stream);
int te_dataset_gather(void* ds, size_t bytes, const te_dataset_geom* geom, int32_t batch, const int64_t* index, uint64_t seed,
                      uint64_t draw, int32_t last_action_mode, float noise_std, float* out_stacked, uint8_t* out_mask,
                      float* out_inertial, float* out_last_action, float* out_teacher, int64_t* out_index, void* stream);

int te_abi_version(void);
const char* te_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* THREATENGAGE_H */
