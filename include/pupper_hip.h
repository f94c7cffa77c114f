/*
 * pupper_hip.h -- C-ABI of the MI355X-native Pupper-v3 environment.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json
 * `north_star`: the batched replacement for
 *
 *   pupperv3_mjx.environment.PupperV3Env.reset(rng)  (environment.py:314-346)
 *   pupperv3_mjx.environment.PupperV3Env.step(state, action)  (environment.py:348-483)
 *
 * including the MJX physics they call (`pipeline_init` environment.py:319,
 * `pipeline_step` environment.py:366 -> 5 x mjx.step), the reward stack
 * (rewards.py:9-138), the observation pipeline (environment.py:485-543) and the
 * per-env domain randomisation (domain_randomization.py:8-112).
 *
 * Plain C types only: pointers + sizes, int status codes, no exceptions and no
 * torch types across the boundary.  All `*_dev` arguments are device pointers
 * on the handle's device; `stream` is a hipStream_t passed as void* (NULL =
 * the handle's own stream).
 *
 * The reference's FFI for this path is Python (Brax `Env.reset/step`,
 * [ext] brax 0.12.1 brax/envs/base.py); the ctypes binding a maintainer adds is
 * shown in INTEGRATION.md and implemented in pupperv3-mjx_amd/pupperv3_mjx/_lib.py.
 */
#ifndef PUPPER_HIP_H_
#define PUPPER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP3_ABI_VERSION 2

/* ---- fixed topology of test_pupper_model.xml (checked at pp3_create) ---- */
#define PP3_NBODY 14      /* world + base_link + 4 legs x 3 links          */
#define PP3_NJNT 13       /* 1 free joint + 12 hinges                      */
#define PP3_NQ 19
#define PP3_NV 18
#define PP3_NU 12
#define PP3_NLEG 4
#define PP3_NFOOT 4
#define PP3_MAX_CGEOM 96  /* collidable geoms (8 spheres + floor + boxes)  */
#define PP3_MAX_PAIR 640  /* candidate collision pairs after filtering     */
#define PP3_MAX_SITE 8
#define PP3_MAX_SENSOR 16     /* <sensor> entries (site-based types below)   */
#define PP3_MAX_SENSORDATA 32 /* total sensordata floats                      */
#define PP3_MAX_LAG 8     /* latency-buffer length limit                   */
#define PP3_NREWARD 18    /* reward terms, order = PP3_REWARD_* below      */
#define PP3_NMETRIC 19    /* total_dist + 18 scaled reward terms           */
#define PP3_NDR 62        /* per-env domain-randomisation scalars          */
#define PP3_OBS_DIM 36    /* environment.py:226                            */

/* MuJoCo enums restated (mjtGeom / mjtJoint / mjtCone / mjtBias) */
enum { PP3_GEOM_PLANE = 0, PP3_GEOM_SPHERE = 2, PP3_GEOM_BOX = 6 };
enum { PP3_JNT_FREE = 0, PP3_JNT_HINGE = 3 };
enum { PP3_CONE_PYRAMIDAL = 0 };
enum { PP3_BIAS_NONE = 0, PP3_BIAS_AFFINE = 1 };
/* sensor types (own numbering; each is attached to a site, objtype="site") */
enum {
  PP3_SENS_ACCELEROMETER = 1,
  PP3_SENS_VELOCIMETER = 2,
  PP3_SENS_GYRO = 3,
  PP3_SENS_FRAMEPOS = 26,
  PP3_SENS_FRAMEQUAT = 27,
  PP3_SENS_FRAMELINVEL = 32,
  PP3_SENS_FRAMEANGVEL = 33
};

/* Reward-term order = the rewards_dict literal in environment.py:391-444
 * (this order is also the fp32 summation order of environment.py:446). */
enum {
  PP3_REWARD_TRACKING_LIN_VEL = 0,
  PP3_REWARD_TRACKING_ANG_VEL,
  PP3_REWARD_TRACKING_ORIENTATION,
  PP3_REWARD_LIN_VEL_Z,
  PP3_REWARD_ANG_VEL_XY,
  PP3_REWARD_ORIENTATION,
  PP3_REWARD_TORQUES,
  PP3_REWARD_JOINT_ACCELERATION,
  PP3_REWARD_MECHANICAL_WORK,
  PP3_REWARD_ACTION_RATE,
  PP3_REWARD_STAND_STILL,
  PP3_REWARD_STAND_STILL_JOINT_VELOCITY,
  PP3_REWARD_ABDUCTION_ANGLE,
  PP3_REWARD_FEET_AIR_TIME,
  PP3_REWARD_FOOT_SLIP,
  PP3_REWARD_TERMINATION,
  PP3_REWARD_KNEE_COLLISION,
  PP3_REWARD_BODY_COLLISION
};

/* Compiled model (host, fp64).  Produced by the MJCF-subset compiler
 * pupperv3_mjx/mjcf.py from test_pupper_model.xml (+ obstacles.py boxes).
 * Field names follow mjModel. */
typedef struct pp3_model_t {
  /* <option> */
  double timestep;
  double gravity[3];
  double impratio;
  double tolerance;
  double ls_tolerance;
  int32_t iterations;
  int32_t ls_iterations;
  int32_t cone;
  int32_t eulerdamp;   /* 1 = enabled; the model disables it (xml:58) */
  double meaninertia;  /* mjStatistic.meaninertia: mean diag(M) at qpos0 */
  /* bodies (0 = world) */
  int32_t body_parentid[PP3_NBODY];
  int32_t body_jntadr[PP3_NBODY];
  int32_t body_dofadr[PP3_NBODY];
  int32_t body_dofnum[PP3_NBODY];
  double body_pos[PP3_NBODY][3];
  double body_quat[PP3_NBODY][4];
  double body_ipos[PP3_NBODY][3];
  double body_iquat[PP3_NBODY][4];
  double body_mass[PP3_NBODY];
  double body_inertia[PP3_NBODY][3];
  double body_invweight0[PP3_NBODY][2];
  /* joints */
  int32_t jnt_type[PP3_NJNT];
  int32_t jnt_bodyid[PP3_NJNT];
  int32_t jnt_qposadr[PP3_NJNT];
  int32_t jnt_dofadr[PP3_NJNT];
  int32_t jnt_limited[PP3_NJNT];
  double jnt_pos[PP3_NJNT][3];
  double jnt_axis[PP3_NJNT][3];
  double jnt_range[PP3_NJNT][2];
  double jnt_margin[PP3_NJNT];
  double jnt_solref[PP3_NJNT][2];
  double jnt_solimp[PP3_NJNT][5];
  /* dofs */
  int32_t dof_bodyid[PP3_NV];
  int32_t dof_jntid[PP3_NV];
  int32_t dof_parentid[PP3_NV];
  double dof_armature[PP3_NV];
  double dof_damping[PP3_NV];
  double dof_frictionloss[PP3_NV];
  double dof_invweight0[PP3_NV];
  double dof_solref[PP3_NV][2];
  double dof_solimp[PP3_NV][5];
  double qpos0[PP3_NQ];
  double key_qpos[PP3_NQ]; /* keyframe "home" */
  /* collidable geoms (contype|conaffinity != 0); cgeom_id = MuJoCo geom id */
  int32_t ngeom;  /* total MuJoCo geoms (ids) */
  int32_t ncgeom;
  int32_t cgeom_id[PP3_MAX_CGEOM];
  int32_t cgeom_type[PP3_MAX_CGEOM];
  int32_t cgeom_bodyid[PP3_MAX_CGEOM];
  int32_t cgeom_condim[PP3_MAX_CGEOM];
  int32_t cgeom_priority[PP3_MAX_CGEOM];
  double cgeom_size[PP3_MAX_CGEOM][3];
  double cgeom_pos[PP3_MAX_CGEOM][3];   /* in body frame */
  double cgeom_quat[PP3_MAX_CGEOM][4];  /* in body frame */
  double cgeom_friction[PP3_MAX_CGEOM][3];
  double cgeom_solref[PP3_MAX_CGEOM][2];
  double cgeom_solimp[PP3_MAX_CGEOM][5];
  double cgeom_solmix[PP3_MAX_CGEOM];
  double cgeom_margin[PP3_MAX_CGEOM];
  double cgeom_gap[PP3_MAX_CGEOM];
  /* candidate pairs (indices into cgeom_*), type(g1) <= type(g2) */
  int32_t npair;
  int32_t pair_g1[PP3_MAX_PAIR];
  int32_t pair_g2[PP3_MAX_PAIR];
  /* sites */
  int32_t nsite;
  int32_t site_bodyid[PP3_MAX_SITE];
  double site_pos[PP3_MAX_SITE][3];
  double site_quat[PP3_MAX_SITE][4];
  /* actuators (general, joint transmission) */
  int32_t actuator_trnid[PP3_NU];  /* joint id */
  int32_t actuator_biastype[PP3_NU];
  int32_t actuator_forcelimited[PP3_NU];
  int32_t actuator_ctrllimited[PP3_NU];
  double actuator_gear[PP3_NU];
  double actuator_gainprm[PP3_NU][3];
  double actuator_biasprm[PP3_NU][3];
  double actuator_forcerange[PP3_NU][2];
  double actuator_ctrlrange[PP3_NU][2];
  /* <custom> numerics (MJX collision caps; -1 = absent) */
  int32_t max_contact_points;
  int32_t max_geom_pairs;
  /* <sensor> (xml:14-23): site sensors, sensordata = mjData.sensordata layout */
  int32_t nsensor;
  int32_t nsensordata;
  int32_t sensor_type[PP3_MAX_SENSOR];   /* PP3_SENS_* */
  int32_t sensor_objid[PP3_MAX_SENSOR];  /* site id */
  int32_t sensor_adr[PP3_MAX_SENSOR];
  int32_t sensor_dim[PP3_MAX_SENSOR];
  double sensor_cutoff[PP3_MAX_SENSOR];  /* 0 = none */
} pp3_model_t;

/* Environment configuration: PupperV3Env.__init__ kwargs
 * (environment.py:35-121) + config.py reward scales. */
typedef struct pp3_env_config_t {
  int32_t n_frames;            /* physics substeps per env step (5)        */
  int32_t obs_history;         /* H                                         */
  int32_t use_imu;
  int32_t latency_len;         /* La = len(latency_distribution)           */
  int32_t imu_latency_len;     /* Li                                        */
  int32_t resample_velocity_step;
  int32_t early_termination_step_threshold;
  int32_t torso_body;
  int32_t feet_site[PP3_NFOOT];
  int32_t lower_leg_body[PP3_NFOOT];
  int32_t n_upper_leg_geoms;
  int32_t upper_leg_geoms[16];
  int32_t n_torso_geoms;
  int32_t torso_geoms[8];
  int32_t rng_partitionable;   /* jax_threefry_partitionable (jax 0.5.0: 1) */
  int32_t ncon_max;            /* contact cap per env (deepest kept): 0 = default 8, 8, 16 */
  double latency_dist[PP3_MAX_LAG];
  double imu_latency_dist[PP3_MAX_LAG];
  double action_scale;
  double default_pose[PP3_NU];
  double joint_lower[PP3_NU];
  double joint_upper[PP3_NU];
  double desired_abduction[4];
  double start_pos_min[3];
  double start_pos_max[3];
  double lin_vel_x_range[2];
  double lin_vel_y_range[2];
  double ang_vel_range[2];
  double zero_command_probability;
  double stand_still_command_threshold;
  double max_pitch_command;    /* degrees */
  double max_roll_command;     /* degrees */
  double ang_vel_noise;
  double gravity_noise;
  double motor_angle_noise;
  double last_action_noise;
  double kick_vel;
  double kick_probability;
  double terminal_body_z;
  double terminal_body_angle;
  double foot_radius;
  double env_dt;               /* self._dt = environment_timestep          */
  double dt;                   /* self.dt = opt.timestep * n_frames        */
  double desired_world_z[3];
  double reward_scales[PP3_NREWARD];
  double tracking_sigma;
} pp3_env_config_t;

typedef struct pp3_env pp3_env_t;

/* ---- per-env state record (float32 words, env-major: state[N][stride]) ---- */
enum {
  PP3_S_QPOS = 0,          /* 19 */
  PP3_S_QVEL = 19,         /* 18 */
  PP3_S_QACC_WS = 37,      /* 18  qacc_warmstart                         */
  PP3_S_RNG = 55,          /*  2  uint32 key words, bit-cast into f32    */
  PP3_S_LAST_ACT = 57,     /* 12 */
  PP3_S_LAST_VEL = 69,     /* 12 */
  PP3_S_COMMAND = 81,      /*  3 */
  PP3_S_DESIRED_Z = 84,    /*  3 */
  PP3_S_AIR_TIME = 87,     /*  4 */
  PP3_S_LAST_CONTACT = 91, /*  4  0.0 / 1.0                             */
  PP3_S_KICK = 95,         /*  2 */
  PP3_S_STEP = 97,         /*  1  step counter (integral value as float) */
  PP3_S_ACT_BUF = 98       /* 12*La action buffer [12][La], then 6*Li imu buffer [6][Li] */
};

/* Field ids for pp3_field / pp3_copy_field.  Every field is ONE device buffer owned by the
 * handle, allocated at pp3_create and updated in place: the pointer pp3_field returns stays
 * valid (and constant) until pp3_destroy, so a training loop may wrap it once; its contents are
 * overwritten by every pp3_step / pp3_reset launched on the handle's stream (copy a field out
 * first, on that stream, to keep a previous step's values). */
enum {
  PP3_F_STATE = 0,    /* [N][state_stride] f32 */
  PP3_F_OBS = 1,      /* [N][36H] f32 */
  PP3_F_REWARD = 2,   /* [N] f32 */
  PP3_F_DONE = 3,     /* [N] f32 */
  PP3_F_METRICS = 4,  /* [N][19] f32: total_dist, scaled rewards */
  PP3_F_DR = 5,       /* [N][62] f32 */
  PP3_F_PIPELINE = 6, /* [N][PP3_PIPE_STRIDE] f32 (when enabled) */
  PP3_F_ACTION = 7,   /* [N][12] f32 scratch action buffer owned by the handle */
  PP3_F_EPISODE = 8,  /* [N][PP3_EP_STRIDE] f32 episode bookkeeping (auto-reset mode) */
  PP3_F_FIRST_STATE = 9, /* [N][PP3_FIRST_STRIDE] f32 qpos|qvel|qacc_warmstart of the reset */
  PP3_F_FIRST_OBS = 10   /* [N][36H] f32 observation of the reset */
};

/* Optional pipeline-state output (brax State.x / xd of the last substep,
 * environment.py:367): written only when pp3_set_pipeline_output(h, 1). */
enum {
  PP3_P_XPOS = 0,           /* 13 x 3  body origins (bodies 1..13)       */
  PP3_P_XQUAT = 39,         /* 13 x 4 */
  PP3_P_XD_VEL = 91,        /* 13 x 3 */
  PP3_P_XD_ANG = 130,       /* 13 x 3 */
  PP3_P_SITE_XPOS = 169,    /*  4 x 3  foot sites                         */
  PP3_P_QFRC_ACT = 181,     /* 18 */
  PP3_P_QACC = 199,         /* 18 */
  PP3_P_NCON = 217,         /*  1  penetrating contacts (float)           */
  PP3_P_CON_DIST = 218,     /* 16  dist of contacts 0..15                  */
  PP3_P_CON_GEOM = 234,     /* 32  geom1, geom2 of contacts 0..15 (float)  */
  PP3_P_SUBTREE_COM = 266,  /*  3 */
  PP3_P_NHIT = 269,         /*  1  penetrating pairs before the contact cap (> ncon: the cap bound) */
  PP3_P_SENSOR = 272,       /* 32  mjData.sensordata (model's <sensor>) */
  PP3_PIPE_STRIDE = 304
};

/* DR record layout (domain_randomization.py:21-66, absolute values). */
enum {
  PP3_DR_FRICTION = 0,  /* geom_friction[:,0] for every geom            */
  PP3_DR_KP = 1,        /* actuator_gainprm[:,0] = -biasprm[:,1]         */
  PP3_DR_KD = 2,        /* -actuator_biasprm[:,2]                        */
  PP3_DR_BASE_IPOS = 3, /* body_ipos[1] (3)                               */
  PP3_DR_INERTIA = 6,   /* body_inertia[14][3]                            */
  PP3_DR_MASS = 48      /* body_mass[14]                                  */
};

/* Status codes */
enum {
  PP3_OK = 0,
  PP3_ERR_ARG = 1,
  PP3_ERR_MODEL = 2,   /* model topology / options unsupported          */
  PP3_ERR_HIP = 3,
  PP3_ERR_NOMEM = 4,
  PP3_ERR_COMM = 5     /* RCCL unavailable or a collective failed        */
};

int pp3_abi_version(void);
/* sizeof the ABI structs: which = 0 model, 1 env config (ctypes layout check). */
size_t pp3_struct_size(int which);
const char* pp3_last_error(void);
/* HIP device count (0 when no runtime / no GPU). */
int pp3_device_count(void);

/* Create a batch of `num_envs` environments on `device`.  Validates the model
 * (replaces the trace-time assert of environment.py:534 and the name lookups of
 * environment.py:183-203). */
int pp3_create(const pp3_model_t* model, const pp3_env_config_t* cfg,
               int32_t num_envs, int32_t device, pp3_env_t** out);
int pp3_destroy(pp3_env_t* env);
int32_t pp3_num_envs(const pp3_env_t* env);
int32_t pp3_state_stride(const pp3_env_t* env);
/* The HIP device the handle was created on (-1 for NULL). */
int32_t pp3_env_device(const pp3_env_t* env);

/* reset(rng): keys_dev = uint32[N][2] (one jax PRNG key per env); mask_dev =
 * optional uint8[N] (NULL = all envs).  environment.py:314-346. */
int pp3_reset(pp3_env_t* env, const uint32_t* keys_dev, const uint8_t* mask_dev, void* stream);
/* step(state, action): actions_dev = f32[N][12].  environment.py:348-483. */
int pp3_step(pp3_env_t* env, const float* actions_dev, void* stream);
/* nsteps env steps fused into one launch: the unroll of brax's PPO generate_unroll (a lax.scan of
 * env.step, [ext] brax 0.12.1 training/acting.py) with the actions given up front.  Step t reads
 * actions_dev + t * action_stride (elements; 0 = the same action every step) and is the same
 * computation as the t-th of nsteps pp3_step calls (bit for bit); the handle ends in the same
 * state.  Optional trajectory outputs (device, NULL = not written): reward_dev f32[nsteps][N],
 * done_dev f32[nsteps][N], obs_dev f32[nsteps][N][36H] -- step t's reward, done and observation
 * as pp3_step leaves them in the handle (auto-reset: the reset's obs for done envs).  Each wave
 * runs its two envs' steps back to back, so the launch ends with the slowest wave's SUM of step
 * times instead of every step waiting for that step's slowest wave.  With auto-reset and
 * action_repeat > 1 every wrapper step stays `repeat` launches. */
int pp3_rollout(pp3_env_t* env, const float* actions_dev, int64_t action_stride, int32_t nsteps, float* reward_dev,
                float* done_dev, float* obs_dev, void* stream);
/* Per-env DR parameters f32[N][62] (device), or NULL to disable DR. */
int pp3_set_dr(pp3_env_t* env, const float* dr_dev);
int pp3_set_pipeline_output(pp3_env_t* env, int32_t enable);

/* Per-env terrain (the reference's obstacles.py:16-57 boxes are static and
 * shared by all envs).  The model's world-body box geoms become per-env slots: boxes_host =
 * f32[N][n_boxes][PP3_TERRAIN_BOX] host array, per box pos[3] (world), quat[4] (w,x,y,z, any
 * norm) and half sizes[3]; a box whose half sizes are all <= 0 is absent in that env, so envs
 * may hold different numbers of boxes.  n_boxes must equal the model's world box-geom count
 * (pp3_terrain_slots).  Contact parameters (friction, solref, solimp) stay the model's.
 * boxes_host = NULL returns to the model's static boxes.  Synchronises the handle's stream. */
#define PP3_TERRAIN_BOX 10
int pp3_set_terrain(pp3_env_t* env, const float* boxes_host, int32_t n_boxes);
int32_t pp3_terrain_slots(const pp3_env_t* env);

/* Raw physics: `nsteps` x mj_step on the qpos/qvel/qacc_warmstart stored in the
 * state records, with ctrl_dev = f32[N][12] held fixed (no env logic).  Used by
 * the substep parity tests; writes the pipeline record of the last substep. */
int pp3_physics_step(pp3_env_t* env, const float* ctrl_dev, int32_t nsteps, void* stream);

/* Auto-reset mode = brax.envs.training.wrap(env, episode_length, action_repeat) on device
 * ([ext] brax 0.12.1 EpisodeWrapper + AutoResetWrapper, the wrappers Brax PPO puts around
 * PupperV3Env).  Per env: episode step counter, truncation flag and the
 * episode sum_reward / length; pp3_reset stores the reset's qpos/qvel/qacc_warmstart and obs
 * as the env's "first" state; every pp3_step then
 *   - zeroes the episode counter if the previous step was done (AutoResetWrapper.step),
 *   - runs the env step, increments the counter, sets done |= counter >= episode_length and
 *     truncation = (counter >= episode_length) & !env_done (EpisodeWrapper.step),
 *   - replaces qpos/qvel/qacc_warmstart and obs by the first state where done (the env's
 *     info -- rng, command, last action, ... -- carries over, as in Brax).
 * episode_length <= 0 turns the mode off (plain PupperV3Env.step semantics). */
#define PP3_EP_STEPS 0
#define PP3_EP_TRUNCATION 1
#define PP3_EP_SUM_REWARD 2
#define PP3_EP_LENGTH 3
#define PP3_EP_STRIDE 4
#define PP3_FIRST_STRIDE 55
int pp3_set_auto_reset(pp3_env_t* env, int32_t episode_length);
/* brax.envs.training.wrap(..., action_repeat=k) (EpisodeWrapper.step scans env.step k times with
 * the same action): in auto-reset mode every pp3_step launches the env step k times; reward =
 * the sum over the k repeats, the episode counter and length advance by k, and done, truncation
 * and the auto-reset are decided after the last repeat (the env's own done of that repeat, as in
 * Brax).  k = 1 is the plain mode; k > 1 needs auto-reset mode (PP3_ERR_ARG otherwise); turning
 * auto-reset off resets k to 1. */
int pp3_set_action_repeat(pp3_env_t* env, int32_t action_repeat);

/* Device pointer + element count per env of a field (PP3_F_*). */
int pp3_field(pp3_env_t* env, int32_t field, void** dev_ptr, int64_t* elems_per_env);
/* Synchronous host <-> device copies of a whole field (tests / host API). */
int pp3_copy_field_to_host(pp3_env_t* env, int32_t field, void* host, size_t bytes);
int pp3_copy_field_from_host(pp3_env_t* env, int32_t field, const void* host, size_t bytes);
int pp3_synchronize(pp3_env_t* env);
/* Asynchronous device -> host copy of a whole field on the handle's stream (no synchronisation:
 * pair it with pp3_synchronize).  Meant for page-locked host memory (pp3_host_malloc), which is
 * what lets it run at PCIe speed without a staging copy (the host API's per-step outputs). */
int pp3_copy_field_to_host_async(pp3_env_t* env, int32_t field, void* host, size_t bytes);
/* The host API's per-step outputs in one go (environment.py:348 `step` returns State.obs /
 * .reward / .done): a kernel on the handle's stream stores [obs N x 36H | reward N | done N] straight
 * into `host`, page-locked memory from pp3_host_malloc of at least N * (36H + 2) floats, through its
 * device mapping (no copy-engine transfer).  No synchronisation: pair it with pp3_synchronize. */
int pp3_outputs_to_host(pp3_env_t* env, float* host);
/* The device address of page-locked host memory from pp3_host_malloc, e.g. to pass a host block as
 * pp3_rollout's trajectory outputs so the step kernel stores its rows straight into host memory
 * (the host API's step). */
int pp3_host_device_ptr(void* host, void** dev_ptr);
/* The handle's own HIP stream (hipStream_t), for ordering other work (e.g. pp3_policy_act) with it. */
void* pp3_stream(pp3_env_t* env);
/* Completion markers for the host API's asynchronous step (environment.py:348 `step`: the State
 * returns at once and its obs / reward / done wait for their own step only): a HIP event (timing
 * disabled) on the handle's device, recorded on the handle's stream; synchronize waits until every
 * operation queued before its last record has completed (at once if never recorded). */
int pp3_event_create(pp3_env_t* env, void** ev_out);
int pp3_event_record(pp3_env_t* env, void* ev);
int pp3_event_synchronize(void* ev);
int pp3_event_destroy(void* ev);

/* Small device-memory helpers so a host can run without any other GPU runtime. */
int pp3_device_malloc(int32_t device, size_t bytes, void** out);
int pp3_device_free(void* ptr);
int pp3_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int pp3_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int pp3_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
/* Asynchronous host -> device copy on `stream` (from page-locked memory: the host API's actions). */
int pp3_memcpy_h2d_async(void* dst_dev, const void* src_host, size_t bytes, void* stream);
/* Page-locked host memory (hipHostMalloc) for the host API's output arrays. */
int pp3_host_malloc(size_t bytes, void** out);
int pp3_host_free(void* ptr);

/* Benchmark helpers: fill actions f32[N][12] with U(lo,hi) from a counter hash
 * keyed by (seed, step) on device; record HIP events around the step kernel
 * launches on the handle's stream so the average kernel duration can be read. */
int pp3_fill_uniform(pp3_env_t* env, float* dev, int64_t count, uint32_t seed, uint32_t ctr, float lo, float hi, void* stream);
/* nsteps back-to-back pp3_step launches on the handle's stream, step i reading actions
 * actions_dev + i * action_stride (elements; 0 = reuse); HIP events bracket the launches and
 * kernel_ms_total receives their elapsed time. */
int pp3_step_timed(pp3_env_t* env, const float* actions_dev, int64_t action_stride, int32_t nsteps,
                   float* kernel_ms_total);
/* The same for one pp3_rollout over nsteps (trajectory outputs as pp3_rollout). */
int pp3_rollout_timed(pp3_env_t* env, const float* actions_dev, int64_t action_stride, int32_t nsteps,
                      float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total);

/* Rendering (environment.py:545-547 PupperV3Env.render -> Brax PipelineEnv.render, the policy
 * videos of utils.py:214-293; not on the training path).  A z-buffer rasteriser over a triangle
 * soup built on the host by pupperv3_mjx/render.py from the model's visual geoms:
 *   tris [ntri][9]        vertices in the geom's local frame (device)
 *   tri_geom [ntri]       geom index of each triangle (device)
 *   geom_rgb [ngeom][3]   colour in 0..1 (device)
 *   geom_xf [F][ngeom][12] per frame: world rotation (row-major 3x3) then translation (device)
 *   cams [F][16]          per frame: position, right, up, forward (unit), focal length in pixels
 *                         (= height / 2 / tan(fovy / 2)), 3 pad (device)
 *   scene [17]            floor checker colours rgb1[3], rgb2[3], square size, floor height, sky
 *                         top[3], sky bottom[3], ambient, diffuse, floor on (HOST pointer)
 *   out [F][H][W][3]      u8 RGB (device)
 * Nearest fragment per pixel by a 64-bit atomicMin of (depth bits, rgb): deterministic.
 * Synchronous on `stream` (NULL = default stream); its own errors via pp3_render_last_error(). */
int pp3_render(int32_t device, const float* tris, const int32_t* tri_geom, int32_t ntri, const float* geom_rgb,
               int32_t ngeom, const float* geom_xf, const float* cams, int32_t nframes, int32_t height,
               int32_t width, const float* scene, uint8_t* out, void* stream);
const char* pp3_render_last_error(void);


/* ---------------------------------------------------------------------------------------
 * On-device MLP policy in the reference's deployment format (export.py:13-81 convert_params:
 * "layers": dense, "weights": [kernel [in][out], bias [out]], normalisation folded into the
 * first layer, final layer = Gaussian-head mean, "activation" per layer, final tanh).
 * pupperv3_mjx/export.py loads such a dict into this API.  Batch forward on the f32 matrix
 * cores (csrc/pp3_policy.hip).
 * ------------------------------------------------------------------------------------- */
typedef struct pp3_policy pp3_policy_t;
#define PP3_POLICY_MAX_LAYERS 8
#define PP3_POLICY_MAX_WIDTH 576 /* >= 36 * 15 (observation_history 15) */
enum { PP3_ACT_LINEAR = 0, PP3_ACT_RELU = 1, PP3_ACT_ELU = 2, PP3_ACT_TANH = 3, PP3_ACT_SIGMOID = 4 };
/* weights = for each layer: kernel [in][out] row-major, then bias [out] (host memory). */
int pp3_policy_create(int32_t device, int32_t in_dim, int32_t n_layers, const int32_t* out_dims,
                      const int32_t* activations, const float* weights, pp3_policy_t** out);
/* actions[i][0:out_dim] = policy(obs[i][0:in_dim]) for i < n (device pointers, strides in floats). */
int pp3_policy_act(pp3_policy_t* policy, const float* obs_dev, int64_t obs_stride, int32_t n,
                   float* actions_dev, int64_t action_stride, void* stream);
int pp3_policy_out_dim(const pp3_policy_t* policy);
int pp3_policy_destroy(pp3_policy_t* policy);
/* The unroll of brax's generate_unroll with the policy in the loop ([ext] brax 0.12.1
 * training/acting.py: actions = policy(obs), state = env.step(state, actions), nsteps times), on the
 * env's stream with no host round trip: before step t the policy acts on the env's observation
 * buffer, writing actions_dev + t * N * 12 (f32[nsteps][N][12], required: the trajectory's
 * actions), then the env steps on them; reward / done / obs trajectories as pp3_rollout
 * (optional).  ONE launch for the nsteps steps (workgroups of 16 envs run the policy's MLP, the
 * code of pp3_policy_act, before each step: the actions equal pp3_policy_act's bit for bit); with
 * max_contacts = 16 or action_repeat > 1, per step a pp3_policy_act launch then a step launch.
 * The policy must have 12 outputs and 36H inputs and live on the env's device. */
int pp3_rollout_policy(pp3_env_t* env, pp3_policy_t* policy, int32_t nsteps, float* actions_dev,
                       float* reward_dev, float* done_dev, float* obs_dev, void* stream);
/* The same bracketed by HIP events on the handle's stream (kernel_ms_total = their elapsed time). */
int pp3_rollout_policy_timed(pp3_env_t* env, pp3_policy_t* policy, int32_t nsteps, float* actions_dev,
                             float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total);
const char* pp3_policy_last_error(void);

/* ---- Stochastic policy: Brax PPO's data-collection actor (additive; PP3_ABI_VERSION stays 2) ----
 * The training form of the network keeps the whole Gaussian head: a linear last layer of 24
 * columns, loc = y[0:12] and s = y[12:24] (pupperv3_mjx/export.py convert_training_params).
 * NormalTanhDistribution ([ext] brax 0.12.1 training/distribution.py; quoted from memory):
 *   scale = (softplus(s) + min_std) * var_scale        (Brax: min_std 0.001, var_scale 1)
 *   raw = loc + scale * eps, action = tanh(raw),
 *   log_prob = sum_j [ normal_logpdf(raw_j; loc_j, scale_j) - 2 (log 2 - raw_j - softplus(-2 raw_j)) ]
 * eps is jax.random.normal(key, (N, 12)) restated on the library's threefry: sqrt(2) * erfinv of
 * jax.random.uniform(key, (N, 12), nextafter(-1, 0), 1), the word of env i, column j being element
 * i * 12 + j of the key's N * 12 random bits.  The uniform is bit-exact with jax; erfinv is the
 * device library's, not bit-pinned to XLA's erf_inv, so eps agrees with jax to f32 rounding only. */
enum { PP3_DIST_NONE = 0, PP3_DIST_NORMAL_TANH = 1 };
/* Gives the policy its head.  PP3_ERR_ARG unless kind is PP3_DIST_NORMAL_TANH, the policy has 24
 * outputs and a linear last layer, min_std >= 0 and var_scale > 0.  (A handle created with
 * device < 0 holds the layer records only, no device memory: it serves this check and the queries
 * on a host without a GPU, and every launch refuses it.) */
int pp3_policy_set_distribution(pp3_policy_t* policy, int32_t kind, float min_std, float var_scale);
/* One sample per row i < n from key (two host words): actions[i][0:12] = tanh(raw) (required),
 * and where the pointer is not null raw[i][0:12] (row stride 12), logp[i] and logits[i][0:24] (the
 * last layer as computed, row stride 24).  partitionable: the env config's rng_partitionable. */
int pp3_policy_sample(pp3_policy_t* policy, const float* obs_dev, int64_t obs_stride, int32_t n,
                      const uint32_t* key, int32_t partitionable, float* actions_dev, int64_t action_stride,
                      float* raw_dev, float* logp_dev, float* logits_dev, void* stream);
/* pp3_rollout_policy with the sampling actor in the loop: the data collection of brax's
 * generate_unroll ([ext] brax 0.12.1 training/acting.py, from memory).  Key schedule: K_0 = key;
 * at step t, (cur, next) = jax.random.split(K_t), the step samples with cur, K_{t+1} = next;
 * key_out = K_nsteps (computed on the host), so unrolls chain.  The env's rng_partitionable
 * selects the split and bits layout.  actions_dev f32[nsteps][N][12] (required: the env steps on
 * it), raw_dev f32[nsteps][N][12] and logp_dev f32[nsteps][N] (optional), reward / done / obs as
 * pp3_rollout_policy.  ONE launch for the nsteps steps where pp3_rollout_policy is one launch (the
 * head runs in the workgroup's MLP, the chain advances on the device); otherwise per step a
 * pp3_policy_sample launch with that step's key, then a step launch.  Bit for bit the same either
 * way.  The policy needs a distribution, 36H inputs and the env's device. */
int pp3_rollout_policy_sample(pp3_env_t* env, pp3_policy_t* policy, int32_t nsteps, const uint32_t* key,
                              uint32_t* key_out, float* actions_dev, float* raw_dev, float* logp_dev,
                              float* reward_dev, float* done_dev, float* obs_dev, void* stream);
/* The same bracketed by HIP events on the handle's stream (kernel_ms_total = their elapsed time). */
int pp3_rollout_policy_sample_timed(pp3_env_t* env, pp3_policy_t* policy, int32_t nsteps, const uint32_t* key,
                                    uint32_t* key_out, float* actions_dev, float* raw_dev, float* logp_dev,
                                    float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total);

/* ---- PPO batch: truncation rows and value targets (additive; PP3_ABI_VERSION stays 2) ----
 * With the sampling actor above and a 1-column critic run through pp3_policy_act
 * (pupperv3_mjx/export.py convert_value_params), these give a learner everything brax's
 * compute_ppo_loss consumes without the trajectory leaving the device
 * (PupperV3Env.collect_ppo). */
/* EpisodeWrapper's info['truncation'] per step ([ext] brax 0.12.1 envs/wrappers/training.py):
 * after this call every pp3_rollout / pp3_rollout_policy / pp3_rollout_policy_sample (and their
 * _timed forms) of nsteps <= max_steps also writes trunc_dev f32[nsteps][N], row t = the value
 * PP3_EP_TRUNCATION holds after wrapper step t (all zeros when auto-reset is off).  nsteps >
 * max_steps: PP3_ERR_ARG before anything is launched.  trunc_dev NULL (the state after
 * pp3_create) turns it off.  The buffer stays the caller's; pp3_step never writes it. */
int pp3_set_truncation_trajectory(pp3_env_t* env, float* trunc_dev, int32_t max_steps);
/* Brax PPO's generalised advantage estimation ([ext] brax 0.12.1 training/agents/ppo/losses.py
 * compute_gae as compute_ppo_loss calls it; restated from memory, the recurrence below is the
 * contract).  All device pointers; trajectory arrays [nsteps][N] with row stride `row_stride`
 * floats (>= N); bootstrap f32[N]; outputs vs (the value targets) and adv [nsteps][N], same
 * stride.  In-place is not supported (PP3_ERR_ARG if an output aliases an input).  f32, every
 * *, + and - rounded on its own in exactly this association (no fused multiply-add):
 *   for t = nsteps-1 .. 0, per env, with vnext = bootstrap and acc = 0 before the loop:
 *     tm    = 1 - truncation[t]
 *     term  = done[t] * tm                    (1 - discount_t)(1 - truncation_t), discount_t = 1 - done_t
 *     g     = discount * (1 - term)
 *     r     = reward[t] * reward_scaling
 *     delta = ((r + g * vnext) - values[t]) * tm
 *     acc   = delta + (((g * tm) * lambda) * acc)
 *     vs[t] = acc + values[t]
 *     vnext = values[t]
 *   then adv[t] = ((r_t + g_t * vs[t+1]) - values[t]) * tm_t, with vs[nsteps] = bootstrap.
 * One kernel on `stream` (NULL = default stream) of `device`, one lane per env; PP3_ERR_ARG
 * (nothing launched) on a null pointer, nsteps < 1, n < 1, row_stride < n or a non-finite
 * discount / lambda / reward_scaling.  Its own errors via pp3_ppo_last_error(). */
int pp3_gae(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward,
            const float* done, const float* truncation, const float* values, const float* bootstrap,
            float discount, float lambda, float reward_scaling, float* vs, float* adv, void* stream);
const char* pp3_ppo_last_error(void);

/* ---- PPO evaluation: episode metrics and their mean / std (additive; PP3_ABI_VERSION stays 2) ----
 * What Brax's Evaluator reports ([ext] brax 0.12.1 envs/wrappers/training.py EvalWrapper and
 * training/acting.py Evaluator, restated from memory; what is written here is the contract).  Free
 * functions on raw device pointers, in pp3_gae's style; errors through pp3_ppo_last_error().
 *
 * The accumulator acc is f32[PP3_EVAL_WORDS][n], column c of env i at acc[c * n + i]:
 *   columns 0 .. 19   episode_metrics: total_dist, the 18 reward terms in PP3_REWARD_* order (the 19
 *                     words of PP3_F_METRICS), then reward
 *   PP3_EVAL_ACTIVE   active_episodes: 1 until the env's first done, 0 afterwards
 *   PP3_EVAL_STEPS    episode_steps: the episode counter at the env's first done
 * pp3_eval_reset: all zeros, active = 1.
 * pp3_eval_accumulate: one wrapper step (auto-reset mode) of every env, from the env's buffers after
 * that step: reward [n] and done [n] (PP3_F_REWARD, PP3_F_DONE), metrics [n][metrics_stride]
 * (PP3_F_METRICS, the first PP3_NMETRIC words of a row) and episode [n][episode_stride]
 * (PP3_F_EPISODE, word PP3_EP_STEPS of a row, which after a done step still holds the finished
 * episode's count).  Per env, f32, * and + each rounded on their own (no fused multiply-add):
 *   episode_steps      = active != 0 ? steps : episode_steps
 *   episode_metrics[c] = episode_metrics[c] + x[c] * active       x = (metrics[0 .. 18], reward)
 *   active             = active * (1 - done)
 * pp3_eval_accumulate_rows: the same three lines on the reward column, active and episode_steps for
 * the nsteps wrapper steps of a fused launch, from its reward / done trajectories [nsteps][n] (row
 * stride row_stride floats), t = 0 .. nsteps-1 in step order, with steps = (step0 + t + 1) *
 * action_repeat: the episode counter of an env that was reset step0 wrapper steps before row 0 and
 * has not been done since, which is every env that is still active.  Columns 0 .. 18 are not touched.
 * pp3_eval_reduce: out42[k] = mean and out42[PP3_EVAL_NOUT + k] = population standard deviation
 * (ddof 0) over the n envs of reduced column k: k < 20 the metrics columns, k = 20 episode_steps.
 * One 1024-lane workgroup, f32, every operation rounded on its own, in this order: lane i adds
 * envs i, i + 1024, .. ascending from 0; the 1024 lane sums meet in a binary tree (for s = 512,
 * 256, .. 1: sum[j] = sum[j] + sum[j + s], j < s); mean = sum / n; the second pass sums (x - mean) *
 * (x - mean) in the same order; std = sqrt(that sum / n).  Both quotients and the root are correctly
 * rounded (one residual step on the build's fast division and square root; rare double roundings
 * excepted).  No atomics: a call repeats bit for bit.
 * One kernel each on `stream` (NULL = default stream) of `device`, one lane per env for the first
 * three.  PP3_ERR_ARG (nothing launched): a null pointer, n < 1, nsteps < 1, metrics_stride <
 * PP3_NMETRIC, episode_stride < PP3_EP_STRIDE, row_stride < n, step0 < 0, action_repeat < 1, (step0 +
 * nsteps) * action_repeat >= 2^24 (the counter stays exact in f32), or the accumulator (pp3_eval_reduce:
 * out42) overlapping an input. */
#define PP3_EVAL_NCOL 20
#define PP3_EVAL_ACTIVE 20
#define PP3_EVAL_STEPS 21
#define PP3_EVAL_WORDS 22
#define PP3_EVAL_NOUT 21
int pp3_eval_reset(int32_t device, int32_t n, float* acc, void* stream);
int pp3_eval_accumulate(int32_t device, int32_t n, const float* reward, const float* done, const float* metrics,
                        int64_t metrics_stride, const float* episode, int64_t episode_stride, float* acc,
                        void* stream);
int pp3_eval_accumulate_rows(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward,
                             const float* done, int32_t step0, int32_t action_repeat, float* acc, void* stream);
int pp3_eval_reduce(int32_t device, int32_t n, const float* acc, float* out42, void* stream);

/* ---- PPO metrics: rank-ordered sums, the evaluation reduce over ranks, training episode statistics
 * (additive; PP3_ABI_VERSION stays 2) ----
 * Free functions on raw device pointers in pp3_gae's style: f32, every operation rounded on its own
 * (no fused multiply-add), no atomics (a call repeats bit for bit), errors through
 * pp3_ppo_last_error(), PP3_ERR_ARG before any launch with the outputs untouched.  None of them makes
 * a collective: a sum over ranks is pp3_comm_allgather_f32 into [world][count], then
 * pp3_sum_gathered_f32 (pupperv3_mjx sharding.Comm.sum_ranks_device), the same bits on every rank.
 *
 * pp3_sum_gathered_f32: out[i] = ((g_0[i] + g_1[i]) + g_2[i]) + .. over the rows g_r = gathered[r]
 * of gathered f32[world][count], in rank order starting from rank 0's value (world 1: a copy).
 * PP3_ERR_ARG: a null pointer, world outside 1 .. PP3_LEARN_MAX_WORLD, count outside 1 .. 2^30, out
 * overlapping gathered.
 *
 * pp3_eval_reduce cut at the two places where the sum over ranks goes in.  acc is a pp3_eval_*
 * accumulator of this rank's n eval envs; reduced column k is metrics column k for k < 20 and
 * episode_steps for k = 20.
 * pp3_eval_column_sums, mean21 NULL: out22[k] = the sum of reduced column k over the n envs in
 * pp3_eval_reduce's order (one 1024-lane workgroup; lane i adds envs i, i + 1024, .. ascending from 0,
 * then the binary tree), k < 21; out22[21] = (float)n.  mean21 given (f32[21], device): out22[k] = the
 * sum of (x - mean21[k]) * (x - mean21[k]) in the same order; out22[21] = (float)n.
 * pp3_eval_finish, which 0: out42[k] = sums22[k] / sums22[21]; which 1: out42[21 + k] =
 * sqrt(sums22[k] / sums22[21]); k < 21, the quotient and the root those of pp3_eval_reduce (one
 * residual step each).  The other half of out42 is left alone.
 * The chain: column_sums(NULL) -> sum over ranks -> finish(0) -> column_sums(out42) -> sum over
 * ranks -> finish(1).  On one rank's data alone (world 1) it equals pp3_eval_reduce bit for bit.
 * Over ranks the mean and the std weigh every eval env of the job equally, whatever its rank's
 * shard size: both sums and the env count are summed, so ragged shards are exact.  This is not
 * Brax's pmean of per-device means, which weighs every device equally; the two agree when all
 * shards have the same size.  The env count must stay below 2^24 (exact in f32).
 * PP3_ERR_ARG: a null pointer other than mean21, n < 1, which not 0 or 1, an output overlapping an
 * input.
 *
 * Training episode statistics: EpisodeWrapper's episode_metrics (sum_reward, length) at the done steps
 * of a collected batch ([ext] brax 0.12.1 envs/wrappers/training.py and ppo.train's
 * log_training_metrics, restated from memory; what is written here is the contract).  A fused K-step
 * rollout leaves only the record's last value in PP3_F_EPISODE; these rebuild the record at every
 * step from the batch's rows with the step kernel's own arithmetic.
 * pp3_episode_stats_begin, queued before the rollout: carry f32[3][n] (row r of env i at carry[r * n +
 * i]) from the env's fields: ret = word PP3_EP_SUM_REWARD and len = word PP3_EP_LENGTH of episode
 * [n][episode_stride] (PP3_F_EPISODE), pd = done [n] (PP3_F_DONE).
 * pp3_episode_stats_rows, queued after the rollout, on its reward / done / truncation rows
 * [nsteps][n] (row stride row_stride floats; truncation NULL is read as all 0).  Per env i, for
 * t = 0 .. nsteps-1 in order, with cnt = sret = slen = strunc = 0 before the loop in every call:
 *     keep = 1 - pd
 *     ret  = (ret + reward[t][i]) * keep
 *     len  = (len + (float)action_repeat) * keep
 *     if done[t][i] != 0:
 *         cnt = cnt + 1;  sret = sret + ret;  slen = slen + len;  strunc = strunc + truncation[t][i]
 *     pd   = done[t][i]
 * This is the step kernel's line for the record, so the step after a done step contributes nothing
 * (as in Brax, whose record restarts one step late), and carry (written back: ret, len, pd) equals
 * the env's PP3_F_EPISODE words and PP3_F_DONE after the rollout bit for bit.  part f32[4][n] is the
 * caller's workspace and receives (cnt, sret, slen, strunc) per env; out4 f32[4] = (episodes, sum of
 * returns, sum of lengths, truncated episodes): each row of part summed over the envs in
 * pp3_eval_reduce's order.  Two kernels: the chain, one lane per env with the next rows' loads in
 * flight ahead of it, then the one-workgroup sum.
 * PP3_ERR_ARG: a null pointer other than truncation, n < 1, nsteps < 1, row_stride < n,
 * action_repeat < 1, episode_stride < PP3_EP_STRIDE, nsteps * n >= 2^24 (the count stays exact in
 * f32), carry / part / out4 overlapping an input or each other. */
int pp3_sum_gathered_f32(int32_t device, const float* gathered, int32_t world, int64_t count, float* out,
                         void* stream);
int pp3_eval_column_sums(int32_t device, int32_t n, const float* acc, const float* mean21, float* out22,
                         void* stream);
int pp3_eval_finish(int32_t device, const float* sums22, int32_t which, float* out42, void* stream);
int pp3_episode_stats_begin(int32_t device, int32_t n, const float* episode, int64_t episode_stride,
                            const float* done, float* carry, void* stream);
int pp3_episode_stats_rows(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward,
                           const float* done, const float* truncation, int32_t action_repeat, float* carry,
                           float* part, float* out4, void* stream);

/* ---- PPO learner: loss gradients, Adam, weight reload (additive; PP3_ABI_VERSION stays 2) ----
 * One PPO iteration on the env's stream with no host round trip: collect, per minibatch loss +
 * gradient + Adam, reload the actor and the critic, collect again (csrc/pp3_learn.hip).  All f32.
 * The formulas restate [ext] brax 0.12.1 training/agents/ppo/losses.py compute_ppo_loss and optax
 * adam from memory; what is written here is the contract.
 *
 * Networks: two MLPs in pp3_policy_create's format (at most 8 layers, widths at most
 * PP3_POLICY_MAX_WIDTH, PP3_ACT_* activations, last layer linear): the policy with 24 outputs and
 * the PP3_DIST_NORMAL_TANH head (min_std, var_scale), the value net with 1 output.  The trainable
 * parameters live on the device as one f32 blob per net in pp3_policy_create's `weights` layout
 * (per layer: kernel [in][out] row-major, then bias [out]), UN-folded: the normaliser is separate.
 * Gradients and both Adam moments have the same layout.
 *
 * Minibatch: the contiguous env range [e0, e0 + B) of a collected batch of N envs and K steps,
 * R = K B rows, read in place through the row stride N: obs_all [K+1][N][in_dim] (the buffer behind
 * PupperV3Env.collect_ppo's "observation" and "obs"), raw_action [K][N][12], log_prob / reward /
 * done / truncation [K][N], the caller's entropy noise eps [K][N][12], and the optional normaliser
 * mean[in_dim], std[in_dim] (both NULL: identity).
 *
 * Loss:
 *   x = (obs - mean) / std
 *   baseline[t][e] = V(x[t][e]) for t < K, bootstrap[e] = V(x[K][e])
 *   (vs, adv) = the pp3_gae recurrence on reward, done, truncation, baseline, bootstrap with
 *       discount, gae_lambda, reward_scaling; both are constants for the gradient, and the
 *       bootstrap rows receive none
 *   normalize_advantage: adv <- (adv - mean_R adv) / (std_R adv + 1e-8), the population std
 *   logits = pi(x[t][e]) for t < K; loc = logits[0:12], s = logits[12:24],
 *       scale = (softplus(s) + min_std) * var_scale; logp = the head's log_prob(logits, raw_action)
 *       as stated above pp3_policy_sample; rho = exp(logp - log_prob)
 *   policy_loss  = -mean_R min(rho adv, clip(rho, 1 - clip_eps, 1 + clip_eps) adv)
 *   v_loss       = 0.25 mean_R (vs - baseline)^2
 *   entropy_loss = -entropy_cost mean_R sum_j [ 1/2 + 1/2 log 2 pi + log scale_j
 *                                               + 2 (log 2 - a_j - softplus(-2 a_j)) ],
 *       a_j = loc_j + scale_j eps_j (the gradient flows through a_j into loc and scale)
 *   total = policy_loss + v_loss + entropy_loss
 * Outputs: d total / d (every policy and value parameter) into the learner's gradient blobs
 * (overwritten each call, not accumulated) and metrics_dev f32[4] = total, policy, value, entropy.
 * The matrix products run on the exact-f32 MFMA; the weight gradient sums rows in chunks of
 * PP3_LEARN_ROW_CHUNK and the chunks in ascending order, no atomics: a call repeats bit for bit.
 *
 * Adam, with c1 = 1 - b1^t and c2 = 1 - b2^t from the host as f32 (no fused multiply-add):
 *   m <- b1 m + (1 - b1) g;   v <- b2 v + ((1 - b2) g) g;
 *   p <- p - (lr (m / c1)) / (sqrt(v / c2) + eps)
 * ------------------------------------------------------------------------------------------- */
typedef struct pp3_learner pp3_learner_t;
#define PP3_LEARN_ROW_CHUNK 256
/* Owns the parameter, gradient and moment blobs of both nets (the moments start at zero, the
 * parameters from the host blobs given here) and the workspace for minibatches of up to max_rows
 * rows, counting the bootstrap rows: (K + 1) B <= max_rows.  PP3_ERR_ARG on a null pointer, a
 * shape outside the format above, a policy not 24 wide, a value net not 1 wide, a non-linear last
 * layer, min_std < 0, var_scale <= 0, or max_rows outside 2 .. 2^21. */
int pp3_learner_create(int32_t device, int32_t in_dim, int32_t policy_layers, const int32_t* policy_out_dims,
                       const int32_t* policy_acts, const float* policy_weights, int32_t value_layers,
                       const int32_t* value_out_dims, const int32_t* value_acts, const float* value_weights,
                       float min_std, float var_scale, int64_t max_rows, pp3_learner_t** out);
int pp3_learner_destroy(pp3_learner_t* learner);
/* Device pointer and element count of a blob: net 0 = policy, 1 = value; which 0 = parameters,
 * 1 = gradients, 2 = Adam m, 3 = Adam v. */
int pp3_learner_buffers(pp3_learner_t* learner, int32_t net, int32_t which, float** ptr, int64_t* count);
/* The loss and its gradients on one minibatch (all batch pointers on the learner's device).
 * PP3_ERR_ARG with nothing launched and no output touched: a null pointer (mean and std_dev may
 * both be NULL, not one of them), batch < 1, nsteps < 1, e0 < 0 or e0 + batch > num_envs,
 * (nsteps + 1) * batch over max_rows, a non-finite hyper-parameter, clip_eps <= 0. */
int pp3_ppo_loss_grad(pp3_learner_t* learner, int32_t nsteps, int32_t batch, int32_t num_envs, int32_t e0,
                      const float* obs_all, const float* raw_action, const float* log_prob, const float* reward,
                      const float* done, const float* truncation, const float* eps, const float* mean,
                      const float* std_dev, float discount, float gae_lambda, float reward_scaling, float clip_eps,
                      float entropy_cost, int32_t normalize_advantage, float* metrics_dev, void* stream);
/* One Adam step of both nets from their gradient blobs.  PP3_ERR_ARG (nothing launched) on a null
 * learner, a non-finite argument, c1 <= 0 or c2 <= 0. */
int pp3_adam_step(pp3_learner_t* learner, float lr, float b1, float b2, float eps, float c1, float c2,
                  void* stream);
/* Overwrites an existing handle's fragment-order weights from a device blob in the layout above
 * (in_dim, n_layers, out_dims: the blob's shape, which must be the handle's; PP3_ERR_ARG before
 * any launch otherwise, or for a host-side handle).  Layer 0 is folded with the normaliser:
 *   W'[k][m] = W[k][m] / std[k],   b'[m] = b[m] - sum_k (mean[k] / std[k]) W[k][m], k ascending;
 * mean_dev and std_dev both NULL: a pure repack, bit for bit what pp3_policy_create packs from the
 * same values.  The handle then serves pp3_policy_act, pp3_policy_sample and pp3_rollout_policy*
 * unchanged; work queued on `stream` before this call sees the old weights. */
int pp3_policy_load_params(pp3_policy_t* policy, const float* params_dev, int32_t in_dim, int32_t n_layers,
                           const int32_t* out_dims, const float* mean_dev, const float* std_dev, void* stream);

/* ---- PPO learner: running normaliser, shuffled minibatches, gradient clip (additive; ABI stays 2) ----
 * What [ext] brax 0.12.1 training_step does around compute_ppo_loss, restated from memory (brax
 * running_statistics.update, jax.random.permutation in sgd_step, optax.clip_by_global_norm); what is
 * written here is the contract.  f32, fixed-order sums, no atomics: a call repeated on the same
 * inputs gives the same bits.  Errors are PP3_ERR_ARG through pp3_learn_last_error() before
 * anything is launched, outputs untouched.
 *
 * pp3_learner_normalizer_update: one running_statistics.update of (mean, summed_variance, std_dev),
 * each [in_dim] on the device and updated in place, from obs [rows][in_dim] (contiguous; in_dim is
 * the learner's).  count_new is the old count plus rows, kept by the host as an integer and passed
 * rounded to f32 (as Adam's c1 and c2 are).  Per column k:
 *   d_old[r] = obs[r][k] - mean[k]
 *   mean'[k] = mean[k] + (sum_r d_old[r]) / count_new
 *   sv'[k]   = sv[k] + sum_r d_old[r] * (obs[r][k] - mean'[k])
 *   std'[k]  = clip(sqrt(max(sv'[k], 0) / count_new), std_min, std_max)
 * both quotients correctly rounded.  Brax starts from count 0, mean 0, summed_variance 0, std 1, with
 * std_min = 1e-6 and std_max = 1e6.  The rows of a collect_ppo batch are rows 0 .. K-1 of its
 * [K+1][N][in_dim] observation buffer: rows = K N from its base; the bootstrap row K is not read.
 * Two sweeps over obs (the second needs mean').  The rows are summed in 1024 equal ranges (of
 * ceil(rows / 1024) rows) into a workspace the learner owns, then the ranges; the order depends on
 * (rows, in_dim) alone and rows is not bounded by max_rows.
 * PP3_ERR_ARG: a null pointer, rows < 1, count_new not finite or < rows, std_min or std_max not
 * finite, or not 0 < std_min <= std_max. */
int pp3_learner_normalizer_update(pp3_learner_t* learner, const float* obs, int64_t rows, float count_new,
                                  float std_min, float std_max, float* mean, float* summed_variance, float* std_dev,
                                  void* stream);
/* Shuffled minibatches.  pp3_learner_set_env_index validates on the host that num_envs >= 1 and
 * every entry of index_host[num_envs] lies in [0, num_envs) (else PP3_ERR_ARG and nothing is copied:
 * an invalid index never reaches a kernel), then copies it into a device buffer the learner owns,
 * in stream order: work queued on `stream` earlier keeps the old index, and index_host is free
 * again on return.  pp3_ppo_loss_grad_indexed is pp3_ppo_loss_grad (same parameters, results and
 * errors) except that row e of the minibatch reads env index[e0 + e] of every batch array, eps
 * included, where pp3_ppo_loss_grad reads env e0 + e; further PP3_ERR_ARG: no index set, or the
 * index's num_envs differs from the call's.  The index need not be a permutation. */
int pp3_learner_set_env_index(pp3_learner_t* learner, const int32_t* index_host, int32_t num_envs, void* stream);
int pp3_ppo_loss_grad_indexed(pp3_learner_t* learner, int32_t nsteps, int32_t batch, int32_t num_envs, int32_t e0,
                              const float* obs_all, const float* raw_action, const float* log_prob,
                              const float* reward, const float* done, const float* truncation, const float* eps,
                              const float* mean, const float* std_dev, float discount, float gae_lambda,
                              float reward_scaling, float clip_eps, float entropy_cost, int32_t normalize_advantage,
                              float* metrics_dev, void* stream);
/* optax.clip_by_global_norm on the learner's gradient blobs, between the loss and pp3_adam_step:
 *   s = sum of g^2 over the policy blob, then the value blob (chunks of 4096 elements, then the
 *   chunks, each in a fixed order);  norm = sqrt(s), written to norm_dev f32[1] when it is not NULL;
 *   norm < max_norm: the gradients stay bit for bit as they were;  else g <- (g / norm) * max_norm.
 * PP3_ERR_ARG: a null learner, max_norm not finite or <= 0. */
int pp3_grad_clip(pp3_learner_t* learner, float max_norm, float* norm_dev, void* stream);

/* ---- PPO learner across ranks: rank-ordered gradient and statistics reduce (additive; ABI stays 2) ----
 * Data-parallel PPO over a communicator handle, pp3_comm_t: what [ext] brax 0.12.1 training_step does
 * under pmap, restated from memory; what is written here is the contract.  Every rank holds a replica
 * of the learner, collects and differentiates on its own env shard, and the replicas stay bit-identical
 * because every cross-rank sum has ONE order.  ncclAllReduce promises no order of additions, so it is
 * not used: each rank all-gathers the ranks' contributions ([world][count], rank r's at row r) and a
 * kernel adds them in rank order, starting from rank 0's value, in f32, each addition rounded on its
 * own.  Every rank computes the same bits from the same gathered data, whatever the transport.  The
 * ranks must start from identical parameters, moments and statistics; each passes its own PRNG key.
 * Errors are PP3_ERR_ARG through pp3_learn_last_error before any launch or collective, outputs
 * untouched: a null pointer, a world size outside 1 .. PP3_LEARN_MAX_WORLD, a communicator on another
 * device than the learner's (and the per-call conditions below).  A failing collective returns
 * PP3_ERR_COMM.  All calls are enqueued on `stream` with no host synchronisation; the workspaces
 * belong to the learner and are allocated at the first call for a given world size.
 *
 * 1. Gradients and metrics (jax.lax.pmean of both).  After a pp3_ppo_loss_grad* call, for every element
 * i of "policy gradient blob, then value gradient blob, then the 4 metrics" (count = policy count +
 * value count + 4):
 *   g[i] <- (((g_0[i] + g_1[i]) + g_2[i]) + ..) / (float)world, the quotient correctly rounded
 * (world = 1: g[i] itself, bit for bit).  The mean is unweighted, as Brax's: with shards of unequal
 * size a rank's rows weigh 1 / (world * its row count), which is the caller's business.  Advantage
 * normalisation stays local to the rank's minibatch, as in Brax.  pp3_grad_clip and pp3_adam_step then
 * run unchanged on the averaged gradient (optax's chain order).
 * pp3_learner_allreduce_grads: ONE collective per minibatch: a kernel packs the three pieces into one
 * contiguous send of `count` floats, one all-gather, then the reduce kernel; it reads and rewrites
 * the learner's gradient blobs and metrics_dev f32[4].  No shortcut at world = 1.
 * pp3_learner_reduce_gathered: the reduce kernel on its own, from gathered_dev [world][count] on the
 * learner's device into both gradient blobs and metrics_dev (one launch, no collective): what
 * pp3_learner_allreduce_grads runs after its gather, for tests and measurements at any world size.
 *
 * 2. Running statistics (running_statistics.update with pmap_axis_name: its two psums).
 * pp3_learner_normalizer_update_ranks is pp3_learner_normalizer_update (same arguments, and its errors)
 * with obs [rows][in_dim] this rank's own rows and count_new = the old count + the sum over ranks of
 * their rows (the caller's; finite and >= rows).  Per column k, the rank sums starting from rank 0's
 * term:
 *   S_r      = sum over rank r's rows of (obs[.][k] - mean[k])
 *   mean'[k] = mean[k] + ((S_0 / count_new + S_1 / count_new) + ..)     each quotient correctly rounded
 *   V_r      = sum over rank r's rows of (obs[.][k] - mean[k]) * (obs[.][k] - mean'[k])
 *   sv'[k]   = sv[k] + ((V_0 + V_1) + ..)
 *   std'[k]  = clip(sqrt(max(sv'[k], 0) / count_new), std_min, std_max)
 * S_r and V_r are summed over the rank's own rows in the order pp3_learner_normalizer_update fixes for
 * (rows, in_dim).  Each sweep is followed by an all-gather of in_dim floats (two collectives per
 * update).  At world = 1 the result is pp3_learner_normalizer_update's bit for bit. */
#define PP3_LEARN_MAX_WORLD 64
typedef struct pp3_comm pp3_comm_t; /* the communicator of the Multi-GPU section below */
int pp3_learner_allreduce_grads(pp3_learner_t* learner, pp3_comm_t* comm, float* metrics_dev, void* stream);
int pp3_learner_reduce_gathered(pp3_learner_t* learner, const float* gathered_dev, int32_t world, float* metrics_dev,
                                void* stream);
int pp3_learner_normalizer_update_ranks(pp3_learner_t* learner, pp3_comm_t* comm, const float* obs, int64_t rows,
                                        float count_new, float std_min, float std_max, float* mean,
                                        float* summed_variance, float* std_dev, void* stream);

/* ---- PPO learner: entropy noise and minibatch shuffle drawn on the device (additive; ABI stays 2) ----
 * The two random inputs of an iteration that pupperv3_mjx/rng.py draws on the host, restated on the
 * device from the sampling head's threefry (csrc/pp3_mlp.h), in both jax_threefry_partitionable
 * layouts (`partitionable` != 0: jax 0.5's default).  Both are enqueued on `stream` with no host copy
 * and no host synchronisation; a call repeated with the same key gives the same bits.  Errors are
 * PP3_ERR_ARG through pp3_learn_last_error() before any GPU work, outputs untouched.
 *
 * pp3_learner_draw_noise: jax.random.normal(key, (nsteps, num_envs, 12)) into a buffer the learner owns
 * (allocated at the first call, grown when a call needs more, freed by pp3_learner_destroy; a later
 * call overwrites it, and one that grows it waits for the queued work that reads the old one), whose
 * device address it returns in *eps_dev_out: the `eps` of pp3_ppo_loss_grad*.  With count = nsteps *
 * num_envs * 12, flat element i is
 *   1.41421356f * erfinvf(u_i),  u_i = jax.random.uniform(key, (count,), minval = nextafter(-1, 0), maxval = 1)[i]
 * in f32 without FMA contraction: the sampling head's recipe, one thread per element.  u_i is jax's bit
 * for bit; erfinvf is the device library's, so the values agree with rng.normal (scipy's float64 erfinv
 * rounded to f32) and with XLA to f32 rounding, not bitwise.
 * PP3_ERR_ARG: a null pointer, nsteps < 1, num_envs < 1, count >= 2^31.
 *
 * pp3_permute_by_bits: x := x[stable_argsort(bits)] in place, bits_dev uint32 [n] and x_dev int32 [n] on
 * `device`: one round of jax's _shuffle, exposed so that equal bits can be tested.  One workgroup sorts
 * the 64-bit keys (bits[i] << 32) | i, padded to a power of two with all-ones keys, in a bitonic
 * network: in LDS for n <= 8192, above that in a global scratch buffer that this call allocates and
 * frees (it then waits for the sort; the learner's shuffle keeps its own).  PP3_ERR_ARG: a null
 * pointer, device < 0, n outside 1 .. 65536.
 *
 * pp3_learner_shuffle_env_index: jax.random.permutation(key, num_envs) into the learner's env index,
 * the buffer pp3_learner_set_env_index fills and pp3_ppo_loss_grad_indexed reads (afterwards the index
 * is set for num_envs), bit for bit rng.permutation:
 *   rounds = ceil(3 ln(num_envs) / ln(2^32 - 1)) in double  (1 env: 0; up to 1625: 1; up to 65536: 2)
 *   x = arange(num_envs); per round: key, sub = split(key) on the host;
 *   bits = random_bits(sub, (num_envs,)) 32-bit words, one thread each;  x := x[stable_argsort(bits)]
 * PP3_ERR_ARG: a null pointer, num_envs outside 1 .. 65536 (the one-workgroup sort's range).
 *
 * pp3_learner_rng_buffers: the device addresses behind the two (tests, checkpoints): the env index and
 * the entries it is set for (NULL and 0: none set), the noise buffer and its capacity in floats (NULL
 * and 0: pp3_learner_draw_noise was never called).  PP3_ERR_ARG: a null pointer. */
int pp3_learner_draw_noise(pp3_learner_t* learner, const uint32_t key[2], int32_t nsteps, int32_t num_envs,
                           int32_t partitionable, float** eps_dev_out, void* stream);
int pp3_permute_by_bits(int32_t device, const uint32_t* bits_dev, int32_t n, int32_t* x_dev, void* stream);
int pp3_learner_shuffle_env_index(pp3_learner_t* learner, const uint32_t key[2], int32_t num_envs,
                                  int32_t partitionable, void* stream);
int pp3_learner_rng_buffers(pp3_learner_t* learner, int32_t** index_dev, int32_t* index_n, float** noise_dev,
                            int64_t* noise_count);

/* ---- PPO learner: network initialisation on the device (additive; ABI stays 2) ----
 * Restated from memory of jax `nn.initializers.lecun_uniform` (variance_scaling(1.0, "fan_in",
 * "uniform")) and Brax `make_ppo_networks` (MLPs whose kernels take lecun_uniform and whose biases are
 * zero); what is written here is the contract.
 *
 * pp3_learner_init_params overwrites both parameter blobs and zeroes both gradient blobs and both
 * nets' Adam moments m and v, enqueued on `stream` with no host copy and no host synchronisation (one
 * launch per net, one thread per blob element; the caller's Adam step count restarts at 0).  A call
 * repeated with the same key gives the same bits, and so does every rank that passes the same key.
 *
 * Keys (two-way jax.random.split on the host, in the `partitionable` layout):
 *   k_policy, k_value = split(key)
 *   inside a net, for layer l = 0 .. L-1 in order:  k_net, k_l = split(k_net)
 * This schedule is this library's own.  Flax derives a layer's key by folding the module's path into
 * the init key, which depends on module names that cannot be pinned here; the distribution of every
 * kernel is flax's, the stream behind it is not.
 *
 * Layer l with fan_in rows and `out` columns (blob layout [in][out] row-major, then the bias):
 *   kernel element i = u_i * s
 *   u_i = jax.random.uniform(k_l, (fan_in, out), float32, minval = -1, maxval = 1) flat element i, bit
 *         for bit (count = fan_in * out; both counter layouts, the pre-0.5 one zero-padding an odd count)
 *   s   = sqrtf(3.0f * (1.0f / (float)fan_in)), f32 on the host
 *   one f32 multiply, no FMA contraction; every entry lies in [-s, s)
 *   bias = 0
 * pupperv3_mjx/ppo.py init_params is the same in numpy.
 * PP3_ERR_ARG through pp3_learn_last_error() before any launch: a null learner or key; the blobs are
 * untouched. */
int pp3_learner_init_params(pp3_learner_t* learner, const uint32_t key[2], int32_t partitionable, void* stream);
const char* pp3_learn_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU (no reference code: the reference runs one process per device under
 * Brax PPO's pmap, [ext] brax 0.12.1 brax/training/agents/ppo/train.py, where the env batch is
 * sharded across devices and XLA gathers it).  One process per GPU, each owning a contiguous
 * shard of the global env batch (pupperv3_mjx/sharding.py); envs never exchange data inside a
 * step.  The only data-path collective is the optional per-step hand-over of the learner batch
 * obs | reward | done over RCCL (xGMI), launched on the env's stream behind the step kernel with
 * no host synchronisation.  RCCL is dlopen'ed on first use (the single-GPU path never loads it).
 * ------------------------------------------------------------------------------------- */
/* the handle type pp3_comm_t is declared above pp3_learner_allreduce_grads */
#define PP3_COMM_ID_BYTES 128 /* ncclUniqueId */
enum { PP3_REDUCE_SUM = 0, PP3_REDUCE_MAX = 1 };
/* Rank 0 creates the communicator id and hands its 128 bytes to the other ranks out of band. */
int pp3_comm_unique_id(uint8_t* id_out);
int pp3_comm_init(const uint8_t* id, int32_t rank, int32_t world, int32_t device, pp3_comm_t** out);
int pp3_comm_destroy(pp3_comm_t* comm);
int32_t pp3_comm_rank(const pp3_comm_t* comm);
int32_t pp3_comm_world(const pp3_comm_t* comm);
const char* pp3_comm_last_error(void);
/* Learner batch of every rank's env shard: each rank contributes nmax rows (nmax >= its env
 * count; rows past the count are zero) of width 36H + 2 = [obs | reward | done], rank r's rows
 * at dst_dev + r * nmax * (36H + 2).  root >= 0: gather to rank `root` (grouped send/recv,
 * dst_dev needed on the root only); root < 0: all-gather (dst_dev on every rank).  Enqueued on
 * `stream` (NULL = the env's stream): ordered after the env's last step, no host sync.  The env
 * must live on the communicator's device (PP3_ERR_ARG otherwise); the caller's current HIP device
 * is restored on return. */
int pp3_gather(pp3_comm_t* comm, pp3_env_t* env, int32_t nmax, int32_t root, float* dst_dev, void* stream);
/* The same hand-over for a K-step unroll (replaces the per-device trajectory of Brax's
 * generate_unroll, [ext] brax 0.12.1 brax/training/acting.py, that PPO's pmap hands to the learner
 * once per unroll): the trajectory outputs of one fused pp3_rollout of this env (traj_obs
 * [nsteps][N][36H], traj_reward / traj_done [nsteps][N], device pointers) -> rank r's block
 * [nsteps][nmax][36H + 2] at dst_dev + r * nsteps * nmax * (36H + 2); rows past the rank's env
 * count are zero.  ONE collective per unroll instead of one per step; root, stream and device
 * rules as pp3_gather. */
int pp3_gather_rollout(pp3_comm_t* comm, pp3_env_t* env, const float* traj_obs, const float* traj_reward,
                       const float* traj_done, int32_t nsteps, int32_t nmax, int32_t root, float* dst_dev,
                       void* stream);
/* A plain device all-gather of f32: rank r's `count` floats at send_dev land at recv_dev + r * count on
 * every rank (recv_dev holds world * count floats; both on the communicator's device).  Enqueued on
 * `stream` (NULL = the default stream) with no host synchronisation; the caller's current HIP device
 * is restored on return.  PP3_ERR_ARG (no collective): a null pointer, count < 1.  The learner's
 * rank-ordered reduces are built on it. */
int pp3_comm_allgather_f32(pp3_comm_t* comm, const float* send_dev, float* recv_dev, int64_t count, void* stream);
/* The device the communicator was created on (-1 for NULL). */
int32_t pp3_comm_device(const pp3_comm_t* comm);
/* Host-blocking helpers for timing: element-wise sum / max of n <= 64 doubles over ranks, and
 * a barrier. */
int pp3_comm_allreduce(pp3_comm_t* comm, const double* in, double* out, int32_t n, int32_t op);
int pp3_comm_barrier(pp3_comm_t* comm);

#ifdef __cplusplus
}
#endif
#endif /* PUPPER_HIP_H_ */
