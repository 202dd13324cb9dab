/*
 * hydro.h - C ABI of the MI355X-native hydrodynamic force engine (libhydro.so).
 *
 * Drop-in boundary for the per-body, per-physics-step hydrodynamic wrench of
 * Joagai23/silver2_isaacsim.  Each entry point names the reference interface it
 * replaces (paths relative to the reference repo).  Plain pointers and sizes
 * only; no C++ or torch types.  All `state` / `wrench` / `params` pointers are
 * struct-of-arrays: one contiguous float array of length >= n per scalar field,
 * in DEVICE memory unless an argument says otherwise.  The caller owns every
 * array it passes; the engine owns per-body parameters, the previous-step
 * velocity and its reduction scratch.
 *
 * Field orders
 *   state  [13]: px py pz | qx qy qz qw | vx vy vz | wx wy wz     (quaternion xyzw)
 *   prev   [ 6]: vx vy vz | wx wy wz at the previous physics step
 *   params [11]: dimx dimy dimz | cd_lin cd_ang | damp_lin damp_ang | lift |
 *                am_lin am_ang | mass
 *   wrench [ 6]: Fx Fy Fz | Tx Ty Tz       (net world-frame force / torque at the body origin)
 *   comps  [24]: buoyancy_force, drag_force, lift_force, drag_torque, added_mass_force,
 *                added_mass_torque, center_of_buoyancy, center_of_pressure (x,y,z each) - the
 *                order of the reference's return tuple (numba_hydrodynamics.py:314)
 *
 * Error model: every function returns an int status, 0 = OK, <0 =
 * HYDRO_E_*; nothing aborts or throws.  hydro_last_error(h) gives the text of
 * the last failure on that handle.  A handle is not thread-safe; distinct
 * handles are independent.  All step functions are asynchronous with respect
 * to the host and are safe to capture into a HIP graph (no allocation, no
 * synchronisation inside).
 */
#ifndef HYDRO_H
#define HYDRO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.2.0: scene scalars are doubles (hydro_set_scene), hydro_set_semantics, waves_per_simd in hydro_set_tuning
 * 0.3.0: dt is a double in every step / integrate entry point; the model is evaluated in fp64
 * 0.4.0: hydro_step_wrench_tiled_ke / hydro_step_fused_tiled_ke (kinetic energy sampled inside the step kernel),
 *        hydro_reserve_soa; the engine holds 68 B per body and makes its plain-SoA copies on first use
 * 0.5.0: hydro_step_fused_tiled_multi (any number of closed-loop steps in one pass, the bodies stay in registers)
 * 0.6.0: hydro_step_wrench_tiled_batch (several independent scenes in one launch); the kinetic-energy entries are one
 *        launch (the final sum happens in the block that finishes last); hydro_ke_allreduce (RCCL from C)
 * 0.7.0: hydro_ke_rearm, hydro_bind_rccl / hydro_rccl_origin, hydro_debug_ke_fault; a kinetic-energy launch that does not
 *        finish leaves NaNs, never a stale pair; hydro_step_wrench validates before it allocates
 * 0.7.1: hydro_debug_ke_fault is refused unless HYDRO_ENABLE_TEST_HOOKS=1 at load time; the class finishers of the
 *        kinetic-energy reduction poison the partials they consumed; re-arming happens after the cross-stream wait and
 *        never inside a stream capture
 *        added to 0.7.1 (no existing entry changed): hydro_set_watch, hydro_watch_count, hydro_step_fused_tiled_multi_rec - a
 *        trajectory recorder inside the multi-step kernel (watched bodies' states, every `every`-th step, to a device log)
 *        added to 0.7.1 (no existing entry changed): hydro_step_fused_tiled_multi_app, HYDRO_FRAME_* - an external force and
 *        torque per body, world- or body-fixed, applied inside every step of the multi-step kernel
 *        added to 0.7.1 (no existing entry changed): hydro_step_fused_tiled_multi_ctl, HYDRO_CTL_FIELDS - a per-body pose-hold
 *        feedback law evaluated inside every step of the multi-step kernel
 *        added to 0.7.1 (no existing entry changed): hydro_mooring_wrench, hydro_step_fused_tiled_multi_moor,
 *        HYDRO_MOOR_FIELDS - one tension-only mooring line per body, evaluated inside every step of the multi-step kernel
 *        added to 0.7.1 (no existing entry changed): hydro_extremes_reset, hydro_step_fused_tiled_multi_ext,
 *        HYDRO_EXT_FIELDS - running per-body extremes (position box, speed, line tension) updated inside every step
 *        added to 0.7.1 (no existing entry changed): hydro_tether_wrench, hydro_step_fused_tiled_multi_teth,
 *        HYDRO_TETH_FIELDS - one tension-only line between two bodies of a tile, evaluated inside every step
 *        added to 0.7.1 (no existing entry changed): hydro_step_fused_tiled_multi_net, HYDRO_TETH_LAYERS_MAX - up to four
 *        layers of tether records, so that bodies form chains and cables
 *        added to 0.7.1 (no existing entry changed): hydro_step_fused_tiled_multi_peak - the running maximum of every
 *        tether's tension, per body and layer, updated inside every step
 *        added to 0.7.1 (no existing entry changed): hydro_step_fused_tiled_multi_spread, HYDRO_MOOR_LAYERS_MAX - up to four
 *        layers of mooring records, so that a body rides on a spread of anchored lines
 *        added to 0.7.1 (no existing entry changed): hydro_set_sea_spectrum, hydro_sea_spectrum_sample, hydro_step_fused_tiled_multi_irr,
 *        HYDRO_SPECTRUM_WAVES_MAX - an irregular sea of up to 64 wave components in the closed-loop steps
 *        added to 0.7.1 (no existing entry changed): hydro_statistics_reset, hydro_step_fused_tiled_multi_stat, HYDRO_STAT_* -
 *        running per-body response statistics (sum, sum of squares, up-crossings of a level) updated inside every step
 *        added to 0.7.1 (no existing entry changed): hydro_set_sea_ensemble, hydro_sea_ensemble_sample, hydro_step_fused_tiled_multi_ens,
 *        HYDRO_SEA_ENSEMBLE_MAX - up to 1024 sea spectra in one launch, block m of the bodies stepping through member m
 *        added to 0.7.1 (no existing entry changed): hydro_set_sea_finite_depth, hydro_sea_finite_depth_sample,
 *        hydro_step_fused_tiled_multi_fd - the ensemble's spectra in water of finite depth h: waves that feel the bottom
 *        added to 0.7.1 (no existing entry changed): hydro_set_current_profile, hydro_current_profile_sample,
 *        hydro_step_fused_tiled_multi_shear, HYDRO_CURRENT_KNOTS_MAX - a sheared current: a profile over depth of up to 16 knots */
#define HYDRO_VERSION 0x000701

#define HYDRO_OK         0
#define HYDRO_E_ARG    (-1)   /* bad argument (null pointer, n > capacity, dt <= 0, misaligned ...) */
#define HYDRO_E_ALLOC  (-2)   /* device or host allocation failed */
#define HYDRO_E_LAUNCH (-3)   /* kernel launch / stream operation failed */
#define HYDRO_E_DEVICE (-4)   /* no such device / cannot select it */
#define HYDRO_E_STATE  (-5)   /* call order violated (e.g. step before set_params) */

#define HYDRO_STATE_FIELDS  13
#define HYDRO_PREV_FIELDS    6
#define HYDRO_PARAM_FIELDS  11
#define HYDRO_WRENCH_FIELDS  6
#define HYDRO_CTL_FIELDS    17   /* the control record of hydro_step_fused_tiled_multi_ctl */
#define HYDRO_MOOR_FIELDS    9   /* the mooring record of hydro_step_fused_tiled_multi_moor */
#define HYDRO_EXT_FIELDS     8   /* the extremes record of hydro_step_fused_tiled_multi_ext */
#define HYDRO_TETH_FIELDS    7   /* the tether record of hydro_step_fused_tiled_multi_teth */
#define HYDRO_TETH_LAYERS_MAX 4  /* tether records, one behind the other, in the net of hydro_step_fused_tiled_multi_net */
#define HYDRO_MOOR_LAYERS_MAX 4  /* mooring records, one behind the other, in the spread of hydro_step_fused_tiled_multi_spread */
#define HYDRO_COMP_FIELDS   24
#define HYDRO_TILE          64   /* bodies per tile of the tiled-SoA layout = one wavefront */
#define HYDRO_BATCH_MAX     32   /* scenes per hydro_step_wrench_tiled_batch launch */
#define HYDRO_WATCH_MAX  65536   /* bodies in one watch list (hydro_set_watch) */
#define HYDRO_SEA_WAVES_MAX   8   /* regular wave components of a sea state (hydro_set_sea) */
#define HYDRO_SEA_FIELDS      4   /* the record of hydro_sea_sample: eta, u_x, u_y, u_z */
#define HYDRO_SPECTRUM_WAVES_MAX 64 /* wave components of a sea spectrum (hydro_set_sea_spectrum) */
#define HYDRO_SEA_ENSEMBLE_MAX 1024 /* members of a sea ensemble (hydro_set_sea_ensemble) */
#define HYDRO_CURRENT_KNOTS_MAX 16 /* knots of a current profile (hydro_set_current_profile) */
/* the channels of a statistics record (hydro_step_fused_tiled_multi_stat) */
#define HYDRO_STAT_X        0    /* s[0] */
#define HYDRO_STAT_Y        1    /* s[1] */
#define HYDRO_STAT_Z        2    /* s[2] */
#define HYDRO_STAT_VX       3    /* s[7] */
#define HYDRO_STAT_VY       4    /* s[8] */
#define HYDRO_STAT_VZ       5    /* s[9] */
#define HYDRO_STAT_TENSION  6    /* the tension the extremes record samples */
#define HYDRO_STAT_CHANNELS 7
#define HYDRO_STAT_BYTES_PER_BODY 44   /* four doubles and three words */
#define HYDRO_STAT_TILE_BYTES  2816    /* hydro_statistics_tile_t: 64 bodies */
#define HYDRO_STAT_LEVEL_FIELDS   2    /* the level record: one level per body and channel slot */

typedef struct hydro_engine hydro_t;

/* Library identity. */
int         hydro_version(void);
const char *hydro_status_string(int status);
int         hydro_device_count(int *count);

/* Lifetime.  One engine = one device + up to `capacity` bodies.  Replaces the construction of
 * one WarpHydrodynamicsWrapper per prim (warp_hydrodynamics_wrapper.py:10-77; one instance per
 * body, hydrodynamics_behavior.py:155-169) with one batched object.
 * Device memory: 68 B per body of capacity - the tiled parameter record (44 B) and the tiled previous velocity
 * (24 B) - plus 1/16 B of reduction scratch.  The entry points that take PLAIN field pointers (hydro_step_wrench,
 * hydro_step_wrench_ext, hydro_step_components) work on plain-SoA copies of the parameters / previous velocity
 * (82 B per body more, + 14 B for the fp16 coefficient copy) that are made on their FIRST call - which therefore
 * allocates and synchronises once and cannot be captured into a HIP graph; call it once before capturing, or
 * hydro_reserve_soa() up front - before or after hydro_set_params_*: once the copies exist, hydro_set_params_* keeps
 * them current and the step path neither allocates nor synchronises. */
int         hydro_create(int device, int64_t capacity, hydro_t **out);
int         hydro_reserve_soa(hydro_t *h);
int         hydro_destroy(hydro_t *h);
const char *hydro_last_error(const hydro_t *h);
int64_t     hydro_capacity(const hydro_t *h);

/* Scene scalars: water density and gravity ("globals", hydrodynamics_config.json:2-5;
 * ctor arguments water_density / gravity, numba_hydrodynamics_wrapper.py:9-10).  Doubles, as the
 * reference passes Python floats: 9.81 is not an fp32 number, and the kernels evaluate the model in fp64. */
int hydro_set_scene(hydro_t *h, double water_density, double gravity);

/* Which of the reference's two calculators the results follow where the two differ.  Default
 * HYDRO_SEM_NUMBA: numba_hydrodynamics.py, the documented model and the parity target.
 * HYDRO_SEM_WARP: warp_hydrodynamics.py, the twin hydrodynamics_behavior.py:155 actually instantiates:
 *   - added mass rotates the world accelerations with R where Numba uses R^T
 *     (warp_hydrodynamics.py:216-217 vs numba_hydrodynamics.py:229-230);
 *   - component mode: a dry body reports cob = cop = its position (the mean of its wet keypoints if it has
 *     any), not zeros (warp_hydrodynamics.py:59-61,290 vs numba_hydrodynamics.py:277-279).
 * Everything else is common (same matrix from the quaternion - Warp's quat_rotate differs from it by
 * 2(|q|^2-1), 2.4e-7 for an fp32-rounded unit quaternion; lift with a degenerate axis and the pressure
 * centre at rest, which the Warp source leaves unassigned, follow Numba / the N1 completion).
 * What pins HYDRO_SEM_WARP: the reference's warp_hydrodynamics.py and its wrapper EXECUTED under a stand-in for the Warp
 * runtime (fp64, Warp's zero-initialised locals modelled, quat_rotate bound to the matrix form), whose outputs the tests
 * hold every entry to (tests/test_warp_semantics.py).  Not NVIDIA's runtime, not its fp32 rounding, and not Warp's own
 * quat_rotate: against that the net wrench moves by up to 1.0e-5 on fp32-rounded unit quaternions and at order one on
 * non-unit ones.  The first call that selects the mode says so once on stderr (HYDRO_QUIET=1 in the
 * environment silences it). */
#define HYDRO_SEM_NUMBA 0
#define HYDRO_SEM_WARP  1
int hydro_set_semantics(hydro_t *h, int semantics);

/* Per-body constants: the remaining ten ctor arguments of the reference wrappers
 * (numba_hydrodynamics_wrapper.py:9-32) plus the rigid-body mass used by the clamp
 * (hydrodynamics_behavior.py:172-173,222).  `params[f]` points at n floats; `on_device` says
 * where those arrays live.  _f16 stores the seven coefficients as IEEE half in HBM (config 5:
 * 130 B per body-step instead of 144); dims and mass stay fp32; the arithmetic is fp64 either way.
 * Synchronous on the engine's private stream; the caller orders it after steps of this engine still in flight on
 * OTHER streams (they read the records this call rewrites).
 *
 * PARAMETER RECORD - what a negative, zero, NaN or infinite constant does (tests/parameter_cases.py is this paragraph as a
 * table; tests/test_parameter_contract_gpu.py holds every entry to it).  The constants are COMPUTED AS GIVEN: no kernel
 * validates them.  No address, loop bound or lane index in any kernel depends on one - the record is read by tile, lane and
 * field - so no value can fault.  A body's constants are that body's problem alone: every other body keeps the bits it has
 * with the clean record.  The two exceptions are the kinetic-energy pair, which sums every body as given (one NaN mass makes
 * the sum NaN), and a tether's partner, whose wrench is formed from both states.  Negative constants, -0, tiny ones (1e-20 m,
 * 1e-30 kg) and every finite coefficient give what the reference gives.  Where a non-finite constant makes the kernels leave
 * the reference (hydrodynamics_behavior.py:212-226, numba_hydrodynamics.py:54-105), row by row:
 *   - mass = NaN: the UNCLAMPED wrench.  The clamp factor is fminf(1, m 500 / (|F| + 1e-6)) and fminf(1, NaN) = 1; the
 *     reference multiplies by the NaN factor: NaN in all six.
 *   - am_lin = NaN: NaN force, but the torque stays finite and unclamped - for the same reason (|F| = NaN, factor 1), and
 *     because the torque does not pass through the force; the reference: NaN in all six.
 *   - cd_lin, damp_lin or lift = +-Inf: a wrench of EXACTLY ZERO (and no implicit drag).  |F| = Inf makes the factor 0, and the
 *     factor is applied with a multiply in which 0 wins whatever the other operand is (v_mul_legacy_f32, the instruction that
 *     zeroes a dry body); the reference: 0 x Inf = NaN in all six.
 *   - am_lin = +-Inf: R (k R^T a) mixes infinities of both signs.  With a NaN among the force components the factor is 1 and
 *     the torque stays finite; without one |F| = Inf and the wrench is exactly zero.  The reference: NaN in all six.
 *   - a NaN dimension: the submersion ratio is fmin(1, .) of the vertical extent and fmin(1, NaN) = 1 - the box is wet
 *     WHEREVER it is, and its wrench is NaN in all six.  The reference decides on the keypoints that do not involve the
 *     dimension: the same NaNs for a wet body, zeros for a dry one.  An infinite dimension: ratio 1 as well; every component
 *     is +-Inf or NaN by the body's attitude - or, where |F| = Inf without a NaN, the whole wrench is zero.  Component mode
 *     reports ratio 1 and buoyancy (0, 0, NaN or +Inf).
 *   - a dry body (finite dimensions) never reads a coefficient or the mass: zeros, as in the reference.
 *   - cd_ang, damp_ang, am_ang non-finite: the force is untouched, the torque NaN or +-Inf - as in the reference.
 *   - an infinite mass: the wrench is the reference's (factor 1), but the integrator forms 1 / m and 1 / I as a hardware seed and
 *     one Newton step, 0 + 0 (1 - Inf x 0) = NaN: the step leaves NaN in all thirteen fields.
 * hydro_set_params_f16 stores NaN and +-Inf as such, rounds to nearest even (ties, subnormals and underflow to +-0 as IEEE half)
 * and REFUSES what would turn a finite coefficient into an infinity: HYDRO_E_ARG if any |coefficient| is finite and >= 65520
 * (the half format ends at 65504; a linear damping of 1e5 N s/m would otherwise become +Inf and its body's wrench exactly
 * zero).  hydro_last_error names the field and the first such body; NOTHING is written - the previous record, f32 or f16,
 * stays in force - and such a record belongs in hydro_set_params_f32. */
int hydro_set_params_f32(hydro_t *h, int64_t n, const float *const params[HYDRO_PARAM_FIELDS], int on_device);
int hydro_set_params_f16(hydro_t *h, int64_t n, const float *const params[HYDRO_PARAM_FIELDS], int on_device);

/* Previous-step velocity (the only state carried between steps: _last_linear_velocity /
 * _last_angular_velocity, hydrodynamics_behavior.py:196-198,237-238; reset on stop :240-245).
 * get/set exist for checkpoint / resume. */
int hydro_reset_prev_velocity(hydro_t *h);
int hydro_get_prev_velocity(hydro_t *h, int64_t n, float *const prev[HYDRO_PREV_FIELDS], int on_device);
int hydro_set_prev_velocity(hydro_t *h, int64_t n, const float *const prev[HYDRO_PREV_FIELDS], int on_device);

/* The fused hot path: finite-difference acceleration (hydrodynamics_behavior.py:200-202),
 * the nine-component model (numba_hydrodynamics.py:256-314), lever-arm torques and sum
 * (:212-218), safety clamp (:220-226) - one launch for all n bodies.
 *
 * hydro_step_wrench      previous velocity lives in the engine; the kernel reads it and stores
 *                        this step's velocity in its place (24 B more traffic per body).
 * hydro_step_wrench_ext  previous velocity is the caller's (e.g. last step's velocity arrays
 *                        of a ping-pong integrator): pure 144 B (fp32) / 130 B (fp16
 *                        coefficients) per body-step, nothing written but the wrench.
 * `dt` is a double: the reference's callback receives `delta_time` as a Python float
 * (hydrodynamics_behavior.py:138).  Inputs and outputs are fp32 arrays; the arithmetic in between is fp64 - the type
 * of the reference's Numba path, the parity target - each result rounded to fp32 once, which is why neither the scene
 * scalars nor 1/dt may be rounded on the way in: the finite difference is evaluated as the
 * Numba / fp64 oracle evaluates it.  (The reference BEHAVIOUR as shipped divides fp32 torch tensors by dt and feeds
 * its fp32 Warp calculator, :200-209; that pipeline is the unpinned HYDRO_SEM_WARP twin, not the target.)
 * `stream` is a hipStream_t; NULL is HIP's default (null) stream, as in any HIP API.  The
 * engine's private stream (used for its own copies) is available from hydro_stream(). */
int hydro_step_wrench(hydro_t *h, int64_t n, const float *const state[HYDRO_STATE_FIELDS], double dt,
                      float *const wrench[HYDRO_WRENCH_FIELDS], void *stream);
int hydro_step_wrench_ext(hydro_t *h, int64_t n, const float *const state[HYDRO_STATE_FIELDS],
                          const float *const prev[HYDRO_PREV_FIELDS], double dt,
                          float *const wrench[HYDRO_WRENCH_FIELDS], void *stream);

/* The same fused step on the engine's NATIVE layout, tiled struct-of-arrays: a group of F fields
 * over n bodies is stored as [ceil(n/64)][F][64] floats, i.e. body i, field f lives at
 *     base[(i / 64) * tile_stride + f * 64 + (i % 64)]        (tile_stride >= F * 64, in floats).
 * Coalescing is that of plain SoA; the difference is that the ~28 256-byte runs a wavefront needs
 * form three contiguous records instead of 28 pieces of 28 arrays (measured +13 % HBM rate at 4M
 * bodies).  Buffers hold whole tiles (pad the last one) and are 16-byte aligned.
 *   prev == NULL : previous velocity lives in the engine (read, then overwritten).
 *   prev != NULL : caller-owned; for a ping-pong integrator pass the previous state buffer
 *                  + 7 * 64 with its tile stride (the six velocity fields of each state tile). */
int hydro_step_wrench_tiled(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                            const float *prev, int64_t prev_tile_stride, double dt,
                            float *wrench, int64_t wrench_tile_stride, void *stream);

/* The same step for `count` INDEPENDENT scenes in one launch (1 <= count <= HYDRO_BATCH_MAX).  Every scene is what one
 * hydro_step_wrench_tiled call takes - an engine (its parameters, scene scalars and, with prev == NULL, its previous
 * velocity), n bodies, tiled state / prev / wrench buffers - and gets exactly the bits that call would give; what the
 * batch buys is ONE ramp and drain for all of them: k replicas of a 1 M-body scene stream at the rate of a k M-body
 * launch without the caller owning streams.  Replaces the per-prim loop of the reference at the
 * scale of config 3's 1 024 environments (one HydrodynamicsBehavior callback per prim per step,
 * hydrodynamics_behavior.py:131-138,176-238) when the environments live in separate buffers.
 * One kernel instance serves the launch, so all scenes share: the device, the coefficient format (f32 / f16), the
 * semantics, the previous-velocity mode (all prev == NULL or none), and dt.  Scene scalars (rho, g) may differ.  An
 * engine that owns the previous velocity may appear once per launch.  Errors are reported on scenes[0].engine; the
 * hydro_set_tuning knobs that apply (non_temporal) are those of scenes[0].engine, by the size of the whole launch.
 * Everything is validated for every scene before anything is launched; a failure of the launch itself may leave the
 * engine-owned previous velocities of some scenes marked as "tiled copy current", which is always truthful. */
typedef struct hydro_scene {
    hydro_t *engine;
    int64_t n;
    const float *state;  int64_t state_tile_stride;
    const float *prev;   int64_t prev_tile_stride;     /* NULL: engine-owned previous velocity */
    float *wrench;       int64_t wrench_tile_stride;
} hydro_scene_t;
int hydro_step_wrench_tiled_batch(int count, const hydro_scene_t *scenes, double dt, void *stream);

/* The same step, sampling the kinetic energy on the way ("reduced in-kernel"): the kernel adds
 * 1/2 m |v|^2 (and, with `rotational`, the box-inertia term) of the bodies it already holds in registers - the state
 * it READS, i.e. the state the previous step left - reduces over the block (LDS) and the wavefront, and the block
 * that finishes last adds the per-block pairs in a fixed order into ke_out_dev[0..1] (device memory, fp64; same launch).
 * No second pass over the state, no second launch, the wrench bits are those of hydro_step_wrench_tiled, the energy bits those of
 * hydro_kinetic_energy_tiled on the same state.  For the monitor that all-reduces the pair over RCCL every K steps. */
int hydro_step_wrench_tiled_ke(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                               const float *prev, int64_t prev_tile_stride, double dt,
                               float *wrench, int64_t wrench_tile_stride,
                               int rotational, double *ke_out_dev, void *stream);

/* Edges of the tiled layout: simulator tensors -> tiled state and tiled
 * wrench -> forces / torques (both staged through LDS), and a generic plain-SoA <-> tiled
 * repack of `fields` field pointers. */
int hydro_pack_state_aos(hydro_t *h, int64_t n, const float *positions, const float *orientations, int quat_xyzw,
                         const float *velocities, float *state, int64_t state_tile_stride, void *stream);
int hydro_unpack_wrench_aos(hydro_t *h, int64_t n, const float *wrench, int64_t wrench_tile_stride,
                            float *forces, float *torques, void *stream);
int hydro_repack(hydro_t *h, int64_t n, int fields, float *const soa[], float *tiled, int64_t tile_stride,
                 int to_tiled, void *stream);

/* Same step on the array-of-structs tensors the simulator hands over
 * (RigidPrimView.get_world_poses / get_velocities, hydrodynamics_behavior.py:178-189) and takes
 * back (apply_forces_and_torques_at_pos, :229-234): positions (n,3), orientations (n,4) in the
 * simulator's WXYZ order when quat_xyzw == 0 (the reorder of :194 is done in the load) or in the
 * calculators' XYZW order when quat_xyzw != 0, velocities (n,6) [lin|ang]; forces (n,3),
 * torques (n,3).  All five tensors 16-byte aligned.  Every lane moves its body's rows with 12- / 16- / 24-byte
 * accesses (a wave-instruction covers a contiguous run of whole lines; staging the transposition through LDS was
 * measured and is slower).  Previous velocity lives in the engine, as for hydro_step_wrench. */
int hydro_step_wrench_aos(hydro_t *h, int64_t n, const float *positions, const float *orientations, int quat_xyzw,
                          const float *velocities, double dt, float *forces, float *torques, void *stream);

/* Component mode = WarpHydrodynamicsWrapper.calculate_hydrodynamic_forces
 * (warp_hydrodynamics_wrapper.py:79-132) / NumbaHydrodynamicsWrapper.calculate_hydrodynamic_forces
 * (numba_hydrodynamics_wrapper.py:34-53): explicit accelerations in, the eight 3-vectors of
 * the reference's return tuple out (+ submersion ratio, its ninth value; `ratio` may be NULL).
 * Dry bodies give zeros for all eight (Numba semantics, numba_hydrodynamics.py:277-279). */
int hydro_step_components(hydro_t *h, int64_t n, const float *const state[HYDRO_STATE_FIELDS],
                          const float *const accel[HYDRO_PREV_FIELDS], float *const comps[HYDRO_COMP_FIELDS],
                          float *ratio, void *stream);

/* The same on the calculators' own argument layout - calculate_hydrodynamic_forces(position,
 * orientation_quat [x,y,z,w], linear_vel, angular_vel, linear_accel, angular_accel): (n,3) tensors
 * ((n,4) for the quaternion; no alignment requirement) in, eight (n,3) tensors out in the order of the
 * reference's return tuple.  One launch per call; the reference's Warp wrapper needs six assign
 * copies plus a graph launch (warp_hydrodynamics_wrapper.py:85-120). */
int hydro_step_components_aos(hydro_t *h, int64_t n, const float *position, const float *orientation_xyzw,
                              const float *linear_vel, const float *angular_vel, const float *linear_accel,
                              const float *angular_accel, float *const out[8], float *ratio, void *stream);

/* Kinetic energy of the n bodies: out_dev[0] = sum 1/2 m |v|^2, out_dev[1] = sum 1/2 w^T I w (box
 * inertia; 0 unless `rotational`), every body in fp64.  Deterministic reduction on device in ONE launch: the four
 * bodies a lane owns in a group of 256 -> wave64 shuffle tree -> one fp64 pair per group -> the block that draws the
 * last ticket (one integer atomic per block; no floating-point atomics) adds the pairs in a fixed order.  The result
 * does not depend on the order in which blocks run; it stays on the device so that the caller can all-reduce it over
 * RCCL.  New functionality named by BASELINE.json north_star; absent from the reference.
 * These are the stand-alone entries (one pass over the state: 56 B per body with the rotational term);
 * hydro_step_wrench_tiled_ke / hydro_step_fused_tiled_ke sample the same pair, same bits, inside a step.
 * All of them use the engine's reduction scratch (partials + integer ticket counters that a launch leaves at zero).
 * Two of them on one engine must not be in flight at once: a launch on a stream other than the previous one's is
 * ordered behind it by the library (an event wait on the device; not while either stream is being captured - keep a
 * captured graph's kinetic-energy launches on one stream).
 * A launch that does not finish cannot pass for a result: block 0 of every launch first overwrites out_dev[0..1] with
 * NaNs, and only the wavefront that completes the sum replaces them - a launch that did not run to its end (device reset,
 * aborted graph) leaves NaNs.  After such an event the counters may be non-zero: hydro_ke_rearm zeroes them (the library
 * does so by itself, outside stream captures, before the next kinetic-energy launch whenever a HIP call on this handle has
 * reported an error).  Until then later launches give NaNs too: either nobody draws the last ticket, or a class is added
 * before all of its members have published and meets the NaNs every class finisher leaves in the partials it consumed.
 * Not covered (call hydro_ke_rearm if a launch may have died unseen): partials the unfinished launch itself had
 * published - finite, and stale if the scene changed - read by such an early class sum. */
int hydro_kinetic_energy(hydro_t *h, int64_t n, const float *const state[HYDRO_STATE_FIELDS], int rotational,
                         double *out_dev, void *stream);
int hydro_kinetic_energy_tiled(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int rotational,
                               double *out_dev, void *stream);

/* The one collective of the path: sum the pair a kinetic-energy entry left in ke_dev[0..1] over the ranks
 * of `nccl_comm` (an ncclComm_t of RCCL; one rank per GPU), in place, on `stream` -
 * ncclAllReduce(ke_dev, ke_dev, 2, ncclDouble, ncclSum, comm, stream).  16 bytes over xGMI: latency-bound; put it on a
 * side stream every K steps.  RCCL is bound at the first call (the copy already loaded in the process, else librccl.so;
 * HYDRO_RCCL_LIBRARY overrides), so a single-GPU host needs no RCCL; HYDRO_E_STATE if there is none.  New functionality
 * named by BASELINE.json north_star; the reference has no reduction of any kind. */
int hydro_ke_allreduce(hydro_t *h, void *nccl_comm, double *ke_dev, void *stream);

/* Which RCCL hydro_ke_allreduce calls.  A communicator belongs to ONE loaded copy of the library (a Python host's torch
 * ships its own), so the safe binding is the caller's: hydro_bind_rccl((void *)ncclAllReduce, (void *)ncclGetErrorString)
 * hands over the functions of the copy that made the communicator (the second may be NULL).  Without it the first
 * hydro_ke_allreduce looks one up: HYDRO_RCCL_LIBRARY if set (that or nothing), else the copy already loaded in the
 * process, else the system librccl; only success is remembered, a failed look-up is repeated by the next call.
 * hydro_bind_rccl(NULL, NULL) forgets the binding.  Process-wide, thread-safe.  hydro_rccl_origin() says where the
 * current binding came from ("unbound", "hydro_bind_rccl", "HYDRO_RCCL_LIBRARY", ...). */
int hydro_bind_rccl(void *nccl_all_reduce, void *nccl_get_error_string);
const char *hydro_rccl_origin(void);

/* Zero the ticket counters of the kinetic-energy reduction on `stream` (see hydro_kinetic_energy): the recovery path
 * after a launch that did not finish.  Harmless at any other time, provided no kinetic-energy launch of this engine is
 * in flight on another stream. */
int hydro_ke_rearm(hydro_t *h, void *stream);

/* TEST HOOK, refused with HYDRO_E_STATE unless HYDRO_ENABLE_TEST_HOOKS=1 was in the environment when the library was
 * loaded (one build, no second code path; a host that merely binds the library cannot reach a live engine through it):
 * after a device synchronisation, write `value` into ticket counter `counter` (0 = the top counter, 1 + c = class c) - the
 * state an aborted launch leaves behind - and, if as_failed_launch, mark the handle the way a failed HIP call does, so
 * that the next kinetic-energy launch re-arms by itself (tests/test_error_paths_gpu.py). */
int hydro_debug_ke_fault(hydro_t *h, int counter, uint32_t value, int as_failed_launch);

/* Explicit rigid-body step standing in for PhysX in closed-loop runs:
 * semi-implicit Euler with gravity and box inertia.  state_out may alias state_in. */
int hydro_integrate(hydro_t *h, int64_t n, const float *const state_in[HYDRO_STATE_FIELDS],
                    const float *const wrench[HYDRO_WRENCH_FIELDS], double dt,
                    float *const state_out[HYDRO_STATE_FIELDS], void *stream);

int hydro_integrate_tiled(hydro_t *h, int64_t n, const float *state_in, int64_t in_tile_stride,
                          const float *wrench, int64_t wrench_tile_stride, double dt,
                          float *state_out, int64_t out_tile_stride, void *stream);

/* Wrench + integrator fused into one pass over tiled buffers (closed-loop runs): the state is read
 * once and the wrench does not go through memory unless `wrench` is non-NULL.  `prev` is normally the
 * previous state buffer + 7 * 64 (tile stride 13 * 64); `state_out` may alias that previous-state
 * buffer (ping-pong) but not `state`.  implicit_drag == 0: same arithmetic, same bits as
 * hydro_step_wrench_tiled followed by hydro_integrate_tiled (explicit in every force).
 * implicit_drag != 0: the drag part of the wrench (k_lin v, k_ang w) is taken at the new velocity,
 * which is unconditionally stable where the explicit form needs |k| dt / m < 2 (light bodies with
 * strong damping, e.g. the SILVER2 links at 120 Hz). */
int hydro_step_fused_tiled(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                           const float *prev, int64_t prev_tile_stride, double dt,
                           float *state_out, int64_t out_tile_stride,
                           float *wrench, int64_t wrench_tile_stride, int implicit_drag, void *stream);

/* The same, sampling the kinetic energy of the state it WRITES (the state after this step) into
 * ke_out_dev[0..1]; see hydro_step_wrench_tiled_ke.  State bits are those of hydro_step_fused_tiled. */
int hydro_step_fused_tiled_ke(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                              const float *prev, int64_t prev_tile_stride, double dt,
                              float *state_out, int64_t out_tile_stride,
                              float *wrench, int64_t wrench_tile_stride, int implicit_drag,
                              int rotational, double *ke_out_dev, void *stream);

/* `steps` closed-loop steps in ONE pass over the tiled buffers.  No term of the model couples two bodies, so every body is
 * carried through all the steps in registers: state, previous velocity and parameters are read once; `state_out` receives
 * the state after the last step and `prev_out` (6 fields, tiled) the velocity of the step before it, i.e. what the next
 * call needs as `prev`.  Same arithmetic in the same order, hence the same bits, as `steps` calls of
 * hydro_step_fused_tiled - with (120 + 76) / steps bytes of traffic per body-step instead of 172 and one launch
 * instead of `steps` (intermediate states never exist in memory: sample, log or couple at multiples of `steps` - or
 * record the bodies you want to see from inside the launch, hydro_step_fused_tiled_multi_rec below).
 * Aliasing: `state_out` may alias the buffer `prev` points into, `prev_out` may alias `state` + 7 * 64 (the velocity
 * fields of the state being read) - with both, the two-buffer ping-pong of the single-step entry carries over unchanged;
 * `state_out` must not alias `state`.  ke_out_dev != NULL: also sample the kinetic energy of the final state (two doubles
 * on the device, see hydro_step_wrench_tiled_ke).  1 <= steps <= 2^20.
 * New functionality (the reference steps PhysX once per callback); SURVEY.md 8f row 2. */
int hydro_step_fused_tiled_multi(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                 const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                 float *state_out, int64_t out_tile_stride,
                                 float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                 int rotational, double *ke_out_dev, void *stream);

/* Trajectory recorder: the states BETWEEN the first and the last step of a multi-step launch exist in registers only, so
 * a short list of WATCHED bodies is written to a device log from inside the kernel, every `every`-th step - the device-side
 * counterpart of the reference's one validation artefact, the per-frame pose / velocity rows of log_velocity.py:29-57.
 *
 * hydro_set_watch: `bodies_host` (HOST memory) holds `count` strictly ascending body indices in [0, capacity),
 * 1 <= count <= HYDRO_WATCH_MAX; body bodies_host[j] records into COLUMN j of the log.  Builds the engine's watch tables
 * (12 B per tile of the capacity, allocated by the first call, freed by hydro_destroy) on the engine's private stream and
 * waits for them, like hydro_set_params_*: the caller orders it after recording launches of this engine still in flight on
 * other streams.  count == 0 or bodies_host == NULL clears the list.  HYDRO_E_ARG for a count above the maximum, an index
 * out of range, an unsorted list or a duplicate - the previous list stays in force.  hydro_watch_count: bodies on the
 * list, 0 without one.
 *
 * hydro_step_fused_tiled_multi_rec: hydro_step_fused_tiled_multi - same arguments, same aliasing rules, the same state,
 * prev_out and kinetic-energy bits - that also records.  With k = 1 .. steps the steps of this launch, a sample is taken
 * AFTER step k when k >= phase and (k - phase) % every == 0, into row row0 + (k - phase) / every:
 *     log[(row * fields + f) * log_stride + j]      j = column of the watched body, log_stride >= hydro_watch_count
 * i.e. a (rows_capacity, fields, log_stride) float array in device memory.  fields = 13: f is the field of `state` after
 * that step; fields = 19: followed by the six fields of the `wrench` that produced it (the wrench of the state BEFORE the
 * step).  Rows are bit for bit what hydro_step_fused_tiled leaves in memory at that step.  The caller derives phase
 * (1 .. every) and row0 from its own step count, so launches need not be multiples of `every`; phase > steps is legal and
 * records nothing.  *rows_written_host (may be NULL) receives the number of rows this launch writes.  Elements of the log
 * that belong to no (row, field, column) written are not touched.
 * Cost: two scalar loads per wavefront and launch, one scalar compare per step; 13 or 19 dword stores per watched body and
 * sample.  Bodies that are not watched move no extra byte.
 * HYDRO_E_STATE without a watch list.  HYDRO_E_ARG for every < 1 (or > 2^30), phase outside 1 .. every, fields other than
 * 13 / 19, log_stride < the watch count, a watched body >= n, a row at or beyond rows_capacity (< 2^31), besides what
 * hydro_step_fused_tiled_multi refuses - all before anything is launched or written.  Asynchronous, no allocation, no
 * synchronisation, safe to capture (a captured launch replays with the row0 it was captured with).
 * New functionality: the reference logs through one host round trip per row. */
int     hydro_set_watch(hydro_t *h, int64_t count, const int64_t *bodies_host);
int64_t hydro_watch_count(const hydro_t *h);
int hydro_step_fused_tiled_multi_rec(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host, void *stream);

/* Applied wrench: an external force and torque per body inside the closed-loop steps - a thruster, a tether, a towing force,
 * an RL action; what PhysX adds next to the plugin's wrench in the reference (robot.py / cmd_vel), for the loop in which this
 * library is the integrator.  Between the first and the last step of a multi-step launch the states exist in registers only,
 * so a body-fixed thrust can be turned with the body nowhere but inside the kernel.
 *
 * hydro_step_fused_tiled_multi_app: hydro_step_fused_tiled_multi_rec - same arguments up to rows_written_host, same aliasing
 * rules - with `applied`, a tiled 6-field record ([tiles][6][64] floats, tile stride applied_tile_stride >= 384, 16-byte
 * aligned, whole tiles) of a = [Fx Fy Fz | Tx Ty Tz] per body: the force acts AT the body origin, the torque is ABOUT the
 * body origin (a force at an offset point r: pass r x f as torque).  In every step, between the wrench and the integrator:
 *     HYDRO_FRAME_WORLD  wrench[i] += a[i]                                      one fp32 add per component, nothing else
 *     HYDRO_FRAME_BODY   wrench[0:3] += R a[0:3], wrench[3:6] += R a[3:6]       R: the fp32 rotation matrix of the quaternion
 *                        of the state the step STARTS from, used as given (a non-unit quaternion is not normalised), in the
 *                        form the integrator builds it; evaluated anew in every step of the launch
 * Zero-order hold: `a` is read once per launch and held constant IN ITS FRAME for all `steps` steps (a world-fixed pull stays
 * world-fixed, a body-fixed thrust turns with the body).  The safety clamp acts on the hydrodynamic wrench alone; the applied
 * wrench is added after it, unclamped.  With implicit_drag the sum stands where the wrench stood in the implicit form.  The
 * wrench the recorder logs (fields = 19) is the TOTAL that was integrated - the wrench that produced the state.
 * steps = 1 is the single-step form (there is no separate entry).
 *   log == NULL     : no recording; no watch list is needed, the other recorder arguments are ignored, *rows_written_host = 0.
 *   log != NULL     : exactly the rules of hydro_step_fused_tiled_multi_rec.
 *   applied == NULL : legal; the launch and its bits are those of hydro_step_fused_tiled_multi (log == NULL) or
 *                     hydro_step_fused_tiled_multi_rec (log != NULL); applied_tile_stride and applied_frame are ignored.
 * A zero `applied` gives the values of the unapplied step (x + 0 == x; only the sign of a zero may differ).
 * HYDRO_E_ARG for a misaligned `applied`, a stride below 384 (or not a multiple of 4, or >= 2^24), a frame other than 0 / 1,
 * and an `applied` whose address range [applied, applied + tiles * stride) overlaps that of state_out, prev_out or the log -
 * besides what the neighbours refuse; all before anything is launched or written.  `applied` may be rewritten between
 * launches on the same stream (a captured launch replays with the contents of the moment).  Asynchronous, no allocation,
 * no synchronisation, safe to capture.
 * New functionality; the reference leaves actuator forces to PhysX. */
#define HYDRO_FRAME_WORLD 0
#define HYDRO_FRAME_BODY  1
int hydro_step_fused_tiled_multi_app(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame, void *stream);

/* Pose hold: a feedback law per body INSIDE the closed-loop steps - station keeping, a depth or heading hold.  The applied
 * wrench above is a zero-order hold over a launch; a law that is to act at the rate of the physics while the states stay in
 * registers has to be evaluated in the loop.  This one pulls each body towards a target pose with a clamped PD law.
 *
 * hydro_step_fused_tiled_multi_ctl: hydro_step_fused_tiled_multi_app - same arguments up to applied_frame, same rules - with
 * `control`, a tiled record of HYDRO_CTL_FIELDS = 17 floats per body ([tiles][17][64] floats, tile stride
 * control_tile_stride >= 1088, 16-byte aligned, whole tiles), in field order
 *     p*(3) | q*(4, xyzw) | kp_lin(3) | kd_lin(3) | kp_ang | kd_ang | f_max | t_max
 * target position and attitude in the world, gains in absolute units (N/m, N s/m per world axis; N m/rad, N m s/rad),
 * largest force and torque (+inf: unlimited; >= 0).  In EVERY step, from the state s = [p | q | v | omega] the step starts
 * from, in fp32, in exactly this order (fma(a, b, c): a * b + c rounded once; rsqrt: hardware seed + one Newton step):
 *     e_i = p*_i - p_i                         F_i = fma(kp_lin_i, e_i, -(kd_lin_i * v_i))                     i = x, y, z
 *     n2  = fma(F_z, F_z, fma(F_y, F_y, F_x * F_x));       if (n2 > f_max * f_max)  F_i = F_i * (f_max * rsqrt(n2))
 *     q_e = q* (x) conj(q), both as given (not normalised), with t = q*:
 *           w = fma(tw, qw, fma(tx, qx, fma(ty, qy, tz * qz)))
 *           x = fma(qw, tx, fma(-tw, qx, fma(qy, tz, -(qz * ty))))      y, z: the cyclic successors of x
 *     h   = w < 0 ? -2 : 2                     T_i = fma(kp_ang, h * q_e_i, -(kd_ang * omega_i))
 *     n2 of T; if (n2 > t_max * t_max)  T_i = T_i * (t_max * rsqrt(n2))
 *     wrench[0:3] += F   (world, at the body origin)        wrench[3:6] += T   (world, about the body origin)
 * i.e. 2 q_e.xyz is the rotation vector from the attitude to the target to first order, on the short way round (the flip at
 * w = 0 is the law's one discontinuity); the clamps act on the norm and are continuous.  F and T are added after the safety
 * clamp of the hydrodynamic wrench and after the applied wrench; with implicit_drag the sum stands where the wrench stood;
 * the recorder logs the total.  |F|, |T| are expected below 2^63 (their squares are formed); f_max, t_max above that do not clamp.
 *   control == NULL : legal; the launch and its bits are those of hydro_step_fused_tiled_multi_app with the same arguments;
 *                     control_tile_stride is ignored.
 *   applied == NULL : legal with or without control (applied_tile_stride and applied_frame are ignored).
 * All-zero gains give the values of the uncontrolled step (x + 0 == x; only the sign of a zero may differ).  steps = 1 is the
 * single-step form.  HYDRO_E_ARG for a misaligned `control`, a stride below 1088 (or not a multiple of 4, or >= 2^24) and a
 * `control` whose range [control, control + tiles * stride) overlaps that of state_out, prev_out or the log - besides what
 * hydro_step_fused_tiled_multi_app refuses; all before anything is launched or written.  `control` may be rewritten between
 * launches on the same stream (a captured launch replays with the contents of the moment): a planner moves set-points
 * between launches.  Asynchronous, no allocation, no synchronisation, safe to capture.
 * New functionality; the reference leaves control to the simulator's articulation controllers. */
int hydro_step_fused_tiled_multi_ctl(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride, void *stream);

/* Sea state: moving water for the closed-loop steps - a steady uniform current and regular deep-water waves, scene-wide like
 * the density and gravity of hydro_set_scene.  The hydrodynamic wrench is translation-invariant in x and y and sees the water
 * only through the depth of the body centre and the body's velocity, so moving water is the SAME wrench evaluated on a
 * relative state: depth below the local surface, velocity against the local water.  The integrator, the applied wrench, the
 * pose hold, the recorder and the kinetic energy keep acting on the true state.  Only hydro_step_fused_tiled_multi_sea (and
 * the entries built on it), hydro_sea_sample and the two open-loop entries hydro_step_wrench_tiled_sea and
 * hydro_step_wrench_aos_sea ("Sea state, open loop" below; the plugin steps through the latter) know the sea: every other
 * wrench-only, array-of-structs, batch and component entry, and the other closed-loop entries, step through still water with
 * its surface at z = 0 whatever is set here.
 *
 * hydro_sea_t: `current` U (m/s, world frame) and `waves` = 0 .. HYDRO_SEA_WAVES_MAX components, each an amplitude a >= 0 (m),
 * a wave vector (kx, ky) (rad/m, world frame, kappa = |k| > 0 unless a == 0), an angular frequency omega (rad/s) and a phase
 * phi (rad):  eta(x, y, t) = sum_j a_j cos(kx_j x + ky_j y - omega_j t + phi_j).  omega and k are taken as given: the
 * dispersion relation (deep water: omega^2 = g kappa) is the caller's business.
 *
 * WATER AT A BODY.  At the start of local step k = 0 .. steps - 1 of a launch that begins at step index step0, for a body with
 * state s = [p | q | v | omega_b], in exactly this order (fma(a, b, c): a * b + c rounded once):
 *     t     = (step0 + k) * dt                               fp64, one rounding: (step0 + k) is an exact integer
 *     x_j   = fma(-omega_j, t, phi_j)                        fp64
 *     m_j   = rint(x_j * (1 / 2 pi))                         fp64, ties to even
 *     tau_j = fma(-m_j, 2.4492935982947064e-16, fma(-m_j, 6.283185307179586, x_j))      fp64: x_j reduced to [-pi, pi];
 *                                                            then rounded to fp32 (the same for every body)
 *     th_j  = fma(kx_j, p_x, fma(ky_j, p_y, tau_j))          fp32 from here on
 *     r_j   = th_j * 0.15915494 - rint(th_j * 0.15915494)    revolutions, in [-1/2, 1/2]; the subtraction is exact
 *     c_j   = cos(2 pi r_j), s_j = sin(2 pi r_j)             the hardware's v_cos_f32 / v_sin_f32 of r_j
 *     eta   = fma(a_j, c_j, eta)   j = 0, 1, ...             starting from +0
 *     z_rel = p_z - eta
 *     e_j   = exp2(kl2_j * min(z_rel, 0))                    v_exp_f32; kl2_j = kappa_j log2(e): no growth above the surface
 *     u_x   = fma(cx_j, e_j * c_j, u_x),  u_y = fma(cy_j, e_j * c_j, u_y),  u_z = fma(aw_j, e_j * s_j, u_z)
 *                                                            j = 0, 1, ...  starting from U
 * with the constants kl2_j = kappa_j log2(e), cx_j = a_j omega_j kx_j / kappa_j, cy_j = a_j omega_j ky_j / kappa_j,
 * aw_j = a_j omega_j, and a_j, kx_j, ky_j, U formed in fp64 on the host and rounded ONCE to fp32 (omega_j, phi_j stay fp64).
 * RELATIVE STATE.  The step's hydrodynamic wrench is that of s with s[2] = z_rel and s[7:10] = v - u, and of the previous
 * velocity pv with pv[0:3] - u (fp32 subtractions, the same u: the finite-difference acceleration stays the body's own).
 * Everything behind the wrench takes the true s: the applied wrench, the pose hold, the integrator (the implicit-drag form
 * needs no change: -k (v - u) removed at the old velocity and k (v' - u) added at the new one sum to -k v + k v'), the
 * recorder, the kinetic energy, prev_out.  With implicit_drag == 0 and neither applied nor control a step is therefore, bit
 * for bit, hydro_step_wrench_tiled of the relative state followed by hydro_integrate_tiled of the true one.
 * NOT MODELLED: the slope of the surface; the variation of eta and u across the body (long-wave approximation: the body is
 * small against the wavelength); dynamic pressure (Froude-Krylov force); the water's own acceleration in the added-mass term;
 * finite depth; a vertical current U_z is accepted but is not volume-conserving.
 *
 * hydro_set_sea: copies the sea into an engine-owned device table (400 B, allocated by the first call, freed by
 * hydro_destroy) on the engine's private stream and waits, like hydro_set_watch: the caller orders it after launches of this
 * engine still in flight on other streams.  sea == NULL clears the sea.  HYDRO_E_ARG for more than HYDRO_SEA_WAVES_MAX (or
 * fewer than 0) components, a non-finite value, a negative amplitude, kappa == 0 with a != 0, a constant beyond fp32 range -
 * the previous sea stays in force.  A captured launch reads the table at replay time, with the number of components of the
 * moment it was captured.
 *
 * hydro_sea_sample: writes the tiled HYDRO_SEA_FIELDS = 4 field record [eta, u_x, u_y, u_z] ([tiles][4][64] floats, tile
 * stride out_tile_stride >= 256) of bodies 0 .. n - 1 - exactly the values a step that starts from `state` at step index
 * `step_index` uses.  A small kernel of its own; asynchronous on `stream`.  HYDRO_E_STATE without a sea; HYDRO_E_ARG for
 * dt <= 0, step_index outside 0 .. 2^52 - 1, n > capacity, a null or misaligned buffer.
 *
 * hydro_step_fused_tiled_multi_sea: hydro_step_fused_tiled_multi_ctl - same arguments up to control_tile_stride, same rules -
 * through the sea, with `step0` the index of the launch's first step (the caller's running step count).
 *   no sea set      : the launch and its bits are those of hydro_step_fused_tiled_multi_ctl with the same arguments.
 *   a sea set       : log, applied and control are each still optional; what is added between the wrench and the integrator is
 *                     what hydro_step_fused_tiled_multi_ctl adds for the same three pointers.
 * A sea with no current and no waves (or waves of amplitude 0) gives the bits of the entry without a sea: x - (+0) == x, sign
 * of zero included.  HYDRO_E_ARG for step0 < 0 or step0 + steps >= 2^52, besides what hydro_step_fused_tiled_multi_ctl
 * refuses - all before anything is launched or written.  Asynchronous, no allocation, no synchronisation, safe to capture: a
 * captured launch replays with the step0 it was captured with, i.e. at a frozen wave phase - capture current-only seas.
 * Cost and registers: DESIGN.md section 17.  New functionality; the reference's water does not move. */
typedef struct hydro_sea_wave {
    double amplitude, kx, ky, omega, phase;
} hydro_sea_wave_t;
typedef struct hydro_sea {
    double current[3];
    int waves;
    hydro_sea_wave_t wave[HYDRO_SEA_WAVES_MAX];
} hydro_sea_t;
int hydro_set_sea(hydro_t *h, const hydro_sea_t *sea);
int hydro_sea_sample(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int64_t step_index, double dt,
                     float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_sea(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride, int64_t step0, void *stream);

/* Sea state, open loop: the sea for the caller who integrates - a simulator behind the plugin (PhysX integrates, the plugin
 * supplies the wrench) or an integrator of one's own around hydro_step_wrench_tiled.  Two entries, each with the argument list
 * of its parent and `double time` in front of `stream`:
 *     hydro_step_wrench_tiled_sea = hydro_step_wrench_tiled    hydro_step_wrench_aos_sea = hydro_step_wrench_aos
 * MODEL.  "WATER AT A BODY" above with ONE change: t = time, in seconds, an fp64 value taken as given, replaces
 * t = (step0 + k) * dt.  Everything from x_j = fma(-omega_j, t, phi_j) onwards is the stated order, in the same code.  The
 * wrench is that of the state with p_z - eta and v - u and of the previous velocity with pv[0:3] - u: fp32 subtractions with
 * the same u, so the finite-difference acceleration stays the body's own.
 * IDENTITY.  (double)1 * time == time exactly, so hydro_sea_sample(step_index = 1, dt = time) writes exactly the [eta, u] these
 * entries use at time > 0; at time == 0 it is step_index = 0 (with any dt > 0).  A step is therefore, bit for bit, the parent
 * entry on the relative state built from that sample.
 * PREVIOUS VELOCITY.  The engine-owned previous velocity (the array-of-structs entry; the tiled entry with prev == NULL)
 * receives the TRUE velocity, never the relative one.  With a caller-owned `prev` nothing is written but the wrench.
 *   no sea set      : the launch and its bits are those of the parent entry with the same arguments (`time` is validated all
 *                     the same).
 *   a sea set       : kernels of their own beside the parents' (256-thread blocks whatever hydro_set_tuning's block_threads says).
 * A sea with no current and no waves (or waves of amplitude 0) gives the parent's bits, sign of zero included.  HYDRO_E_ARG for
 * a non-finite time, time < 0 or time > 2^52; after that the parent's refusals in the parent's order - all before anything is
 * launched or written.  Asynchronous, no allocation, no synchronisation, safe to capture: a captured launch replays at the
 * frozen `time` it was captured with - capture current-only seas.
 * NOT COVERED - these step through still water whatever is set: hydro_step_wrench_tiled_ke, hydro_step_wrench_tiled_batch, the
 * plain-SoA hydro_step_wrench[_ext], and the component / calculator entries hydro_step_components[_aos] (the calculator takes
 * explicit accelerations and keeps the reference's signature).  Cost and registers: DESIGN.md section 23. */
int hydro_step_wrench_tiled_sea(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                const float *prev, int64_t prev_tile_stride, double dt,
                                float *wrench, int64_t wrench_tile_stride, double time, void *stream);
int hydro_step_wrench_aos_sea(hydro_t *h, int64_t n, const float *positions, const float *orientations, int quat_xyzw,
                              const float *velocities, double dt, float *forces, float *torques, double time, void *stream);

/* Seabed: a floor under the water for the closed-loop steps - the horizontal plane z = z_b, scene-wide like the density, the
 * gravity and the sea.  A body touches it through the EIGHT CORNERS of the box the buoyancy already uses (x/y/zDimension),
 * each a penalty contact: a spring and a damper along z that never pull (no adhesion) and a Coulomb friction with a
 * regularised direction and a capped tangential damping.  Bodies stay independent: nothing couples two of them.  Only
 * hydro_step_fused_tiled_multi_bed and hydro_seabed_wrench know the bed: the wrench-only, array-of-structs, batch, component
 * and plugin entries, and the other five closed-loop entries (hydro_step_fused_tiled, _multi, _multi_rec, _multi_app,
 * _multi_ctl, _multi_sea), ignore it whatever is set here - their bodies sink for ever.
 *
 * hydro_seabed_t.  The five contact constants are MASS-NORMALISED - the force is the constant times the body's mass - so one
 * set serves a 2 kg link and a 500 kg buoy:
 *     z              z_b, height of the plane (m).  Finite; may be above 0.
 *     stiffness      kappa >= 0, normal spring per corner and unit of the body's mass (1/s^2)
 *     damping        beta >= 0, normal damper per corner and unit mass (1/s)
 *     friction       mu >= 0, Coulomb coefficient
 *     slip_speed     v_s > 0, regularisation of the friction direction (m/s)
 *     friction_rate  gamma >= 0, cap on the tangential damping the friction may amount to, per corner and unit mass (1/s)
 * RULE OF THUMB for a step dt, per corner: kappa dt^2 <= 0.04 and beta dt, gamma dt <= 0.04 - explicit penalty forces
 * overshoot inside one step beyond that (without the cap the friction's slope mu N / v_s does, whatever kappa and beta are:
 * DESIGN.md section 18).  kappa = (0.2 / dt)^2, beta = gamma = 0.04 / dt, mu = 0.5, v_s = 0.01 bring boxes of 1.05 to 7.8 times
 * the water's density to rest on four corners at dt = 1/60 and 1/120 with implicit drag; a box at rest stands
 * g (1 - rho / rho_body) / (4 kappa) below z_b.
 *
 * THE CONTACT WRENCH of a body with state s = [p | q | v | omega] (the TRUE state the step starts from), box (dx, dy, dz) and
 * mass m, in fp32, in exactly this order (fma(a, b, c): a * b + c rounded once; the six constants are rounded ONCE from
 * double to fp32 by hydro_set_seabed):
 *     R            the fp32 matrix of q as given, non-unit included - the form the integrator and the body-frame applied
 *                  wrench use: with x2 = q_x + q_x ..., R_00 = 1 - (q_y y2 + q_z z2), R_01 = q_x y2 - q_w z2, ...
 *     A_k = 0.5 * (R_k0 * dx),  B_k = 0.5 * (R_k1 * dy),  C_k = 0.5 * (R_k2 * dz)          k = x, y, z
 *   for corner i = 0 .. 7 with signs (s_x, s_y, s_z) = (i & 1 ? + : -, i & 2 ? + : -, i & 4 ? + : -), in ascending i:
 *     r_k     = (s_x A_k + s_y B_k) + s_z C_k                          two fp32 additions per component
 *     delta   = z_b - (p_z + r_z)                                      the corner contributes only if delta > 0
 *     u_x     = fma(omega_y, r_z, fma(-omega_z, r_y, v_x))             u = v + omega x r, world frame;
 *     u_y     = fma(omega_z, r_x, fma(-omega_x, r_z, v_y)),  u_z = fma(omega_x, r_y, fma(-omega_y, r_x, v_z))
 *     a       = max(0, fma(kappa, delta, -(beta * u_z))),  N = m * a   no adhesion
 *     c       = m * min((mu * a) * rsqrt(fma(v_s, v_s, fma(u_y, u_y, u_x * u_x))), gamma)
 *                                                                      = min(mu N / sqrt(u_x^2 + u_y^2 + v_s^2), m gamma);
 *                                                                      rsqrt: hardware seed + one Newton step,
 *                                                                      y = seed; y = fma(fma(-x * y, y, 1), 0.5 * y, y)
 *     t_x = c * u_x,  t_y = c * u_y                                    F = (-t_x, -t_y, N)
 *     W_0 = W_0 - t_x,  W_1 = W_1 - t_y,  W_2 = W_2 + N                W starts from +0
 *     W_3 = fma(r_y, N, fma(r_z, t_y, W_3))                            r x F
 *     W_4 = fma(-r_z, t_x, fma(-r_x, N, W_4)),  W_5 = fma(r_y, t_x, fma(-r_x, t_y, W_5))
 * W = [force at | torque about] the body origin, world frame.  IN A STEP it is added to the step's wrench with one fp32 add
 * per component - after the clamped hydrodynamic wrench, after the applied wrench and the pose hold, before the integrator.
 * The sum is what the integrator takes (with implicit_drag it stands where f stood) and what the recorder logs.  A body with
 * no contributing corner has its wrench left untouched: +0 is NOT added, the sign of a zero survives.  Whole wavefronts of
 * bodies whose lowest corner, p_z - ((|A_z| + |B_z|) + |C_z|), is not below z_b skip the contact altogether; that value is,
 * bit for bit, the smallest p_z + r_z, so skipping changes no bit.
 * THE SEA DOES NOT TOUCH THE BED: the bed sees the true state, never the state relative to the water, and the wave field
 * stays the deep-water one however shallow z_b makes the scene.
 * NOT MODELLED: slope and terrain; rolling and spinning friction; face or edge contact other than through the corners (a box
 * lying flat is held by its four lower corners); body-to-body contact.
 *
 * hydro_set_seabed: bed == NULL clears the bed.  HYDRO_E_ARG for a non-finite value, a negative stiffness, damping, friction
 * or friction_rate, slip_speed <= 0, a constant beyond fp32 range (a slip speed whose fp32 square is 0 or infinite
 * included) - the previous bed stays in force.  Host-side only: no device memory, no synchronisation; the constants travel as
 * kernel arguments, so a captured launch replays with the bed of the moment it was captured.
 *
 * hydro_seabed_wrench: writes the tiled 6-field W ([tiles][6][64] floats, tile stride out_tile_stride >= 384) of bodies
 * 0 .. n - 1 in `state` - exactly what a step that starts from `state` adds; +0 in all six fields for a body that does not
 * touch.  Uses the engine's parameters (dimensions, mass).  A small kernel of its own; asynchronous on `stream`.
 * HYDRO_E_STATE without a bed or without parameters; HYDRO_E_ARG for n > capacity, a null or misaligned buffer.
 *
 * hydro_step_fused_tiled_multi_bed: exactly the signature and the rules of hydro_step_fused_tiled_multi_sea.
 *   no bed set      : the launch and its bits are those of hydro_step_fused_tiled_multi_sea with the same arguments (which
 *                     without a sea are those of hydro_step_fused_tiled_multi_ctl).
 *   a bed set       : log, applied, control and the sea are each still optional; the hydrodynamic wrench is taken through
 *                     the sea if one is set (without one no view is formed: the bits of the entries without a sea), what is
 *                     added for the three pointers is what hydro_step_fused_tiled_multi_ctl adds, then W.
 * The refusals are those of hydro_step_fused_tiled_multi_sea, in its order; the bed adds none at launch time.  Asynchronous,
 * no allocation, no synchronisation, safe to capture (the bed does not depend on time; waves in a replay stay frozen).
 * Cost and registers: DESIGN.md section 18.  New functionality; the reference has no seabed of its own (its floor is the
 * simulator's rigid-body contact). */
typedef struct hydro_seabed {
    double z, stiffness, damping, friction, slip_speed, friction_rate;
} hydro_seabed_t;
int hydro_set_seabed(hydro_t *h, const hydro_seabed_t *bed);
int hydro_seabed_wrench(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                        float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_bed(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride, int64_t step0, void *stream);

/* Mooring: something to tie a body down with in the closed-loop steps - per body ONE line from an anchor fixed in the world
 * to a fairlead fixed in the body: a spring and a damper along the line that act only while the line is stretched and never
 * push.  A buoy moored to the seabed and an ROV on a tether are the same model.  Bodies stay independent: a line joins one
 * body to a fixed point, never two bodies.  Only hydro_step_fused_tiled_multi_moor and hydro_mooring_wrench know lines; every
 * other entry ignores them.
 *
 * THE RECORD `mooring`: HYDRO_MOOR_FIELDS = 9 floats per body, tiled ([tiles][9][64] floats, tile stride
 * mooring_tile_stride >= 576, 16-byte aligned, whole tiles, addressed like `control`), in this order:
 *     a(3)   anchor, world frame (m)
 *     b(3)   fairlead, body frame (m)
 *     L0     unstretched length (m), >= 0
 *     k      stiffness (N/m), >= 0
 *     c      damping along the line (N s/m), >= 0
 * It is the caller's device buffer and is READ AT EVERY LAUNCH, like `applied` and `control`: a device-side winch may
 * rewrite L0 between launches.  A body without a line has k = c = 0.  The contents are the caller's and are not validated on
 * the device: a lane HAS A LINE if k > 0 or c > 0 (a NaN is neither); with a line, negative or non-finite values are
 * computed as given (k < 0 gives a tension that is clamped to 0 while the line is stretched, c < 0 a negative damper).
 * RULE OF THUMB for a step dt and a body of mass m: k dt^2 / m <= 0.04 and c dt / m <= 0.04 - an explicit spring overshoots
 * inside one step beyond that, and at k dt^2 / m = 0.25 the tension chatters to zero.
 * k = 0.004 m / dt^2, c = 0.02 m / dt hold a 500 kg buoy in a 0.5 m/s current at dt = 1/60.
 *
 * THE LINE'S WRENCH on a body with state s = [p | q | v | omega] (the TRUE state the step starts from, never the one
 * relative to the water), in fp32, in exactly this order (fma(a, b, c): a * b + c rounded once; rsqrt: hardware seed + one
 * Newton step, as for the seabed):
 *     R      the fp32 matrix of q as given, non-unit included (the form the seabed and the integrator use)
 *     r_i    = fma(R_i2, b_z, fma(R_i1, b_y, R_i0 * b_x))              the fairlead's arm, world frame
 *     e_i    = (a_i - p_i) - r_i                                       two subtractions: fairlead -> anchor
 *     l2     = fma(e_z, e_z, fma(e_y, e_y, e_x * e_x)),  inv = rsqrt(l2),  l = l2 * inv
 *     x      = l - L0                                                  the line is TAUT only if x > 0 (l2 = 0 gives NaN: not taut)
 *     u_x    = fma(omega_y, r_z, fma(-omega_z, r_y, v_x))              u = v + omega x r, the seabed's corner velocity;
 *     u_y    = fma(omega_z, r_x, fma(-omega_x, r_z, v_y)),  u_z = fma(omega_x, r_y, fma(-omega_y, r_x, v_z))
 *     un     = fma(u_z, e_z, fma(u_y, e_y, u_x * e_x)) * inv           > 0: the fairlead approaches the anchor
 *     T      = max(0, fma(k, x, -(c * un)))                            tension; a line cannot push
 *     F_i    = (T * inv) * e_i
 *     M_x    = fma(r_y, F_z, -(r_z * F_y)),  M_y = fma(r_z, F_x, -(r_x * F_z)),  M_z = fma(r_x, F_y, -(r_y * F_x))
 * W = [F | M]: force at, torque about the body origin, world frame.  IN A STEP it is added to the step's wrench with one
 * fp32 add per component - after the clamped hydrodynamic wrench, the applied wrench, the pose hold and the seabed, before
 * the integrator.  The sum is what the integrator takes (with implicit_drag it stands where f stood) and what the recorder
 * logs.  A body without a line, with a line that is not taut, or with a T that is not > 0 has its wrench left untouched:
 * +0 is NOT added, the sign of a zero survives.  Whole wavefronts without a line skip the evaluation; that changes no bit.
 * NOT MODELLED: the line's mass and catenary sag; drag on the line; the line lying on the bed; more than one line per
 * body by THIS entry (up to four are a spread: "Mooring spread", below); a line between two bodies ("Tether").
 *
 * hydro_mooring_wrench: writes the tiled 6-field W ([tiles][6][64] floats, tile stride out_tile_stride >= 384) of bodies
 * 0 .. n - 1 in `state` - exactly what a step that starts from `state` adds; +0 in all six fields for a body whose line adds
 * nothing.  A small kernel of its own; asynchronous on `stream`.  HYDRO_E_STATE without parameters; HYDRO_E_ARG for
 * n > capacity, a null or misaligned buffer, a stride below 832 (state) / 576 (mooring) / 384 (out), or `out` overlapping
 * an input.
 *
 * hydro_step_fused_tiled_multi_moor: the signature and the rules of hydro_step_fused_tiled_multi_bed, with `mooring` and its
 * stride in front of step0.
 *   mooring == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_bed with the same arguments.
 *   mooring != NULL : log, applied, control, the sea (hydro_set_sea) and the bed (hydro_set_seabed) are each still optional,
 *                     and what they add is what the entries without lines add (no sea: no view is formed; no bed: no broad
 *                     phase); then W.  Like hydro_step_fused_tiled_multi_bed, this entry knows the sea and the bed.
 * The refusals are those of hydro_step_fused_tiled_multi_bed, in its order, then the mooring's, behind `control`'s: a stride
 * below 576 or misaligned buffer, a record that overlaps an output (state_out, prev_out, log) - HYDRO_E_ARG, and nothing is
 * launched or written.  Asynchronous, no allocation, no synchronisation, safe to capture (a line does not depend on time).
 * Cost and registers: DESIGN.md section 19.  New functionality; the reference has no mooring of its own. */
int hydro_mooring_wrench(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                         const float *mooring, int64_t mooring_tile_stride,
                         float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_moor(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                      const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                      float *state_out, int64_t out_tile_stride,
                                      float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double *ke_out_dev,
                                      float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t *rows_written_host,
                                      const float *applied, int64_t applied_tile_stride, int applied_frame,
                                      const float *control, int64_t control_tile_stride,
                                      const float *mooring, int64_t mooring_tile_stride, int64_t step0, void *stream);

/* Extremes: what a design-load study asks of a long resident run - the peak line tension, how far the body wandered, how
 * deep or how high it got - as a running record per body that the kernel updates in every step.  Between the first and the
 * last step of a launch the states exist in registers only, and the line tension T is never visible at all; the record
 * costs eight floats per body and launch to read and to write, whatever the number of steps.  Only
 * hydro_step_fused_tiled_multi_ext and hydro_extremes_reset know it.  Bodies stay independent.
 *
 * THE RECORD `extremes`: HYDRO_EXT_FIELDS = 8 floats per body, tiled ([tiles][8][64] floats, tile stride
 * extremes_tile_stride >= 512, 16-byte aligned, whole tiles, addressed like `mooring`), in this order:
 *     x_min x_max | y_min y_max | z_min z_max | speed2_max | tension_max
 * It is the caller's device buffer.  Unlike `applied`, `control` and `mooring` it is READ AT THE START OF A LAUNCH AND
 * WRITTEN AT ITS END: the extremes accumulate across launches, chunks and graph replays until the caller resets them.
 * Lanes >= n of the last tile are never written.
 *
 * THE SAMPLE, after every step k of the launch, is the state the step produced - the values a recorder row with
 * fields = 19 holds for that step:
 *     x, y, z   s[0..2] after the step
 *     speed2    fma(v_z, v_z, fma(v_y, v_y, v_x * v_x)) of s[7..9] after the step, in fp32 (fma: rounded once)
 *     tension   the T the mooring formed IN that step, from the state the step started from ("Mooring", above); +0 where
 *               the line adds nothing: no line, a slack line, a T that is not > 0, or no mooring record at all.  With a
 *               spread of L lines ("Mooring spread", below) it is the LARGEST tension of any of the body's lines in that
 *               step: acc = +0, then acc = (t_l > acc) ? t_l : acc over the layers in ascending order, t_l the layer's T
 *               where its line pulls and +0 where it adds nothing - with L = 1 the value above, bit for bit
 * THE UPDATE is an explicit compare-and-select, never fminf / fmaxf:
 *     m = (x < m) ? x : m            M = (x > M) ? x : M
 * so a NaN sample never enters, a NaN accumulator stays NaN, and an equal value (+0 against -0 included) leaves the
 * accumulator's bits as they are.
 * NOT PROVIDED: means and variances; the step at which an extreme occurred; the extremes of the launch's INITIAL state (seed
 * the record from it with hydro_extremes_reset if it is to count); extremes of the wrench.
 *
 * hydro_extremes_reset: state == NULL writes [+inf, -inf, +inf, -inf, +inf, -inf, +0, +0] for bodies 0 .. n - 1; with a
 * tiled state it writes the record of that one sample: min = max = p, speed2 of its v, tension +0.  A small kernel of its
 * own; asynchronous on `stream`; needs no parameters.  HYDRO_E_ARG for n > capacity, a null or misaligned buffer, a stride
 * below 832 (state) / 512 (extremes), or the two overlapping.
 *
 * hydro_step_fused_tiled_multi_ext: the signature and the rules of hydro_step_fused_tiled_multi_moor, with `extremes` and
 * its stride in front of step0.
 *   extremes == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_moor with the same arguments.
 *   extremes != NULL : log, applied, control, the sea, the bed AND `mooring` are each optional, and each adds exactly what
 *                      it adds in the entries without extremes; state_out, prev_out, the kinetic-energy pair and the log
 *                      are bit for bit those of hydro_step_fused_tiled_multi_moor with the same arguments - nothing the
 *                      record computes feeds back.
 * The refusals are those of hydro_step_fused_tiled_multi_moor, in its order, then the extremes', behind the mooring's: a
 * stride below 512 or a misaligned buffer, a record that overlaps an output (state_out, prev_out, log) or - since it is
 * written - an input of the launch (state, prev, applied, control, mooring): HYDRO_E_ARG, and nothing is launched or
 * written.  Asynchronous, no allocation, no synchronisation, safe to capture: a replay accumulates.
 * Cost and registers: DESIGN.md section 20.  New functionality; the reference keeps no extremes. */
int hydro_extremes_reset(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                         float *extremes, int64_t extremes_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_ext(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride,
                                     const float *mooring, int64_t mooring_tile_stride,
                                     float *extremes, int64_t extremes_tile_stride, int64_t step0, void *stream);

/* Tether: ONE tension-only line between TWO BODIES in the closed-loop steps - an ROV on an umbilical under a buoy, a towed
 * body behind a driven one, a float and its sinker: a spring and a damper along the line that act only while the line is
 * stretched and never push.  It is the one term that couples bodies: the partner's fairlead of the very step is read from
 * the partner's lane of the wavefront, inside the kernel.  Only hydro_step_fused_tiled_multi_teth and hydro_tether_wrench know
 * tethers; every other entry ignores them.
 *
 * THE RECORD `tether`: HYDRO_TETH_FIELDS = 7 floats per body, tiled ([tiles][7][64] floats, tile stride
 * tether_tile_stride >= 448, 16-byte aligned, whole tiles, addressed like `mooring`), in this order:
 *     b(3)     this body's fairlead, in its own body frame (m)
 *     L0       unstretched length (m), >= 0
 *     k        stiffness (N/m), >= 0
 *     c        damping along the line (N s/m), >= 0
 *     partner  the other body, as a LANE INDEX WITHIN THE SAME TILE (0 .. 63), stored as a float: body 64 t + partner
 * It is the caller's device buffer and is READ IN EVERY STEP of every launch; between launches a device-side winch may
 * rewrite L0 (on both lanes of a pair).  A lane HAS A TETHER if k > 0 or c > 0 (a NaN is neither); a body without one has
 * k = c = 0.  SCOPE: at most one tether per body; both bodies of a pair in one tile, 64 t .. 64 t + 63; the pairing an
 * involution (partner of partner = self); both records of a pair carry the same L0, k, c (each its own b); the partner a
 * body < n.  NO PARTNER INDEX EVER FORMS A MEMORY ADDRESS: the kernel uses (int)partner & 63 as a lane of its own wavefront.
 * A malformed record - a partner that is not mutual, a partner among the lanes >= n of the last tile (it answers +0),
 * constants that differ between the two, negative or non-finite values - is computed as given and cannot fault; the
 * contents are not validated on the device (the Python host validates what it builds).  A partner that is not finite or
 * lies outside the range of int names an unspecified lane of the tile and still never an address.
 * RULE OF THUMB for a step dt: with the reduced mass mu = m_a m_b / (m_a + m_b), k dt^2 / mu <= 0.04 and c dt / mu <= 0.04
 * (the mooring's rule, DESIGN.md section 19, for the pair's relative motion).
 *
 * THE TETHER'S WRENCH on a body with state s = [p | q | v | omega] (the TRUE state the step starts from, never the one
 * relative to the water), in fp32, in exactly this order (fma(a, b, c): a * b + c rounded once; rsqrt: hardware seed + one
 * Newton step, as for the mooring):
 *     R      the fp32 matrix of q as given, non-unit included
 *     r_i    = fma(R_i2, b_z, fma(R_i1, b_y, R_i0 * b_x))              the fairlead's arm, world frame
 *     P_i    = p_i + r_i                                               the fairlead, world frame (one add)
 *     U_x    = fma(omega_y, r_z, fma(-omega_z, r_y, v_x))              U = v + omega x r, the mooring's three forms;
 *     U_y    = fma(omega_z, r_x, fma(-omega_x, r_z, v_y)),  U_z = fma(omega_x, r_y, fma(-omega_y, r_x, v_z))
 *     P', U' = the partner's P and U of this step                      (six lane exchanges; no memory)
 *     e_i    = P'_i - P_i                                              fairlead -> partner's fairlead
 *     l2     = fma(e_z, e_z, fma(e_y, e_y, e_x * e_x)),  inv = rsqrt(l2),  l = l2 * inv
 *     x      = l - L0                                                  the line is TAUT only if x > 0 (l2 = 0 gives NaN: not taut)
 *     dU_i   = U'_i - U_i
 *     rate   = fma(dU_z, e_z, fma(dU_y, e_y, dU_x * e_x)) * inv        > 0: the fairleads part
 *     T      = max(0, fma(k, x, c * rate))                             tension; a line cannot push
 *     F_i    = (T * inv) * e_i
 *     M_x    = fma(r_y, F_z, -(r_z * F_y)),  M_y = fma(r_z, F_x, -(r_x * F_z)),  M_z = fma(r_x, F_y, -(r_y * F_x))
 * W = [F | M]: force at, torque about the body origin, world frame.  IN A STEP it is added to the step's wrench with one
 * fp32 add per component - behind the mooring line's wrench, in front of the integrator.  The sum is what the integrator
 * takes (with implicit_drag it stands where f stands) and what the recorder logs.  A line PULLS if the lane has a tether and
 * x > 0 and T > 0; otherwise the wrench is left untouched: +0 is NOT added.  Whole wavefronts without a tether skip the
 * evaluation; that changes no bit.
 * EQUAL AND OPPOSITE, EXACTLY (a property that is tested): negation is exact in fp32, so the partner forms -e and -dU and from
 * them the same l2, inv, x, rate and T, and the force -F, bit for bit.  The pair's linear momentum changes by the rounding of
 * the integrator's additions alone.  (The torques r x F and r' x -F are each body's own and need not cancel.)
 * NOT MODELLED: chains, and more than one tether per body; pairs across tiles; the line's mass, sag and drag; the tether's
 * tension in the extremes record - tension_max stays the mooring line's and is unchanged by a tether.  (The first and the
 * third are the TETHER NET's, below: up to four of these records in layers, and a cable of small bodies has what one
 * massless line has not.)
 *
 * hydro_tether_wrench: writes the tiled 6-field W ([tiles][6][64] floats, tile stride out_tile_stride >= 384) of bodies
 * 0 .. n - 1 in `state` - exactly what a step that starts from `state` adds; +0 in all six fields for a body whose line adds
 * nothing - and, unless `tension` is NULL, T in a tiled one-field record ([tiles][1][64] floats, tile stride >= 64; +0
 * likewise).  A small kernel of its own; asynchronous on `stream`.  HYDRO_E_STATE without parameters; HYDRO_E_ARG for
 * n > capacity, a null or misaligned buffer, a stride below 832 (state) / 448 (tether) / 384 (out) / 64 (tension), or an
 * output overlapping an input or the other output.
 *
 * hydro_step_fused_tiled_multi_teth: the signature and the rules of hydro_step_fused_tiled_multi_ext, with `tether` and its
 * stride in front of step0.
 *   tether == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_ext with the same arguments.
 *   tether != NULL : log, applied, control, the sea, the bed, `mooring` AND `extremes` are each optional, and each adds
 *                    exactly what it adds in the entries without tethers; then W.  A record of zeros gives the bits of
 *                    hydro_step_fused_tiled_multi_ext.
 * The refusals are those of hydro_step_fused_tiled_multi_ext, in its order, then the tether's, behind the extremes': a stride
 * below 448 or a misaligned buffer, a record that overlaps an output (state_out, prev_out, log, extremes): HYDRO_E_ARG, and
 * nothing is launched or written.  Asynchronous, no allocation, no synchronisation, safe to capture (a tether does not
 * depend on time).  Cost and registers: DESIGN.md section 22.  New functionality; the reference has no tethers. */
int hydro_tether_wrench(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                        const float *tether, int64_t tether_tile_stride,
                        float *out, int64_t out_tile_stride, float *tension, int64_t tension_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_teth(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                      const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                      float *state_out, int64_t out_tile_stride,
                                      float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double *ke_out_dev,
                                      float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t *rows_written_host,
                                      const float *applied, int64_t applied_tile_stride, int applied_frame,
                                      const float *control, int64_t control_tile_stride,
                                      const float *mooring, int64_t mooring_tile_stride,
                                      float *extremes, int64_t extremes_tile_stride,
                                      const float *tether, int64_t tether_tile_stride, int64_t step0, void *stream);

/* Tether net: SEVERAL tethers per body in the closed-loop steps - chains and cables of bodies: a lumped-mass umbilical or
 * riser (a string of small bodies joined by short lines, each carrying its share of mass, buoyancy and drag), a buoy with
 * a clump weight and a sinker below it, a towed array, a bridle.  No new physics: every line is the tether above, and the
 * bodies of a cable get their mass, sag and drag from the hydrodynamics every body has.
 *
 * THE RECORD: a net is L LAYERS of the tether record, 1 <= L <= HYDRO_TETH_LAYERS_MAX = 4, tiled as ONE record of 7 L
 * fields: [tiles][7 L][64] floats, layer l's field f in row 7 l + f, tile stride tether_tile_stride >= 448 L, 16-byte
 * aligned, whole tiles.  EACH LAYER IS A COMPLETE, VALID TETHER RECORD in the sense above (within a layer: at most one line
 * per body, the pairing an involution inside a tile, both ends the same L0, k, c): `tether + 448 l` with the net's tile
 * stride is an argument for hydro_tether_wrench, which is the net's probe, layer by layer.  A body may have a line in every
 * layer: a chain 0-1-2-3-4 is two layers, (0,1) (2,3) in layer 0 and (1,2) (3,4) in layer 1.  Two lines between the same
 * two bodies (a bridle) are two layers.  A layer of zeros is a layer without lines.
 * IN A STEP every line is evaluated exactly as hydro_step_fused_tiled_multi_teth evaluates its one, from the TRUE state the
 * step starts from (no line sees what another line did in this step), and the wrenches are added to the step's wrench IN
 * ASCENDING LAYER ORDER, one fp32 add per component each, behind the mooring line's wrench and in front of the
 * integrator: f = fl(fl(fl(f + W_0) + W_1) + ...) over the layers in which the body's line pulls.  A layer in which it does
 * not pull leaves f untouched: +0 is not added.  Equal and opposite forces hold bit for bit per line.
 * SCOPE: every line lies inside one tile of 64 bodies, 64 t .. 64 t + 63 - so a cable with its end bodies has at most 64
 * bodies; at most 4 lines per body; the tether tensions still do not enter the extremes record (tension_max stays the
 * mooring line's); no bending stiffness.
 * RULE OF THUMB for a step dt, per body i with mass m_i (Gershgorin on M^-1 K: a body between two springs is not a pair on
 * its reduced mass): 2 (sum of k over the body's lines) dt^2 / m_i <= 0.04 and 2 (sum of c) dt / m_i <= 0.04.
 *
 * hydro_step_fused_tiled_multi_net: the signature and the rules of hydro_step_fused_tiled_multi_teth, with `tether_layers`
 * between tether_tile_stride and step0.
 *   tether == NULL      : the launch and its bits are those of hydro_step_fused_tiled_multi_ext; tether_layers is ignored.
 *   tether_layers == 1  : the bits of hydro_step_fused_tiled_multi_teth with the same record.
 *   trailing layers of zeros change no bit.
 * The refusals are those of hydro_step_fused_tiled_multi_teth, in its order, then: tether_layers outside
 * 1 .. HYDRO_TETH_LAYERS_MAX; a stride below 448 tether_layers or a misaligned buffer; a net that overlaps an output
 * (state_out, prev_out, log, extremes) anywhere in its 7 tether_layers fields: HYDRO_E_ARG, and nothing is launched or
 * written.  Asynchronous, no allocation, no synchronisation, safe to capture.  The layers are a loop inside the kernel:
 * cost and registers in DESIGN.md section 24.  New functionality; the reference has no tethers. */
int hydro_step_fused_tiled_multi_net(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride,
                                     const float *mooring, int64_t mooring_tile_stride,
                                     float *extremes, int64_t extremes_tile_stride,
                                     const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                     int64_t step0, void *stream);

/* Link tensions: the PEAK TENSION of every tether, tracked inside the closed-loop steps.  The load that sizes a cable is
 * the largest tension each of its links ever carried.  Inside a resident launch the states between the first and the last
 * step exist in registers only, and so do the tensions: hydro_tether_wrench sees them at the ends of launches alone.  The
 * record below is kept by the stepping kernel itself, in every step.
 *
 * THE RECORD: a running maximum per body and per layer of the net, tiled [tiles][L][64] floats, L = tether_layers; row l
 * belongs to layer l of the net.  Tile stride tether_peaks_tile_stride >= 64 L floats, a multiple of 4; 16-byte aligned;
 * whole tiles - the rules of every tiled record.  The caller's device buffer.
 * THE SAMPLE of body i, layer l, in a step is what the step's evaluation of that line formed: T where the line pulls, +0
 * where it adds nothing (no line, a slack line, or a T that is not > 0) - exactly the value hydro_tether_wrench writes to
 * its `tension` output for layer l and the state the step starts from.
 * THE UPDATE is the extremes record's: M <- (T > M) ? T : M, a compare-and-select.  A NaN sample never enters, a NaN in the
 * record stays, an equal value leaves the record's bits.  (A sample of +0 changes nothing and is not written.)  Both bodies
 * of a link get the same T bit for bit (antisymmetry), so both hold the same maximum.
 * The record ACCUMULATES over launches, chunks and graph replays.  The empty record is all +0: a plain zero fill resets it,
 * and there is no reset entry.  A slot holds +0, a positive value or a NaN - what the entry itself leaves in a record that
 * started empty; a slot seeded with the sign bit set (-0, a negative value) is outside the contract and is kept as it is.
 * The padding lanes of the last tile, and the floats between 64 L and the tile stride, are never written.
 * NOTHING FEEDS BACK: state_out, prev_out, the kinetic energy, the log and the extremes record are bit for bit those of
 * hydro_step_fused_tiled_multi_net with the same arguments; tension_max of the extremes record stays the mooring line's.
 *
 * hydro_step_fused_tiled_multi_peak: the signature and the rules of hydro_step_fused_tiled_multi_net, with `tether_peaks`,
 * `tether_peaks_tile_stride` between tether_layers and step0.
 *   tether_peaks == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_net; the stride is ignored.
 * The refusals are those of hydro_step_fused_tiled_multi_net, in its order, then: a record with tether == NULL; a stride
 * below 64 tether_layers or a misaligned record; a record that overlaps state_out, prev_out, the log, state, prev, applied,
 * control, mooring, the net or the extremes record: HYDRO_E_ARG, and nothing is launched or written.  Asynchronous, no
 * allocation, no synchronisation, safe to capture.  The update is one vector memory instruction per pulling line and step
 * (DESIGN.md section 25).  SCOPE: the maximum only - not its time of occurrence, no minima, no cycle counts.  New
 * functionality; the reference has no tethers. */
int hydro_step_fused_tiled_multi_peak(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                      const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                      float *state_out, int64_t out_tile_stride,
                                      float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double *ke_out_dev,
                                      float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t *rows_written_host,
                                      const float *applied, int64_t applied_tile_stride, int applied_frame,
                                      const float *control, int64_t control_tile_stride,
                                      const float *mooring, int64_t mooring_tile_stride,
                                      float *extremes, int64_t extremes_tile_stride,
                                      const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                      float *tether_peaks, int64_t tether_peaks_tile_stride,
                                      int64_t step0, void *stream);

/* Mooring spread: a body on up to four anchored lines - the three- or four-line spread that keeps a floating body on station,
 * where one line only gives it a watch circle.  No new physics: every line is a line of "Mooring" (above), and the section
 * states only how several of them are laid out and combined.  Only hydro_step_fused_tiled_multi_spread knows spreads.
 *
 * THE RECORD: a spread is L LAYERS of the mooring record, 1 <= L <= HYDRO_MOOR_LAYERS_MAX = 4, tiled as ONE record of 9 L
 * fields: [tiles][9 L][64] floats, field f of layer l in row 9 l + f, tile stride mooring_tile_stride >= 576 L, 16-byte
 * aligned, whole tiles.  Each layer is a complete mooring record: `mooring + 576 l` with the spread's stride is a valid
 * argument of hydro_mooring_wrench, which is how a host sees one layer's wrenches.  A layer of zeros is a layer without
 * lines.  The caller's device buffer, READ IN EVERY STEP of every launch (a launch must not rewrite it under a running one).
 *
 * IN A STEP every line is evaluated exactly as the single line is - the line's wrench above, from the TRUE state the step
 * starts from - and the wrenches are added to the step's wrench in ASCENDING LAYER ORDER, behind the seabed's and in front
 * of the tethers', one fp32 add per component each: f = fl(fl(f + W_0) + W_1) ..., over the layers whose line pulls.  A
 * layer whose line adds nothing (no line, slack, a T that is not > 0) leaves the wrench untouched: +0 is NOT added.
 * tension_max of the extremes record takes the largest tension of the body's lines in the step ("Extremes", above).
 * RULE OF THUMB, per body: (sum of k) dt^2 / m <= 0.04 and (sum of c) dt / m <= 0.04 over the body's lines - they may all
 * be taut at once, and the anchors are fixed (no factor 2 as in a net, where both ends move).
 * NOT MODELLED: what "Mooring" does not model; more than four lines per body.  NOT PROVIDED: the peak tension of each line
 * on its own (the anchored counterpart of "Link tensions") - the extremes record keeps the largest of them only.
 *
 * hydro_step_fused_tiled_multi_spread: the signature and the rules of hydro_step_fused_tiled_multi_peak, with
 * `mooring_layers` between mooring_tile_stride and `extremes`.
 *   mooring == NULL     : the launch and its bits are those of hydro_step_fused_tiled_multi_peak; mooring_layers is ignored.
 *   mooring_layers == 1 : the bits are those of hydro_step_fused_tiled_multi_peak with the same record.
 *   trailing layers of zeros change no bit.
 * Every other option is still optional and adds what it adds in hydro_step_fused_tiled_multi_peak.  The refusals are those
 * of hydro_step_fused_tiled_multi_peak, in its order (the record is first held to a single line's rules: a stride below
 * 576), then: mooring_layers outside 1 .. HYDRO_MOOR_LAYERS_MAX; a stride below 576 mooring_layers or a misaligned record; a
 * spread any layer of which overlaps state_out, prev_out, the log, the extremes record or tether_peaks: HYDRO_E_ARG, and
 * nothing is launched or written.  Asynchronous, no allocation, no synchronisation, safe to capture.  Cost and registers:
 * DESIGN.md section 28.  New functionality; the reference has no mooring of its own. */
int hydro_step_fused_tiled_multi_spread(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                        const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                        float *state_out, int64_t out_tile_stride,
                                        float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                        int rotational, double *ke_out_dev,
                                        float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                        int64_t row0, int64_t *rows_written_host,
                                        const float *applied, int64_t applied_tile_stride, int applied_frame,
                                        const float *control, int64_t control_tile_stride,
                                        const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                        float *extremes, int64_t extremes_tile_stride,
                                        const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                        float *tether_peaks, int64_t tether_peaks_tile_stride,
                                        int64_t step0, void *stream);

/* Sea spectrum: an irregular sea for the closed-loop steps - the model of "Sea state" (above), unchanged, with `waves` =
 * 0 .. HYDRO_SPECTRUM_WAVES_MAX = 64 components, enough to cut a Pierson-Moskowitz or JONSWAP spectrum of a given significant
 * wave height and peak period into bins.  The cap is a cost decision, not a design limit: a step pays for every component,
 * and nothing in the layout or the arithmetic depends on the number.
 *
 * WATER AT A BODY is "Sea state"'s, statement for statement: t, x_j, m_j, tau_j in fp64, th_j, r_j, c_j, s_j, eta, z_rel, e_j
 * and u in fp32, the sums taken in ASCENDING COMPONENT ORDER, eta starting from +0 and u from U.  For waves <= HYDRO_SEA_WAVES_MAX
 * eta and u are therefore, bit for bit, those of hydro_set_sea with the same components.  Every body evaluates every component;
 * c_j is formed a second time behind eta (the same instructions on the same inputs: the same bits), never stored.
 * RELATIVE STATE and NOT MODELLED: as in "Sea state".
 *
 * hydro_sea_spectrum_t: `current` U (m/s, world frame), `waves` and `wave`, the caller's array of `waves` components (read
 * during the call only; may be NULL when waves == 0).
 *
 * hydro_set_sea_spectrum: hydro_set_sea's rules for the current and for every component (one validator serves both), into an
 * engine-owned device table of its own (16 + 64 * 48 = 3088 B, allocated by the first call, freed by hydro_destroy), copied on
 * the engine's private stream and waited for.  spec == NULL clears the spectrum.  HYDRO_E_ARG for waves outside
 * 0 .. HYDRO_SPECTRUM_WAVES_MAX, a NULL `wave` with waves > 0, and whatever hydro_set_sea refuses of a component - the
 * previous spectrum stays in force.
 * A SPECTRUM AND A SEA EXCLUDE EACH OTHER, at set time: hydro_set_sea_spectrum(non-NULL) returns HYDRO_E_STATE while a sea is
 * set (clear it first: hydro_set_sea(h, NULL)), hydro_set_sea(non-NULL) returns HYDRO_E_STATE while a spectrum is set (clear it
 * first: hydro_set_sea_spectrum(h, NULL)); what was set stays in force.  Clearing with NULL is always allowed.
 * ONLY hydro_step_fused_tiled_multi_irr and hydro_sea_spectrum_sample know the spectrum: EVERY OTHER ENTRY IGNORES IT and steps
 * through the water it stepped through before - the sea of hydro_set_sea where it knows one, still water otherwise - as the
 * entries below hydro_step_fused_tiled_multi_bed ignore the bed.  (Besides them the two open-loop entries
 * hydro_step_wrench_tiled_irr and hydro_step_wrench_aos_irr know the spectrum: "Irregular sea in the open-loop steps" below.)
 *
 * hydro_sea_spectrum_sample: the signature and the rules of hydro_sea_sample, read against the spectrum: the [eta, u_x, u_y, u_z]
 * a step of hydro_step_fused_tiled_multi_irr that starts from `state` at step index `step_index` uses.  HYDRO_E_STATE without
 * a spectrum.
 *
 * hydro_step_fused_tiled_multi_irr: exactly the signature, the refusals and the refusal order of
 * hydro_step_fused_tiled_multi_spread.
 *   no spectrum set : the launch and its bits are those of hydro_step_fused_tiled_multi_spread with the same arguments - with
 *                     a sea of hydro_set_sea set, through that sea.
 *   a spectrum set  : log, applied, control, the bed, the spread, the extremes, the net and the link tensions are each still
 *                     optional and add what they add in hydro_step_fused_tiled_multi_spread; the hydrodynamic wrench is taken
 *                     through the spectrum.  One kernel family of its own serves every combination.
 * Trailing components of amplitude 0 change no bit.  Asynchronous, no allocation, no synchronisation, safe to capture: a
 * captured launch replays with the step0 it was captured with, i.e. at a frozen wave phase - capture current-only spectra.
 * Cost and registers: DESIGN.md section 29.  New functionality; the reference's water does not move. */
typedef struct hydro_sea_spectrum {
    double current[3];
    int waves;
    const hydro_sea_wave_t *wave;
} hydro_sea_spectrum_t;
int hydro_set_sea_spectrum(hydro_t *h, const hydro_sea_spectrum_t *spec);
int hydro_sea_spectrum_sample(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int64_t step_index, double dt,
                              float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_irr(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride,
                                     const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                     float *extremes, int64_t extremes_tile_stride,
                                     const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                     float *tether_peaks, int64_t tether_peaks_tile_stride,
                                     int64_t step0, void *stream);

/* Statistics: what a mooring designer takes from an irregular-sea run besides the peak - the mean and the standard deviation
 * of a response and its mean up-crossing rate, from which come the mean offset and mean tension, the significant response
 * 2 sigma, the zero-up-crossing period Tz = duration / up-crossings, the most probable maximum mu + sigma * sqrt(2 ln N_up)
 * of a storm of any length (Rayleigh), and - on the tension channel against the level +0 - the number of slack-to-taut events
 * of a line (snap loads).  A peak ("Extremes", above) is the largest sample of one random realisation; these are not.  Between
 * the first and the last step of a launch the states exist in registers only and the tension is never visible at all, so the
 * sums are kept where the extremes are kept: inside the stepping kernel, every step, for every body.  Only
 * hydro_step_fused_tiled_multi_stat and hydro_statistics_reset know them.  Bodies stay independent.
 *
 * TWO CHANNELS per launch, `channel_a` and `channel_b`, each one of HYDRO_STAT_X, _Y, _Z = 0 .. 2 (s[0..2]), HYDRO_STAT_VX,
 * _VY, _VZ = 3 .. 5 (s[7..9]) and HYDRO_STAT_TENSION = 6.  The two may be the same.  THE SAMPLE is taken where the extremes
 * take theirs: after every step k of the launch, of the state the step produced - the values a recorder row of that step
 * holds - and HYDRO_STAT_TENSION is EXACTLY the tension the extremes record samples in that step: the T the body's mooring
 * line or spread formed in it (the largest of a spread's), +0 where no line pulls or there is no mooring record.
 *
 * THE LEVEL RECORD `levels`: HYDRO_STAT_LEVEL_FIELDS = 2 floats per body, tiled ([tiles][2][64] floats, tile stride
 * levels_tile_stride >= 128 floats = 512 B, 16-byte aligned, addressed like `mooring`): the reference level L of the body for
 * slot a, then for slot b.  It is the caller's read-only device buffer, read from it in every step (as a mooring spread's layers
 * are); required whenever a statistics record is given.  L is any float: a NaN or infinite level poisons that body's slot.
 *
 * THE STATISTICS RECORD `statistics`: per tile of 64 bodies one hydro_statistics_tile_t,
 *     { double sums[4][64]; uint32_t words[3][64]; }    = HYDRO_STAT_TILE_BYTES = 2 816 B, HYDRO_STAT_BYTES_PER_BODY = 44
 *     sums  = S1_a, S2_a, S1_b, S2_b : the sum of d and of d * d of slot a, then of slot b, d the sample less its level
 *     words = up_a, up_b, n          : the two up-crossing words (below) and the number of samples
 * statistics_tile_stride counts 4-byte units like every stride of this header: >= 704 (2 816 B), a multiple of 4, the
 * buffer 16-byte aligned (so every double is 8-byte aligned).  It is the caller's device buffer, READ AT THE START OF A LAUNCH AND
 * WRITTEN AT ITS END like the extremes: it accumulates over launches, chunks and graph replays until it is reset.  Lanes >= n
 * of the last tile are never written.  THE RECORD DOES NOT REMEMBER ITS CHANNELS OR LEVELS: a caller that changes either
 * resets it first.
 *
 * THE ARITHMETIC is fixed so that a host reproduces the bits in plain IEEE double arithmetic.  Per slot and step, x the fp32
 * sample and L the fp32 level:
 *     d  = (double)x - (double)L          one fp64 subtraction (exact conversions)
 *     S1 = S1 + d                         one fp64 addition
 *     q  = d * d;   S2 = S2 + q           one fp64 product, rounded, then one fp64 addition: NO fused multiply-add anywhere
 * UP-CROSSINGS: above = (x > L), an fp32 compare, false for a NaN.  Bit 31 of an up-crossing word says "the last sample was
 * not above its level", bits 0 .. 30 are the count (modulo 2^31).  If bit 31 is set and `above`, the count goes up by one; then
 * bit 31 = !above.  A reset record has bit 31 clear, so the first sample never counts, and x == L is not above.  With L = +0
 * on the tension channel the count is the number of slack-to-taut events.
 * n is not touched inside the loop: the end of a launch adds `steps` to the value it reads from the record.  n is a uint32_t and
 * wraps modulo 2^32, as the count wraps modulo 2^31 without touching bit 31.
 * A NaN sample makes that body's S1 and S2 of that slot NaN for good and nobody else's; it is never above, so it leaves bit 31
 * set and the next sample above the level counts.  A sample equal to an infinite level gives d = NaN (Inf - Inf) likewise.
 * NOT PROVIDED: heave relative to the moving surface; covariances between channels; more than two channels per record;
 * statistics of the wrench; per-link statistics of tether nets.
 * SIGN SYMMETRY: exact, WITH ONE EXCEPTION.  A channel the map does not flip - z, vz and tension always,
 * and whichever of x, y, vx, vy it leaves alone - keeps every word of its slot.  A flipped channel, taken against the level
 * L' = -L, has d' = -d exactly: S1' = -S1 and S2 keeps its bits.  n keeps its bits.  The exception is the UP-CROSSING WORD OF A
 * FLIPPED CHANNEL: an up-crossing of L by x is a DOWN-crossing of -L by -x, which the record does not count - the image's word is
 * the scene's count of down-crossings, not its image (tests/symmetry.py, tests/test_symmetry_gpu.py).
 *
 * hydro_statistics_reset: sums +0.0 and words 0 for bodies 0 .. n - 1 (lanes >= n of the last tile are not written).  A small
 * kernel of its own; asynchronous on `stream`; needs no parameters.  HYDRO_E_ARG for n > capacity, a null or misaligned buffer
 * or a stride below 704.
 *
 * hydro_step_fused_tiled_multi_stat: the signature of hydro_step_fused_tiled_multi_irr with `statistics`, its stride, `levels`,
 * its stride, `channel_a` and `channel_b` in front of step0.
 *   statistics == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_irr with the same arguments; the
 *                        channels are still checked (0 .. 6), `levels` is not looked at.
 *   statistics != NULL : every other option is optional and adds what it adds in hydro_step_fused_tiled_multi_irr - through
 *                        the sea spectrum if one is set, through the sea of hydro_set_sea or still water otherwise; state_out,
 *                        prev_out, the kinetic-energy pair, the log, the extremes and the link tensions are bit for bit
 *                        those of hydro_step_fused_tiled_multi_irr - nothing the record computes feeds back.
 * The refusals are those of hydro_step_fused_tiled_multi_irr, in its order, then: a channel outside 0 .. 6; a null `levels`;
 * a stride below 704 / 128 or a misaligned buffer; `statistics` overlapping an output (state_out, prev_out, log, extremes,
 * tether_peaks) or - since it is written - an input (state, prev, applied, control, mooring, tether, levels); `levels`
 * overlapping an output: HYDRO_E_ARG, and nothing is launched or written.  Asynchronous, no allocation, no synchronisation,
 * safe to capture: a replay accumulates and adds `steps` to n.
 * Cost and registers: DESIGN.md section 30.  New functionality; the reference keeps no statistics. */
typedef struct hydro_statistics_tile {
    double sums[4][HYDRO_TILE];
    uint32_t words[3][HYDRO_TILE];
} hydro_statistics_tile_t;
int hydro_statistics_reset(hydro_t *h, int64_t n, void *statistics, int64_t statistics_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_stat(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                      const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                      float *state_out, int64_t out_tile_stride,
                                      float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double *ke_out_dev,
                                      float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t *rows_written_host,
                                      const float *applied, int64_t applied_tile_stride, int applied_frame,
                                      const float *control, int64_t control_tile_stride,
                                      const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                      float *extremes, int64_t extremes_tile_stride,
                                      const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                      float *tether_peaks, int64_t tether_peaks_tile_stride,
                                      void *statistics, int64_t statistics_tile_stride,
                                      const float *levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                      int64_t step0, void *stream);

/* Sea ensemble: `count` sea spectra ("Sea spectrum", above) in one launch, each over a block of the bodies - the realisations
 * (seeds), headings and currents a design extreme is taken over, stepped together instead of one run after the other.  A single
 * realisation of a few thousand bodies leaves most of the device idle; sixteen of them in one launch cost little more than one.
 *
 * MAPPING: body i belongs to tile i / 64, and tile T steps through member  sea(T) = T / tiles_per_sea,  tiles_per_sea =
 * bodies_per_sea / 64 - so member m has the bodies m * bodies_per_sea .. (m + 1) * bodies_per_sea - 1.  bodies_per_sea is a
 * positive multiple of 64.  A member's block may lie partly or wholly past n (the last one usually does): what is past n is not
 * stepped, as ever.  A launch needs ceil(tiles(n) / tiles_per_sea) members, tiles(n) = ceil(n / 64).
 * WATER AT A BODY is "Sea spectrum"'s, statement for statement, read against the body's member.  So, bit for bit, a body of
 * member m takes the step it takes in hydro_step_fused_tiled_multi_stat under hydro_set_sea_spectrum(member m) - the ensemble
 * changes which table a wavefront reads and nothing else.
 * MEMBERS: every member has its own current U and its own components; all members have the SAME `waves`, 0 .. 64.  At most
 * HYDRO_SEA_ENSEMBLE_MAX = 1024 members.  The device table is count * 3088 B, engine-owned (it grows when a call needs more
 * members than any before, and is freed by hydro_destroy).
 *
 * hydro_set_sea_ensemble: `members` is the caller's array of `count` hydro_sea_spectrum_t (read, with their components, during
 * the call only).  hydro_set_sea_spectrum's validator is applied to every member; the table is copied on the engine's private
 * stream and waited for.  members == NULL clears the ensemble (count and bodies_per_sea are not looked at).  HYDRO_E_ARG for
 * count outside 1 .. HYDRO_SEA_ENSEMBLE_MAX, bodies_per_sea below 64 or not a multiple of 64, members of unequal `waves`, and
 * whatever hydro_set_sea_spectrum refuses of any member - the previous ensemble stays in force.
 * AN ENSEMBLE, A SPECTRUM AND A SEA EXCLUDE EACH OTHER, at set time: each of hydro_set_sea, hydro_set_sea_spectrum and
 * hydro_set_sea_ensemble (non-NULL) returns HYDRO_E_STATE while another kind is set, and its message names the call that clears
 * that kind (an ensemble: hydro_set_sea_ensemble(h, NULL, 0, 0)); what was set stays in force.  Clearing with NULL is always
 * allowed.  ONLY hydro_step_fused_tiled_multi_ens and hydro_sea_ensemble_sample know the ensemble: EVERY OTHER ENTRY IGNORES IT,
 * as every entry but hydro_step_fused_tiled_multi_irr and _stat ignores a spectrum.  (Besides them the two open-loop entries
 * hydro_step_wrench_tiled_irr and hydro_step_wrench_aos_irr know a spectrum, an ensemble and a finite-depth sea: "Irregular sea
 * in the open-loop steps" below.)
 *
 * hydro_sea_ensemble_sample: the signature and the rules of hydro_sea_spectrum_sample, each body read against its member.
 * HYDRO_E_STATE without an ensemble; HYDRO_E_ARG, last, if n needs more members than `count`.
 *
 * hydro_step_fused_tiled_multi_ens: exactly the signature, the refusals and the refusal order of
 * hydro_step_fused_tiled_multi_stat.
 *   no ensemble set : the launch and its bits are those of hydro_step_fused_tiled_multi_stat with the same arguments.
 *   an ensemble set : every other option is still optional and adds what it adds in hydro_step_fused_tiled_multi_stat;
 *                     statistics == NULL gives the family without statistics.  One further refusal comes LAST:
 *                     ceil(tiles(n) / tiles_per_sea) > count returns HYDRO_E_ARG, and nothing is launched or written.
 * Asynchronous, no allocation, no synchronisation, safe to capture under the spectrum's rule: a captured launch replays at a
 * frozen step0 - capture current-only members.
 * COST: with tiles_per_sea a multiple of 4 the four wavefronts of a block read one member, as they read one spectrum; with
 * tiles_per_sea = 1 every wavefront streams its own 3 KB table through the scalar cache.  Measured on an MI355X at 65 536 bodies
 * and 64 components: 16 members of 4 096 bodies cost 0.99 - 1.01 times the single spectrum's step, and 16
 * seeds of 4 096 bodies in one launch 1 / 16 of sixteen launches; SMALL BLOCKS ARE MARKEDLY SLOWER - members of 256 bodies 1.01
 * (nothing but the sea) to 1.17 times (a spread, extremes and statistics), members of 64 bodies 1.11 to 1.42 times.  Guidance, not a
 * rule: give each member as many bodies as the study has, a multiple of 256 bodies.
 * NOT PROVIDED: members with different component counts; a per-body index table (the mapping is by block); ensembles in the
 * open-loop entries (hydro_step_wrench_*_sea) and the plugin.
 * SIGN SYMMETRY: exact, member by member.  Under the mirror in y = 0, the mirror in x = 0 and the half turn about z (DESIGN.md
 * section 21) the image of an ensemble is the image of each member - current and (kx, ky) polar, everything else unchanged - in
 * the members' ORDER and over the same bodies_per_sea: the maps do not renumber bodies.  A launch over the image of a scene then
 * writes the image of what it wrote, by float equality, eta and every scalar the same bits (tests/test_symmetry_gpu.py).
 * New functionality; the reference's water does not move. */
int hydro_set_sea_ensemble(hydro_t *h, const hydro_sea_spectrum_t *members, int64_t count, int64_t bodies_per_sea);
int hydro_sea_ensemble_sample(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int64_t step_index, double dt,
                              float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_ens(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                     const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                     float *state_out, int64_t out_tile_stride,
                                     float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double *ke_out_dev,
                                     float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t *rows_written_host,
                                     const float *applied, int64_t applied_tile_stride, int applied_frame,
                                     const float *control, int64_t control_tile_stride,
                                     const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                     float *extremes, int64_t extremes_tile_stride,
                                     const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                     float *tether_peaks, int64_t tether_peaks_tile_stride,
                                     void *statistics, int64_t statistics_tile_stride,
                                     const float *levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                     int64_t step0, void *stream);

/* Finite-depth sea: the spectra of "Sea ensemble" in water of still-water depth h > 0 (m) - linear (Airy) waves that feel the
 * bottom.  Moorings are a shallow- and intermediate-water business: a Tp = 7 s wave is 76 m long in deep water, and over h = 20 m
 * its kappa h is about 1.7.  There the horizontal orbital velocity at the surface is larger by coth(kappa h), and it does not
 * die off with depth as e^{kappa z}: it goes to a purely horizontal, non-zero motion at the bed - where the lower end of a cable,
 * a bottom-sitting box and an ROV on a tether live.  "Sea spectrum"'s model is unchanged except for the depth profile.
 *
 * WATER AT A BODY of member m (the mapping is "Sea ensemble"'s), component j of wavenumber kappa_j, q_j = e^{-2 kappa_j h}:
 *   eta, tau_j, th_j, r_j, c_j, s_j      exactly "Sea spectrum"'s WATER AT A BODY (the surface does not change)
 *   z_rel = p_z - eta
 *   zc    = max(min(z_rel, 0), -h)       fp32; h rounded once to fp32.  No growth above the surface, nothing below the bed
 *   E_j   = exp2(kl2_j * zc)             as in deep water
 *   G_j   = exp2(fma(-kl2_j, zc, gl_j))  gl_j = -2 kappa_j h log2(e), formed in fp64, rounded once
 *   u_x = fma(cx_j, (E_j + G_j) * c_j, u_x)   u_y likewise with cy_j   u_z = fma(aw_j, (E_j - G_j) * s_j, u_z)
 * CONSTANTS: cx_j, cy_j and aw_j are "Sea spectrum"'s constants times 1 / (1 - q_j), formed in fp64 on the host and rounded once.
 * PROFILES: (E + G) / (1 - q) = cosh(kappa (zc + h)) / sinh(kappa h) and (E - G) / (1 - q) = sinh(kappa (zc + h)) / sinh(kappa h):
 * linear theory, evaluated at the stretched depth z_rel as the deep model is.  u_z = 0 on the bed; below it the water is the bed's.
 * ORDER: the sums run in ascending j, eta from +0 and u from U; the relative state and everything behind the wrench are unchanged.
 * DISPERSION: omega and the wave vector are TAKEN AS GIVEN, as ever.  omega^2 = g kappa tanh(kappa h) is the caller's business
 * (the Python constructors solve it: sea.wavenumber, depth= on pierson_moskowitz / jonswap and their ensembles).
 * CLAMP: the clamp at -h makes zc finite for every p_z, +-inf and NaN included (min and max return the number): a finite table
 * never produces a NaN that the deep model would not.
 * DEEP WATER: where q_j = 0 in fp64 and gl_j - kl2_j zc is below -149 for every body (kappa_j h beyond a few hundred), G_j = +0,
 * the constants are the deep ones and every statement returns "Sea ensemble"'s bits.
 *
 * hydro_set_sea_finite_depth: hydro_set_sea_ensemble's arguments and rules (members, count 1 .. HYDRO_SEA_ENSEMBLE_MAX,
 * bodies_per_sea a positive multiple of 64, equal `waves`, the spectrum's validator on every member, the table engine-owned and
 * of its own, the copy waited for) plus `depth`, ONE depth for all members.  A lone spectrum is an ensemble of one member whose
 * block covers n.  HYDRO_E_ARG also for a depth that is non-finite or <= 0 (or not a positive finite fp32), and for a depth at
 * which a scaled constant or gl_j leaves fp32 range (kappa_j h so small that 1 / (1 - q_j) overflows the component) - the
 * previous table stays in force on every refusal.  members == NULL clears (count, bodies_per_sea and depth are not looked at).
 * IT IS THE FOURTH KIND OF SEA: it and a sea, a spectrum and an ensemble exclude each other at set time - each of the four setters
 * (non-NULL) returns HYDRO_E_STATE while another kind is set, and its message names the call that clears that kind (this one:
 * hydro_set_sea_finite_depth(h, NULL, 0, 0, 0)); what was set stays in force.  ONLY hydro_step_fused_tiled_multi_fd and
 * hydro_sea_finite_depth_sample know it: EVERY OTHER ENTRY IGNORES A FINITE-DEPTH SEA.  (Besides them the two open-loop entries
 * hydro_step_wrench_tiled_irr and hydro_step_wrench_aos_irr: "Irregular sea in the open-loop steps" below.)
 *
 * hydro_sea_finite_depth_sample: the signature and the rules of hydro_sea_ensemble_sample.  HYDRO_E_STATE without a finite-depth
 * sea; HYDRO_E_ARG, last, if n needs more members than `count`.
 *
 * hydro_step_fused_tiled_multi_fd: exactly the signature, the refusals and the refusal order of hydro_step_fused_tiled_multi_ens.
 *   no finite-depth sea set : the launch and its bits are those of hydro_step_fused_tiled_multi_ens with the same arguments.
 *   a finite-depth sea set  : every option stays optional; statistics == NULL gives the family without statistics; the
 *                             ensemble's last refusal (n needs more members than `count`) is read against this table.
 * Asynchronous, no allocation, no synchronisation, safe to capture under the ensemble's rule (capture current-only members).
 * THE SEABED IS INDEPENDENT: h and hydro_set_seabed's z_b know nothing of each other.  Set z_b = -h for a scene whose bodies
 * rest on the bottom the waves feel.
 * COST: one more v_exp_f32 and four more vector instructions per component and body in the second pass (42 for 37); nothing more is
 * loaded.  Measured on an MI355X at 64 components against the ensemble's step on the same bodies: 1.09 times
 * at 4 096 bodies and 1.11 times at 1 048 576 with nothing but the sea, 1.07 and 1.09 times with a spread, extremes and statistics.
 * A run in deep water pays nothing: leave the depth away and the kernels are the ensemble's.
 * NOT MODELLED / NOT PROVIDED: a depth-limited spectral shape (TMA); shoaling, breaking and a sloping bed; depth in the 8-wave
 * hydro_set_sea, in the open-loop entries (hydro_step_wrench_*_sea) and the plugin; members of different depths; any coupling
 * between h and the seabed's z_b.
 * SIGN SYMMETRY: exact at any depth.  h is a scalar and so are kl2_j, gl_j, aw_j times 1 / (1 - q_j), zc, E_j and G_j; cx_j and
 * cy_j times 1 / (1 - q_j) are formed from kx_j and ky_j by products and a division - exact negations under a map that flips
 * them - and the phase keeps its bits.  So the image of a scene (the image of the sea has the same depth)
 * gives the image of its outputs by float equality, eta the same bits (tests/test_symmetry_gpu.py).
 * New functionality; the reference's water does not move. */
int hydro_set_sea_finite_depth(hydro_t *h, const hydro_sea_spectrum_t *members, int64_t count, int64_t bodies_per_sea, double depth);
int hydro_sea_finite_depth_sample(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int64_t step_index, double dt,
                                  float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_fd(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                    const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                    float *state_out, int64_t out_tile_stride,
                                    float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                    int rotational, double *ke_out_dev,
                                    float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                    int64_t row0, int64_t *rows_written_host,
                                    const float *applied, int64_t applied_tile_stride, int applied_frame,
                                    const float *control, int64_t control_tile_stride,
                                    const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                    float *extremes, int64_t extremes_tile_stride,
                                    const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                    float *tether_peaks, int64_t tether_peaks_tile_stride,
                                    void *statistics, int64_t statistics_tile_stride,
                                    const float *levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                    int64_t step0, void *stream);

/* Current profile: a sheared current - the steady current as a PROFILE OVER DEPTH, scene-wide, on top of "Finite-depth sea".
 * A real current is strongest at the surface and close to zero at the bed, and design codes give it as a profile (DNV-RP-C205
 * 4.1: a 1/7 power law over the depth for the tidal part, a wind-driven slab that dies out linearly over the top 50 m, often on
 * another heading).  A cable's bow and a mooring's load below the surface are set by that shear; one vector U over-loads both.
 *
 * THE PROFILE: K = 0 .. HYDRO_CURRENT_KNOTS_MAX knots (z_l, V_l), z_l in m (<= 0, 0 the still-water surface), strictly ascending
 * as fp32 values, V_l a 3-vector in m/s.  Piecewise linear between the knots; V_0 below the lowest, V_{K-1} above the highest.
 * WATER AT A BODY of member m, behind "Finite-depth sea"'s WATER AT A BODY (eta and u_fd are that section's, bit for bit):
 *   zc  = max(min(p_z - eta, 0), -h)                 fp32: "Finite-depth sea"'s statement over again from the same eta - the
 *                                                    profile rides with the instantaneous surface; zc is finite for every p_z
 *   P   = V_0
 *   t_l = min(max((zc - z_l) * inv_l, 0), 1)         l = 0 .. K-2 in ascending order; a subtraction, a product, two clamps
 *   P_i = fma(D_l,i, t_l, P_i)                       i = x, y, z
 *   u_i = u_fd,i + P_i                               one fp32 add per component
 * Branch-free: a segment below the body adds all of D_l, a segment above it adds D_l * +-0.
 * CONSTANTS: inv_l = 1 / (z_{l+1} - z_l) and D_l = V_{l+1} - V_l are formed in fp64 on the host from the fp32 knots and rounded
 * once each.  ROUNDING: every statement above is ONE fp32 operation (the fma one rounding); the sum over the segments telescopes to
 * the knot values only up to these roundings - DESIGN.md section 34 bounds the distance to the exact profile (PROFILE_BOUND).
 * THE MEMBER'S OWN U STAYS: it is inside u_fd, and the profile is added to EVERY member.  The relative state, restore and
 * everything behind the wrench are "Finite-depth sea"'s.
 * SCOPE: the profile takes effect ONLY WHILE THE ENGINE HOLDS A FINITE-DEPTH SEA (a profile is defined over a water column: it
 * needs h).  Deep water is depth = 1e6, where the _fd kernels return the ensemble's bits; a current-only scene is a member with
 * waves = 0.
 *
 * hydro_set_current_profile: the engine copies the knots into a table of its own (synchronous, like hydro_set_sea).  NULL or
 * knots = 0 clears.  Settable whether or not a sea of any kind is set.  HYDRO_E_ARG for knots outside 0 .. HYDRO_CURRENT_KNOTS_MAX,
 * NULL z or v with knots > 0, a non-finite value, a z_l > 0, knots not strictly ascending, an inv_l or a D_l outside fp32 range -
 * the previous profile stays in force on every refusal.  ONLY hydro_step_fused_tiled_multi_shear and hydro_current_profile_sample
 * know it: EVERY EXISTING ENTRY IGNORES A PROFILE - hydro_step_fused_tiled_multi_fd, hydro_step_wrench_tiled_irr,
 * hydro_step_wrench_aos_irr and every *_sample included.
 *
 * hydro_current_profile_sample: the signature and the rules of hydro_sea_finite_depth_sample (HYDRO_E_STATE without a
 * finite-depth sea); it writes [eta, u] with the profile in u.  Without a profile it writes hydro_sea_finite_depth_sample's bits.
 *
 * hydro_step_fused_tiled_multi_shear: exactly the signature, the refusals and the refusal order of hydro_step_fused_tiled_multi_fd.
 *   no profile set                       : the launch and its bits are those of hydro_step_fused_tiled_multi_fd with the same arguments.
 *   a profile and a finite-depth sea set : every option stays optional; the water is the one above.
 *   a profile and NO finite-depth sea    : HYDRO_E_STATE, behind every other refusal; the message names hydro_set_sea_finite_depth.
 *                                          Nothing is launched or written.
 * Asynchronous, no allocation, no synchronisation, safe to capture under the ensemble's rule (capture current-only members; a
 * profile over current-only members is steady, so it replays exactly).
 * COST: per segment and body five vector instructions (a subtraction, a product that carries both clamps, three fmas) behind two
 * scalar loads, 75 at 16 knots; no more registers than the _fd kernels (0 or 1 VGPR), no LDS, no scratch.  Expected before measuring:
 * about 6 per segment, +18 % on a current-only step and +3 % in a full sea of 64 components where the step is issue-bound, less
 * elsewhere.  Measured on an MI355X with 16 knots against the _fd step on the same bodies: 1.15 times
 * current-only and 1.05 times in a full sea at 1 048 576 bodies; 1.44 and 1.04 times at 4 096 bodies, where a step is latency and the
 * 15 dependent trips, each behind its scalar load, show in full (+0.57 us per step).  A run without a profile pays nothing.
 * NOT MODELLED / NOT PROVIDED: a profile in the open-loop entries (hydro_step_wrench_*) and the plugin; in the 8-wave hydro_set_sea
 * and in the deep kinds of sea without a depth (spectrum, ensemble); a profile per member; a profile that varies in time; the
 * Doppler shift of the waves by the current (omega and the wave vector are taken as given, as ever).
 * SIGN SYMMETRY: exact.  The knots' z_l and inv_l are scalars and so is t_l; V_0 and every D_l are polar - D_l is rounded once from
 * a difference of fp32 values, an exact negation under a map that flips the component - and the knots are summed in ascending l on
 * the scene and on its image.  So the image of a scene (the image of the profile has the same z_l) gives the
 * image of its outputs by float equality (tests/test_symmetry_gpu.py).
 * New functionality; the reference's water does not move. */
typedef struct hydro_current_profile {
    int knots;
    const float *z;
    const float *v; /* knots x 3 */
} hydro_current_profile_t;
int hydro_set_current_profile(hydro_t *h, const hydro_current_profile_t *profile);
int hydro_current_profile_sample(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, int64_t step_index, double dt,
                                 float *out, int64_t out_tile_stride, void *stream);
int hydro_step_fused_tiled_multi_shear(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                       const float *prev, int64_t prev_tile_stride, double dt, int steps,
                                       float *state_out, int64_t out_tile_stride,
                                       float *prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                       int rotational, double *ke_out_dev,
                                       float *log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                       int64_t row0, int64_t *rows_written_host,
                                       const float *applied, int64_t applied_tile_stride, int applied_frame,
                                       const float *control, int64_t control_tile_stride,
                                       const float *mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                       float *extremes, int64_t extremes_tile_stride,
                                       const float *tether, int64_t tether_tile_stride, int64_t tether_layers,
                                       float *tether_peaks, int64_t tether_peaks_tile_stride,
                                       void *statistics, int64_t statistics_tile_stride,
                                       const float *levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                       int64_t step0, void *stream);

/* Irregular sea in the open-loop steps: the spectrum, the ensemble and the finite-depth sea for the caller who integrates - a
 * simulator behind the plugin, or an integrator of one's own around hydro_step_wrench_tiled.  Two entries, each with exactly the
 * prototype of its _sea sibling ("Sea state, open loop"), `double time` in front of `stream`:
 *     hydro_step_wrench_tiled_irr = hydro_step_wrench_tiled_sea    hydro_step_wrench_aos_irr = hydro_step_wrench_aos_sea
 * WHICH WATER.  The four kinds of sea exclude each other at set time, so the engine holds at most one, and the step goes through it:
 *   a finite-depth sea : "Finite-depth sea"'s WATER AT A BODY; the bodies of block m step through member m (tile T through
 *                        member T / tiles_per_sea), as in hydro_step_fused_tiled_multi_fd
 *   an ensemble        : "Sea spectrum"'s WATER AT A BODY read against the body's member, as in hydro_step_fused_tiled_multi_ens
 *   a lone spectrum    : "Sea spectrum"'s WATER AT A BODY - in the ensemble's kernels, as an ensemble of one member
 *   an 8-wave sea      : the launch and its bits are those of the _sea sibling with the same arguments
 *   no sea             : the launch and its bits are those of the parent entry (`time` is validated all the same)
 * MODEL.  As in "Sea state, open loop", with ONE change to the stated WATER AT A BODY: t = time, in seconds, an fp64 value taken
 * as given, replaces t = (step0 + k) * dt.  The wrench is that of the state with p_z - eta and v - u and of the previous velocity
 * with pv[0:3] - u: fp32 subtractions with the same u.
 * IDENTITY.  (double)1 * time == time exactly, so hydro_sea_spectrum_sample, hydro_sea_ensemble_sample and
 * hydro_sea_finite_depth_sample with (step_index = 1, dt = time) write exactly the [eta, u] these entries use at time > 0; at
 * time == 0 it is step_index = 0 (with any dt > 0).  A step is therefore, bit for bit, the parent entry on the relative state
 * built from that sample; and one explicit step of hydro_step_fused_tiled_multi_fd at step0 (no option set) is this entry at
 * time = step0 * dt followed by hydro_integrate_tiled of the true state.
 * PREVIOUS VELOCITY.  "Sea state, open loop"'s rule: the engine-owned previous velocity receives the TRUE velocity, never the
 * relative one; with a caller-owned `prev` nothing is written but the wrench.
 * A spectrum with no current and no components (or components of amplitude 0) gives the parent's bits, sign of zero included; a
 * spectrum of up to HYDRO_SEA_WAVES_MAX components gives the bits of the _sea sibling under the same components set with
 * hydro_set_sea; a finite-depth sea in deep water ("DEEP WATER" above) gives the ensemble's.
 * REFUSALS.  HYDRO_E_ARG for a non-finite time, time < 0 or time > 2^52, first; after that the parent's refusals in the parent's
 * order; then, LAST and with an ensemble or a finite-depth sea only, ceil(tiles(n) / tiles_per_sea) > count with the message of
 * hydro_step_fused_tiled_multi_ens (_fd) - all before anything is launched or written.  Asynchronous, no allocation, no
 * synchronisation, safe to capture: a captured launch replays at the frozen `time` it was captured with, and reads the table at
 * replay time with the number of components, the mapping and the depth of the moment it was captured.
 * EVERY EXISTING ENTRY BEHAVES AS BEFORE, the _sea entries included: with a spectrum, an ensemble or a finite-depth sea set they
 * issue the parent's launch.  Kernels of their own beside the _sea kernels (256-thread blocks whatever hydro_set_tuning's
 * block_threads says).
 * NOT COVERED - these step through still water whatever is set: hydro_step_wrench_tiled_ke, hydro_step_wrench_tiled_batch, the
 * plain-SoA hydro_step_wrench[_ext], and the component / calculator entries hydro_step_components[_aos].
 * SIGN SYMMETRY: exact, whichever sea the engine holds, for both entries (hydro_step_wrench_aos_irr in either quaternion order),
 * their _sea siblings and the samples at a time: the image's wrench is the image of the wrench, the engine-owned previous
 * velocity afterwards the image of the scene's, eta the same bits (tests/test_symmetry_gpu.py).
 * Cost and registers: DESIGN.md section 33.  New functionality; the reference's water does not move. */
int hydro_step_wrench_tiled_irr(hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride,
                                const float *prev, int64_t prev_tile_stride, double dt,
                                float *wrench, int64_t wrench_tile_stride, double time, void *stream);
int hydro_step_wrench_aos_irr(hydro_t *h, int64_t n, const float *positions, const float *orientations, int quat_xyzw,
                              const float *velocities, double dt, float *forces, float *torques, double time, void *stream);

/* Kernel-variant selection for tuning: bodies per lane (0 = default, 1, 2), threads per block
 * (0 = chosen by size, 128, 256), streaming accesses - non-temporal loads, write-through stores - (-1 = chosen by size, 0, 1), resident waves per
 * SIMD of the tiled wrench kernel (-1 = chosen by size, 0 = whatever the registers allow, 1..8 = cap,
 * enforced with a dynamic-LDS request: the kernel itself uses no LDS). */
int hydro_set_tuning(hydro_t *h, int bodies_per_lane, int block_threads, int non_temporal, int waves_per_simd);

int   hydro_sync(hydro_t *h);
void *hydro_stream(hydro_t *h);

#ifdef __cplusplus
}
#endif
#endif /* HYDRO_H */
