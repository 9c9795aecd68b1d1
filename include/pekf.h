/*
 * pekf.h -- C ABI of libpekf.so, the MI355X (gfx950) batched quaternion-EKF engine.
 *
 * The reference exposes this path as a pure-Python module API with no FFI
 * (SURVEY.md §8b).  Each entry point below replaces one reference interface; the
 * Python drop-in modules (poseestimationkf_amd/dropin/) bind them with ctypes, exactly
 * as a maintainer would bind them from the reference side.
 * Paths are relative to "/root/reference/Python Kalman Filter/".
 *
 * Conventions
 *   - Plain C types only: int64_t counts, double/float/uint32_t arrays, void* streams.
 *   - Quaternions are [w, x, y, z]; 4x4 / 3x3 / 4x3 matrices are row-major.
 *   - "_dev" entry points take DEVICE pointers and a hipStream_t (as void*, NULL =
 *     the null stream) and only enqueue work.  The other batched entry points take
 *     HOST pointers, stage through a pinned buffer, and return when results are on
 *     the host.  All pointers are caller-owned and contiguous.
 *   - Every entry returns a status (PEKF_OK = 0).  pekf_last_error() gives the
 *     calling thread's message for the last failure.  No exceptions cross the ABI.
 *   - There is no CPU fallback: without a usable gfx950 device every compute entry
 *     returns PEKF_ERR_NODEVICE.
 */
#ifndef PEKF_H
#define PEKF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEKF_ABI_VERSION 1

#define PEKF_OK 0
#define PEKF_ERR_INVALID 1  /* bad argument (null pointer, negative size, ...)          */
#define PEKF_ERR_HIP 2      /* HIP runtime error (message has hipGetErrorString)        */
#define PEKF_ERR_SINGULAR 3 /* S = P + R singular in predict: np.linalg.LinAlgError      */
#define PEKF_ERR_NODEVICE 4 /* no HIP device visible                                     */
#define PEKF_ERR_SVD 5      /* non-finite Wahba matrix B: np.linalg.svd raises LinAlgError  */
                            /* "SVD did not converge" (Wahba.py:14)                         */
#define PEKF_ERR_COMM 6     /* collective library (RCCL) unavailable or failed              */
#define PEKF_ERR_TIMEOUT 7  /* a collective step passed its deadline; the communicator was aborted */

/* Bit 31 of a stream record's dt word: magnetometer sample missing ("Wahba-skip"). */
#define PEKF_MISSING_MAG_BIT 0x80000000u
/* Bits 0-30 of the dt word: the record's dt = T - previousT in ns (ExtendedKalmanFilter.py:62), an
 * integer in [0, 2^31 - 1).  All ones (PEKF_DT_ESCAPE) = the dt is not in the word: it is the float64
 * dt_ext[row][filter] of the window's dt side plane -- any value the reference's float64 T - previousT
 * can take: a pause of 2^31 ns (2.1 s) or more, a negative or a fractional difference. */
#define PEKF_DT_MASK 0x7FFFFFFFu
#define PEKF_DT_ESCAPE 0x7FFFFFFFu

/* pekf_run_dev flags.  Default (0): every operation in FP64, as the reference.
 * PEKF_RUN_MIXED_PRECISION: opt-in; the covariance recursion (P-, S^-1, K, P) in FP32, the
 * quaternion path (RK4, Wahba, R->q, X update) in FP64.  Quaternions stay within ~1e-8 of FP64. */
#define PEKF_RUN_MIXED_PRECISION 0x1u
/* PEKF_RUN_STATE_SOA: X and P are in the coalesced SoA layout of pekf_state_layout_dev (for launches
 * that cover few records, where the state read/write dominates: online serving). */
#define PEKF_RUN_STATE_SOA 0x2u

int pekf_abi_version(void);
const char *pekf_last_error(void);

/* ---------------- device, memory, streams, events (host plumbing, no PyTorch) ---------------- */
int pekf_device_count(int *count);
int pekf_set_device(int device);
int pekf_get_device(int *device);
int pekf_device_name(int device, char *buf, int buflen); /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
int pekf_malloc(void **dptr, size_t bytes);
int pekf_free(void *dptr);
int pekf_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int pekf_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int pekf_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int pekf_memset(void *dst, int value, size_t bytes, void *stream);
int pekf_stream_create(void **stream);
int pekf_stream_destroy(void *stream);
int pekf_stream_sync(void *stream);
int pekf_device_sync(void);
int pekf_event_create(void **event);
int pekf_event_destroy(void *event);
int pekf_event_record(void *event, void *stream);
int pekf_event_sync(void *event);
int pekf_event_elapsed_ms(float *ms, void *start, void *stop);

/* ---------------- per-call operators (batched over n independent items) ----------------
 * One GPU thread per item.  These are the drop-in replacements for the reference's
 * per-timestep methods; at n = 1 they serve main_file.py through the Python shims. */

/* How n = 1 calls of pekf_predict / pekf_correct / pekf_wahba_quaternion (one record of
 * main_file.py:38-45 at a time) reach the GPU:
 *   PEKF_PERCALL_SERVICE (default): a resident one-wave kernel answers requests posted in
 *     coherent pinned host memory (~4 us round trip instead of a launch); it ends by itself
 *     after 5 ms without requests and before pekf_device_sync, and is restarted on demand.
 *   PEKF_PERCALL_LAUNCH: one kernel launch per call (also selected by PEKF_PERCALL=launch).
 * Both run the same device code, so results are identical. */
#define PEKF_PERCALL_SERVICE 0
#define PEKF_PERCALL_LAUNCH 1
int pekf_set_percall_mode(int mode);
int pekf_get_percall_mode(int *mode);

/* KalmanFilter.RungeKutta4(q_0, T, w), ExtendedKalmanFilter.py:25-41.
 * q0[n*4], dt_ns[n] (nanoseconds; dt = dt_ns * 1e-9 as at :32), w[n*3] -> q_out[n*4]. */
int pekf_rk4(int64_t n, const double *q0, const double *dt_ns, const double *w, double *q_out);
int pekf_rk4_dev(int64_t n, const double *q0, const double *dt_ns, const double *w, double *q_out,
                 void *stream);

/* UtilityFunctions.norm(a), UtilityFunctions.py:16-21: sqrt of the sequential sum of squares
 * of each of n vectors of length len: a[n*len] -> out[n]. */
int pekf_norm(int64_t n, int64_t len, const double *a, double *out);

/* KalmanFilter.GetJacobian_A(w) -> 0.5*Omega(w) [n*16], ExtendedKalmanFilter.py:43-48 */
int pekf_jacobian_a(int64_t n, const double *w, double *A);
/* KalmanFilter.GetJacobian_B(q) -> 0.5*Xi(q) [n*12], ExtendedKalmanFilter.py:51-56 */
int pekf_jacobian_b(int64_t n, const double *q, double *Jb);
/* KalmanFilter.Comparator(q1, q2) -> conj(q1) (x) q2 [n*4], ExtendedKalmanFilter.py:16-23 */
int pekf_comparator(int64_t n, const double *q1, const double *q2, double *out);

/* KalmanFilter.Prediction(Gyro, T, X_k, P_k), ExtendedKalmanFilter.py:58-68, minus the
 * previousT bookkeeping (:62,:67), which stays with the caller: dt_ns = T - previousT.
 * gyro[n*3], dt_ns[n], X[n*4], P[n*16], Q[n*9], R[n*16] -> z[n*4], Pm[n*16], K[n*16].
 * Returns PEKF_ERR_SINGULAR if any S = Pm + R is singular (the reference raises
 * np.linalg.LinAlgError from np.linalg.inv, :65).  Singular means what it means to LAPACK: a
 * pivot of the LU factorisation with partial pivoting is exactly zero.  No determinant is formed,
 * so the scale of S does not matter, and K = Pm inv(S) carries an error of eps cond(S). */
int pekf_predict(int64_t n, const double *gyro, const double *dt_ns, const double *X,
                 const double *P, const double *Q, const double *R, double *z, double *Pm,
                 double *K);
int pekf_predict_dev(int64_t n, const double *gyro, const double *dt_ns, const double *X,
                     const double *P, const double *Q, const double *R, double *z, double *Pm,
                     double *K, int32_t *status /* device int32[n]: 1 = S singular; may be NULL */,
                     void *stream);

/* KalmanFilter.Correction(Mag, Acc, z_k, P_k, K_k), ExtendedKalmanFilter.py:70-80, with the
 * filter's Wahba reference vectors acc0/mag0 (Wahba.__init__, Wahba.py:4-6).
 * mag[n*3], acc[n*3], z[n*4], P[n*16], K[n*16], acc0[n*3], mag0[n*3] -> X[n*4], P_out[n*16].
 * Returns PEKF_ERR_SVD if any item's B is non-finite (outputs of that item are NaN). */
int pekf_correct(int64_t n, const double *mag, const double *acc, const double *z,
                 const double *P, const double *K, const double *acc0, const double *mag0,
                 double *X, double *P_out);
int pekf_correct_dev(int64_t n, const double *mag, const double *acc, const double *z,
                     const double *P, const double *K, const double *acc0, const double *mag0,
                     double *X, double *P_out, void *stream);

/* Wahba.getRotation(acc, mag, k_acc, k_mag), Wahba.py:8-17 -> R[n*9] (closed form).
 * Returns PEKF_ERR_SVD if any item's B is non-finite, as np.linalg.svd raises there. */
int pekf_wahba_rotation(int64_t n, const double *acc0, const double *mag0, const double *acc,
                        const double *mag, const double *k_acc, const double *k_mag, double *R);
/* Wahba.getQuarternion(acc, mag, k_acc, k_mag), Wahba.py:49-50 -> q[n*4] */
int pekf_wahba_quaternion(int64_t n, const double *acc0, const double *mag0, const double *acc,
                          const double *mag, const double *k_acc, const double *k_mag, double *q);
/* The two on device pointers: the launch alone, on the caller's stream.  The result is the optimum wherever B is
 * finite, whatever the vectors' lengths (each is brought to unit scale by an exact power of two); a pair counts
 * as parallel (rank-1 B: the shortest arc) only where Gram-Schmidt's remainder is rounding noise, 2^-48 |mag|. */
int pekf_wahba_rotation_dev(int64_t n, const double *acc0, const double *mag0, const double *acc,
                            const double *mag, const double *k_acc, const double *k_mag, double *R,
                            int32_t *status /* device int32[n]: 1 = B not finite; may be NULL */, void *stream);
int pekf_wahba_quaternion_dev(int64_t n, const double *acc0, const double *mag0, const double *acc,
                              const double *mag, const double *k_acc, const double *k_mag, double *q,
                              int32_t *status /* as above */, void *stream);
/* Wahba.RotationMatrix2Quart(M), Wahba.py:19-47 -> q[n*4] (3-branch, strict '>', no trace branch) */
int pekf_rotmat_to_quat(int64_t n, const double *M, double *q);

/* ---------------- fused hot path: the whole main_file.py:38-47 loop on the device ----------------
 * One lane per filter; each lane runs n_steps of Prediction + Correction with X and P in
 * registers.  Step t of the launch reads stream row (step0 + t) % window:
 *   plane_gd : float4 [window][batch] {gyro x, y, z, bits(dt word)}   dt word = dt_ns | flags
 *   plane_am : float4 [window][batch] {acc x, y, z, mag x}
 *   plane_my : float2 [window][batch] {mag y, z}
 * refs[batch*6] = {acc0 xyz, mag0 xyz} (float64; KalmanFilter(T0, mag_0, acc_0), :6-11).
 * X[batch*4], P[batch*16] (row-major, symmetric; the kernel reads the upper triangle) are
 * read at launch start and written at the end.  q, r: setQ/setR scales (:12-15).
 * A record whose dt word has PEKF_MISSING_MAG_BIT set runs Prediction only (X = z, P = P-).
 * A non-finite sample cannot raise per filter inside a batch: that filter's X and P become NaN
 * (the reference raises LinAlgError from np.linalg.svd at that record).
 * traj (optional, NULL to skip): X after every step, [n_steps][batch][4].
 * counts (optional, NULL = all n_steps): filter b applies only its first min(counts[b], n_steps)
 *   records of this launch (ragged logs / front-end output sharing one launch); its traj rows after
 *   that repeat its final X.
 * flags: PEKF_RUN_MIXED_PRECISION and/or PEKF_RUN_STATE_SOA (X[4][batch], P[10][batch]). */
int pekf_run_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                 const void *plane_gd, const void *plane_am, const void *plane_my,
                 const double *refs, double *X, double *P, double q, double r, double *traj,
                 const int32_t *counts, uint32_t flags, void *stream);
/* pekf_run_dev for a window with escaped dt words: dt_ext = the window's dt side plane, float64
 * [window][batch] (read only at rows whose dt word is PEKF_DT_ESCAPE; NULL = no escapes, exactly
 * pekf_run_dev). */
int pekf_run_ext_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                     const void *plane_gd, const void *plane_am, const void *plane_my, const double *dt_ext,
                     const double *refs, double *X, double *P, double q, double r, double *traj,
                     const int32_t *counts, uint32_t flags, void *stream);
/* The same launch over FP64 records, for inputs that are float64 to begin with (recorded logs, which the
 * reference parses into float64, ReadFile.py:14-21): 80 B per filter-record in three
 * filter-minor planes,
 *   plane_gd : double4 [window][batch] {gyro x, y, z, dt_ns} -- dt the float64 T - previousT itself
 *              (ExtendedKalmanFilter.py:62): any pause, clock step or fraction
 *   plane_am : double4 [window][batch] {acc x, y, z, mag x}
 *   plane_my : double2 [window][batch] {mag y, z}
 * Every record is a full record (no missing-magnetometer flag).  refs, X, P, q, r, traj, counts as
 * pekf_run_dev (AoS FP64 state); always the multi-record arithmetic, so a window of f32-representable
 * values gives pekf_run_dev's state (n_steps >= 2) bit for bit.  batch < 2^27 (32-bit lane offsets of
 * the 32 B planes); planes 32 B aligned (my: 16 B). */
int pekf_run_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                       const void *plane_am, const void *plane_my, const double *refs, double *X, double *P,
                       double q, double r, double *traj, const int32_t *counts, void *stream);
/* ---------------- per-filter noise: q and r per filter through the fused kernels ----------------
 * The four entries below are pekf_run_ext_dev, pekf_run_rec64_dev, pekf_live_resume_dev and pekf_live_join_dev
 * with `double q, double r` replaced by `const double *noise`: a plane double2 [batch] of {q, r} in device
 * memory, 16-byte aligned, so filter b runs with Q = noise[2b] I and R = noise[2b + 1] I.  Each lane reads its
 * entry once, before its first record (and its r once more at the launch's end); a filter whose entry is (q, r)
 * gets, bit for bit, what the parent entry gives it with that q and r.  Every other argument, check and status is the parent's; a NULL or misaligned noise with
 * batch > 0 is PEKF_ERR_INVALID before anything is launched.
 *   Precondition, per entry of the plane: r finite and > 0, q finite and >= 0.  The entry cannot look at device
 * memory, so it does not check this.  A filter whose entry breaks it gets NaN in its own X and P and no other
 * filter is touched (nothing in the kernels indexes or loops on these values).
 *   FP64 filter on AoS state only.  The one-record serving kernel, the filter handle (pekf_filter_*), the side
 * outputs and pekf_live_dev / _ext_dev / _traj_dev take one q and one r for the launch. */
/* pekf_run_ext_dev with per-filter noise (dt_ext may be NULL: pekf_run_dev).  flags must be 0:
 * PEKF_RUN_MIXED_PRECISION and PEKF_RUN_STATE_SOA are refused (PEKF_ERR_INVALID).  Always the multi-record
 * arithmetic, also for n_steps == 1 (as pekf_run_rec64_dev), so it equals pekf_run_ext_dev bit for bit for
 * launches of n_steps >= 2. */
int pekf_run_noise_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                       const void *plane_gd, const void *plane_am, const void *plane_my, const double *dt_ext,
                       const double *refs, double *X, double *P, const double *noise, double *traj,
                       const int32_t *counts, uint32_t flags, void *stream);
/* pekf_run_rec64_dev with per-filter noise. */
int pekf_run_rec64_noise_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                             const void *plane_am, const void *plane_my, const double *refs, double *X, double *P,
                             const double *noise, double *traj, const int32_t *counts, void *stream);
/* AoS state (X[batch][4], P[batch][4][4]) <-> SoA state (X[4][batch], P[10][batch] holding
 * P00 P01 P02 P03 P11 P12 P13 P22 P23 P33).  to_soa != 0: AoS -> SoA, else SoA -> AoS. */
int pekf_state_layout_dev(int64_t batch, double *X_aos, double *P_aos, double *X_soa, double *P_soa,
                          int to_soa, void *stream);

/* ---------------- side outputs: what main_file.py plots beside X ----------------
 * Pure-gyro attitude: the RK4 chain of the gyro records alone, same dt as the filter (KFS/KalmanFilter.cpp:149,
 * logged as "q_gyro"; step = ExtendedKalmanFilter.py:25-41).  q_gyro[batch*4] in/out; traj optional. */
int pekf_gyro_chain_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                        const void *plane_gd, double *q_gyro, double *traj, void *stream);
/* pekf_gyro_chain_dev for a window with escaped dt words: dt_ext = the window's dt side plane, float64
 * [window][batch], read at rows whose dt word is PEKF_DT_ESCAPE (NULL = exactly pekf_gyro_chain_dev). */
int pekf_gyro_chain_ext_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                            const double *dt_ext, double *q_gyro, double *traj, void *stream);
/* Pure-Wahba attitude of every record with fixed weights (main_file.py:40: getQuarternion(acc, mag,
 * 0.5, 0.5)), out[n_steps][batch][4], same branch/sign convention as Wahba.RotationMatrix2Quart. */
int pekf_wahba_stream_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                          const void *plane_am, const void *plane_my, const double *refs, double k_acc,
                          double k_mag, double *out, void *stream);
/* The pure-gyro chain and the pure-Wahba stream over FP64 records (pekf_run_rec64_dev's planes: the gd
 * plane double4 {gyro xyz, dt_ns}, am double4 {acc xyz, mag x}, my double2 {mag yz}); the same arithmetic as
 * the two above, dt the float64 itself. */
int pekf_gyro_chain_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                              double *q_gyro, double *traj, void *stream);
int pekf_wahba_stream_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_am,
                                const void *plane_my, const double *refs, double k_acc, double k_mag, double *out,
                                void *stream);
/* UtilityFunctions.Quart2RPY(q), UtilityFunctions.py:3-14: q[n*4] -> rpy[n*3] in degrees. */
int pekf_quat_to_rpy(int64_t n, const double *q, double *rpy);
int pekf_quat_to_rpy_dev(int64_t n, const double *q, double *rpy, void *stream);

/* ---------------- recorded traces: the server's text log -> 40 B records ----------------
 * Host-side ingest (no device work).  Tags / precedence of ReadFile.py:27-45; one record per Acc_1 line
 * (main_file.py:38), dt_ns = T[i+1] - T[i] in float64 (ExtendedKalmanFilter.py:62).
 * pekf_log_scan gives the record count; pekf_log_read fills gyro/acc/mag[n*3] (float), dtw[n],
 * acc0/mag0[3] (double) and t0 (first timestamp; may be NULL); it refuses a log with a dt that is not an
 * integer in [0, 2^31 - 1).  pekf_log_read_ext takes any dt: such a record gets the escape word and its
 * float64 dt in dt_ext[n] (the window's dt side plane; other entries are set to 0); *n_escaped (may be
 * NULL) receives how many records were escaped. */
int pekf_log_scan(const char *path, int64_t *n_records);
int pekf_log_read(const char *path, int64_t n_records, float *gyro, float *acc, float *mag, uint32_t *dtw,
                  double *acc0, double *mag0, double *t0);
int pekf_log_read_ext(const char *path, int64_t n_records, float *gyro, float *acc, float *mag, uint32_t *dtw,
                      double *dt_ext, int64_t *n_escaped, double *acc0, double *mag0, double *t0);
/* The log's records as parsed, float64 (the records of pekf_run_rec64_dev): gyro/acc/mag[n*3], dt_ns[n] =
 * T[i+1] - T[i] (any value), acc0/mag0[3], t0 (may be NULL). */
int pekf_log_read64(const char *path, int64_t n_records, double *gyro, double *acc, double *mag, double *dt_ns,
                    double *acc0, double *mag0, double *t0);
/* The emit side: writes (truncates) path with the lines the server's KalmanFilter writes for one client
 * (KFS/KalmanFilter.cpp WriteTextFile, :335-340): mag_0 / acc_0 (:26-33), the initial q_gyro / X_k /
 * Wahba_quart (:55-67), then per record gyro (:265-277), T (the first record: previousT before it,
 * :136-141), q_gyro (:150-153), Mag_1 / Acc_1 (:279-303), X_k / Wahba_quart (:180-183).  Numbers as
 * std::to_string prints them in the "C" locale ("%f", the integer ns times).  t_ns[n_records + 1] = T0
 * then one time per record; gyro/acc/mag[n*3]; acc0/mag0[3]; q_gyro / x_k / wahba[n*4] may be NULL
 * (written as zeros).  Replaces the server's logging for traces made elsewhere (a batch run's inputs and
 * outputs, synthetic streams); pekf_log_read* and ReadFile.getData read it back. */
int pekf_log_write(const char *path, int64_t n_records, const int64_t *t_ns, const double *gyro, const double *acc,
                   const double *mag, const double *acc0, const double *mag0, const double *q_gyro, const double *x_k,
                   const double *wahba);

/* ---------------- server front-end: raw phone events -> records ----------------
 * Device kernel.  Per filter, the phase-3 state machine of Parser::WriteKalmanFilterMeasurement
 * (KFS/Parser.cpp:148-219), linear interpolation of acc / mag to the gyro time (:259-267),
 * normalisation (:221-228) and the alpha low-pass from a zero state (KFS/KalmanFilter.cpp:16-18,
 * 21-24,279-303) -> records written to plane_gd / plane_am / plane_my rows 0..counts[b]-1
 * ([r_max][batch], the layout pekf_run_dev reads), dt = gyro time - previous record's (initially
 * t_init[b]).  Events: ev_planes float4 [n_events][batch] {x, y, z, bits(word)}, 16 B each, with
 * word = (ns since the filter's previous event, first: since t_init[b]) << 2 | type (0 acc, 1 gyro,
 * 2 mag, 3 a message no sensor takes: skipped in phase 3, a message like any other in phase 2), so gaps
 * must be < 2^30 ns (and a type-3 message's > 0: word 3 is the time event below).  init[batch*6] = raw phase-2 means {acc xyz, mag xyz}
 * (Parser.cpp:44-53); refs[batch*6] receives their normalised values (the filter's acc0 / mag0).
 * A filter whose init is not finite (pekf_frontend_init_dev's "not ready") produces no record (counts 0).
 * *dev_error |= 1 if a record dt does not fit 31 bits, 2 if a filter had more than r_max records. */
int pekf_frontend_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                      const int64_t *t_init, double alpha, int64_t r_max,
                      void *plane_gd, void *plane_am, void *plane_my, int32_t *counts, double *refs,
                      int *dev_error, void *stream);
/* Time events (type 3, PEKF_EV_TIME): an event whose word is exactly 3 carries no sample; its x and y
 * floats are the two halves (low, high) of a float64 time step in ns added to the filter's clock --
 * any gap the 30-bit field cannot hold (a pause of 2^30 ns or more, or a clock that steps back).  The
 * event after it then has its own gap from the new time (usually 0).  A time event with step 0 is a
 * no-op, which pads shorter event streams to the plane's length.  Phase 2 (pekf_frontend_init_dev)
 * always honours them; the phase-3 kernels do with PEKF_EV_TIME_EVENTS in flags (without it a word-3
 * event is skipped and the clock does not move, at no cost to the event loop). */
#define PEKF_EV_TIME 3u
#define PEKF_EV_TIME_EVENTS 0x1u
#define PEKF_EV_F32_RECORDS 0x2u /* pekf_live_ext_dev: records rounded to the f32 stream record format */
/* FP64 events (pekf_live_ext_dev, pekf_frontend_ext_dev, pekf_frontend_init_ext_dev): ev_planes is double4
 * [n_events][batch], 32 B per event, {x, y, z, w} where x, y, z are the sample as the server parses it
 * (std::stod of the phone's text, KFS/Parser.cpp:23-25 -- in general not the f32 the phone measured) and
 * w's bits are those of the event's absolute time in ns as a float64 (an integer, |t| < 2^51) with the
 * type (0 acc, 1 gyro, 2 mag, 3 a message no sensor takes) in its two lowest bits; w = the bits of -0.0
 * with type 3 (0x8000000000000003, which no time packs to) is no message at all, for padding.  t_init /
 * t_start are times on the same clock.  Any gap or clock step is just the next event's time (no time events); records are FP64
 * throughout, their dt any float64.  Host packing: pekf_wire_parse (wire text) or pekf_f32_wire_values
 * (f32 samples -> the doubles the server would parse). */
#define PEKF_EV_F64_EVENTS 0x4u
/* pekf_frontend_dev with time events (flags) and escaped records: a record whose dt does not fit the
 * dt word gets PEKF_DT_ESCAPE and its float64 dt in dt_ext[r_max][batch] (the window's dt side plane for
 * pekf_run_ext_dev; only escaped entries are written), and *dev_error |= 4 says some record was escaped.
 * dt_ext = NULL: such a record sets *dev_error bit 1, as pekf_frontend_dev. */
int pekf_frontend_ext_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                          const int64_t *t_init, double alpha, int64_t r_max, void *plane_gd, void *plane_am,
                          void *plane_my, double *dt_ext, int32_t *counts, double *refs, uint32_t flags,
                          int *dev_error, void *stream);

/* The server's phase 3 with the filter fused in: pekf_frontend_dev's records are not
 * written anywhere -- each is applied to the filter's state on the same lane (Prediction + Correction,
 * main_file.py:42-45) as soon as the wave runs its next filter step.  Same events, init, t_init, alpha
 * and refs as pekf_frontend_dev; X[batch*4], P[batch*16] (AoS, FP64) are the filters' state, read at
 * the start and written at the end (left untouched for a filter with no record, as for one whose init
 * is not finite: phase 2 never got ready); q, r as pekf_run_dev.
 * counts[b] receives the number of records filter b applied.  A record's acc / mag reach the filter as
 * the FP64 low-pass outputs, as the server hands them to its filter (KFS/KalmanFilter.cpp:279-303); with
 * PEKF_EV_F32_RECORDS (pekf_live_ext_dev) they are rounded to f32 first, as in the 40 B stream record,
 * and the final state then equals pekf_frontend_dev followed by pekf_run_dev with those counts, bit for
 * bit.  A record whose dt does not fit the dt word
 * keeps its float64 dt beside it on the lane (as pekf_frontend_ext_dev + pekf_run_ext_dev would), so any
 * gap is applied; dev_error is kept for the ABI and never set by this kernel (no r_max either: there is
 * no record window). */
int pekf_live_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                  const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                  int32_t *counts, double *refs, int *dev_error, void *stream);
/* pekf_live_dev with flags (PEKF_EV_TIME_EVENTS: the planes hold time events; PEKF_EV_F32_RECORDS: f32
 * records, the split pipeline's; PEKF_EV_F64_EVENTS alone: FP64 events, every record field FP64 -- the
 * server's own input values end to end). */
int pekf_live_ext_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                      const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                      int32_t *counts, double *refs, uint32_t flags, int *dev_error, void *stream);
/* pekf_live_ext_dev with a pose per record: what the server does with every phase-3 record --
 * Parser::ExecuteKalmanFilter (KFS/Parser.cpp:248-267) hands it to the filter and the resulting X_k goes to
 * the plotter and into the log's "X_k :" line.  Flags and every check as pekf_live_ext_dev; X, P, counts and
 * refs come out exactly as from it.
 * traj[traj_rows][batch][4] (device, 16-byte aligned, required when traj_rows > 0): row r of filter b is its X
 * after the r-th record it applied in this launch -- the unit, world-basis quaternion, formed as pekf_run_dev's
 * trajectory row and as the launch's final X are, so row counts[b] - 1 equals X[b] bit for bit.  The row index
 * is the filter's own record index, not a time step shared by the batch: filters complete records at different
 * events.  traj_dt[traj_rows][batch] (device, may be NULL): the same record's dt in float64 ns as the filter
 * applied it (the dt word, an escaped record's float64 dt, or an FP64 event's time difference).
 * Nothing else is written: rows >= counts[b], rows >= traj_rows, every row of a filter that is not ready and of
 * a stream without records keep what the caller put there (fill with 0xFF bytes to read them as NaN);
 * counts[b] still reports every record applied, also above traj_rows.  0 <= traj_rows < 2^31;
 * traj_rows == 0 is pekf_live_ext_dev itself (traj and traj_dt are not looked at). */
int pekf_live_traj_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                       const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                       int32_t *counts, double *refs, uint32_t flags, double *traj, double *traj_dt,
                       int64_t traj_rows, int *dev_error, void *stream);

/* A live session fed in chunks: pekf_live_traj_dev on the next n_events rows of the same filters' streams,
 * leaving in `state` what the next call needs to continue -- however a session's events are cut into calls,
 * every output (X, P, refs, the summed counts, the trajectory rows and their dts in order) has the bits of the
 * one call over all of them.  resume == 0 starts a session: the front-end from init / t_init / alpha and the
 * filter from X / P, exactly as pekf_live_ext_dev; resume != 0 continues it from `state`.
 *   What carries over, in `state`: the front-end's half-assembled record (the pending samples, their times and
 * flags), its low-pass outputs and its clocks, and the filter as the kernel's loop holds it (the unnormalised
 * state in the reference pair's basis, the covariance factor, the number of records applied so far).  What does
 * not: the record queue (every launch applies all the records it completes before it ends), and init, t_init,
 * alpha, q, r, which every call of a session must pass unchanged (t_init is read only with resume == 0).
 *   X / P: written at the end of every call for the filters that applied a record in it (the server's X_k of
 * their last record), left alone for the others; counts[b] and the trajectory rows count within the call.  With
 * resume != 0 X and P are NOT read: the state holds the filter, so what the caller writes to X / P between two
 * chunks does not reach it (start a new session, resume == 0, to do that).
 *   state: a device buffer of pekf_live_state_bytes(batch, flags) bytes, 16-byte aligned, required.  Its layout
 * is private and belongs to one event form -- f32 events (flags 0 or PEKF_EV_TIME_EVENTS, which may differ from
 * chunk to chunk) or FP64 events (PEKF_EV_F64_EVENTS) -- and one batch: it is indexed by the filter's number among
 * `batch`, so it cannot be resumed with another batch or the other form, but its bytes may be copied to another
 * buffer or device.  PEKF_EV_F32_RECORDS is refused (PEKF_ERR_INVALID): it exists to equal the one-shot split
 * pipeline.  Every other check is pekf_live_traj_dev's.  n_events == 0 is legal: with resume == 0 it writes the
 * fresh state, with resume != 0 it changes nothing; counts are 0 either way. */
int pekf_live_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                         const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                         int32_t *counts, double *refs, uint32_t flags, void *state, int resume,
                         double *traj, double *traj_dt, int64_t traj_rows, int *dev_error, void *stream);
/* The bytes of a session state for `batch` filters and these flags (host only, no device needed); < 0: flags
 * pekf_live_resume_dev refuses, or a negative batch.  The one entry that returns a size, not a status: 64 bits,
 * int64_t's width on every platform this library builds for, spelled so that the declaration reads
 * `int pekf_...(` at the start of a line like every other entry's (tests/test_capi.py lists the ABI by that). */
long long
int pekf_live_state_bytes(int64_t batch, uint32_t flags);
/* pekf_live_resume_dev for phones that do not move in lock-step: no `resume` word for the launch -- each filter
 * joins the session by itself.  `state` (pekf_live_state_bytes(batch, PEKF_EV_F64_EVENTS) bytes) is zeroed by the
 * caller before the first call; a mark in it says which filters have joined.  Per filter and call:
 *   not joined: it starts fresh exactly as resume == 0 does, from THIS call's init / t_init and from X / P;
 *   joined: it continues from the state exactly as resume != 0 does (X / P and t_init are not used for it).
 * A filter joins at the end of a call in which it was ready (finite init) and its column held at least one
 * message (an event that is not the no-message event).  Until then nothing of it is kept: no-message rows move no
 * state, so its fresh start in the call that holds its first message is the one call over all rows.  The phase-3
 * messages of a filter that is not ready are dropped, and it stays unjoined.  So init / t_init may change from
 * call to call (pekf_frontend_init_resume_dev's outputs of the same chunk) until a filter joins; from then on its
 * init must stay, which phase 2 guarantees (a ready phone's means never change).
 *   FP64 events only: flags must be PEKF_EV_F64_EVENTS, anything else is PEKF_ERR_INVALID.  They carry absolute
 * times; in the f32 planes a phone's first phase-3 gap is relative to its last phase-2 message and padding moves
 * the clock, which a filter that keeps nothing until it joins would lose.  Every other check, and n_events == 0,
 * as pekf_live_resume_dev with resume == 0 (a launch that writes refs and counts = 0). */
int pekf_live_join_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                       const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                       int32_t *counts, double *refs, uint32_t flags, void *state, double *traj, double *traj_dt,
                       int64_t traj_rows, int *dev_error, void *stream);

/* pekf_live_resume_dev and pekf_live_join_dev with per-filter noise (the plane `noise`, its precondition and what
 * a filter that breaks it gets: see pekf_run_noise_dev above).  Like q and r in their parents, the plane must
 * stay what it was for as long as a session lasts: the session state holds a filter's covariance in a form
 * scaled by its r, so a changed r would reinterpret its P.  The one point at which a column's entry may change
 * is pekf_session_recycle_dev, which starts that column's filter afresh: write the new phone's {q, r} before it. */
int pekf_live_resume_noise_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                               const int64_t *t_init, double alpha, double *X, double *P, const double *noise,
                               int32_t *counts, double *refs, uint32_t flags, void *state, int resume,
                               double *traj, double *traj_dt, int64_t traj_rows, int *dev_error, void *stream);
int pekf_live_join_noise_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                             const int64_t *t_init, double alpha, double *X, double *P, const double *noise,
                             int32_t *counts, double *refs, uint32_t flags, void *state, double *traj,
                             double *traj_dt, int64_t traj_rows, int *dev_error, void *stream);

/* pekf_live_resume_dev and pekf_live_join_dev handing out the records they apply: what the server writes into
 * its log beside each X_k (KalmanFilter::WriteTextFile, KFS/KalmanFilter.cpp: the `gyro`, `Acc_1` and `Mag_1`
 * lines and the dt between two `T` lines), per record of Parser::ExecuteKalmanFilter (KFS/Parser.cpp:248-267).
 * The b-th filter's r-th record of the call (r < traj_rows, the row of its pose in traj) is stored in three
 * filter-minor planes of traj_rows rows, exactly pekf_run_rec64_dev's input layout:
 *   rec_gd [traj_rows][batch] double4 {gyro xyz, dt_ns}   (32-byte aligned)
 *   rec_am [traj_rows][batch] double4 {acc xyz, mag x}    (32-byte aligned)
 *   rec_my [traj_rows][batch] double2 {mag y, mag z}      (16-byte aligned)
 * The values are the doubles the filter step was handed: the low-pass acc / mag, the gyro (f32 events: the
 * float32 sample widened) and the dt it was applied with, traj_dt's double (a pause of 2^31 ns or more too).  So
 * pekf_run_rec64_dev with counts over a session's concatenated rows repeats the session, and
 * pekf_gyro_chain_rec64_dev / pekf_wahba_stream_rec64_dev give the log's q_gyro / Wahba_quart lines.  Nothing
 * else is written: rows >= counts[b], every row of a filter that is not ready or has not joined.
 *   noise: NULL -- the launch's q and r, as the parents; otherwise the {q, r} plane of the _noise_dev entries
 * (16-byte aligned; q and r are then ignored).  Records do not depend on the noise.
 *   Refused (PEKF_ERR_INVALID) before any device call: traj_rows == 0 or a null traj / traj_dt (a record comes
 * beside its pose), a null or misaligned record plane, PEKF_EV_F32_RECORDS, and for the join entry any flags but
 * PEKF_EV_F64_EVENTS.  Every other check, batch == 0 and n_events == 0 as the parents'.  Every output the parents
 * write has the bits they give it. */
int pekf_live_resume_rec_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                             const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                             const double *noise, int32_t *counts, double *refs, uint32_t flags, void *state,
                             int resume, double *traj, double *traj_dt, int64_t traj_rows, void *rec_gd,
                             void *rec_am, void *rec_my, int *dev_error, void *stream);
int pekf_live_join_rec_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                           const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                           const double *noise, int32_t *counts, double *refs, uint32_t flags, void *state,
                           double *traj, double *traj_dt, int64_t traj_rows, void *rec_gd, void *rec_am,
                           void *rec_my, int *dev_error, void *stream);

/* Phase 2 of the server's Parser (KFS/Parser.cpp:36-58,84-140; KFS/InitialValues.cpp) on the device: per
 * filter, the mean and sample variance of the first n_avg (the server: 100) samples of each sensor type,
 * and the time phase 3 continues from.  Events as for pekf_frontend_dev (ev_planes [n_events][batch], word
 * = gap << 2 | type, the first gap from t_start[b]).  A filter is ready once every sensor has had a sample
 * after its first n_avg and one more message of any type (3 included) has arrived (the KalmanFilter
 * construction, :41-55); later messages move t_init to their time (:57-62).  Time events and FP64
 * no-message events are not messages.  Outputs (device): init[batch*6] = raw means {acc xyz, mag
 * xyz} and t_init[batch] -- pekf_frontend_dev's init / t_init --, ready[batch] (0: not enough phase-2
 * events; init is then NaN), stats[batch*12] (optional) = {gyro mean, acc / mag / gyro variance};
 * with stats NULL the second pass over the events (the variances) is skipped. */
int pekf_frontend_init_dev(int64_t batch, int64_t n_events, const void *ev_planes, const int64_t *t_start,
                           int n_avg, double *init, int64_t *t_init, double *stats, int32_t *ready, void *stream);
/* pekf_frontend_init_dev with flags: PEKF_EV_F64_EVENTS (FP64 events: the means and variances of the
 * server's own stod values, Parser.cpp:23-25,84-140; times absolute).  PEKF_EV_TIME_EVENTS is accepted
 * and changes nothing (phase 2 always honours time events). */
int pekf_frontend_init_ext_dev(int64_t batch, int64_t n_events, const void *ev_planes, const int64_t *t_start,
                               int n_avg, double *init, int64_t *t_init, double *stats, int32_t *ready,
                               uint32_t flags, void *stream);
/* Phase 2 fed in chunks: pekf_frontend_init_ext_dev's means on the next n_events rows of the same phones' phase-2
 * plane.  resume == 0 starts a session from t_start as the one call does; resume != 0 continues it from `state`
 * (t_start is then not read and may be NULL).  What carries over, in `state`: per phone the three running FP64
 * sums, the three sample counts, the three "initialised" flags, the "filter built" flag and the two clocks.
 *   init, t_init and ready are written by EVERY call and are what pekf_frontend_init_ext_dev with stats = NULL
 * writes for all the rows fed so far, bit for bit, however they were cut into calls: a phone that is not ready
 * has NaN means; a ready phone's means never change again (the sums stop once all three sensors are
 * initialised), only its t_init moves, to each later message's time.
 *   NO VARIANCES: there is no stats argument.  The reference's variance is a second pass over the first n_avg
 * samples once the mean is known (KFS/InitialValues.cpp), and a chunked feed no longer has them; a one-pass
 * formula would not give the reference's bits.  Use pekf_frontend_init_ext_dev on the whole plane for them.
 *   state: a device buffer of pekf_frontend_init_state_bytes(batch, flags) bytes, 16-byte aligned, required; its
 * layout is private and belongs to one batch, its bytes may be copied.  flags as pekf_frontend_init_ext_dev.
 * The no-message / zero-step time events that pad a chunk move nothing.  n_events == 0 is legal: it changes
 * nothing but the outputs (with resume == 0 it writes the fresh state). */
int pekf_frontend_init_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes, const int64_t *t_start,
                                  int n_avg, double *init, int64_t *t_init, int32_t *ready, uint32_t flags,
                                  void *state, int resume, void *stream);
/* The bytes of a phase-2 session state for `batch` phones (host only); < 0: flags the call above refuses, or a
 * negative batch.  64 bits, spelled as pekf_live_state_bytes is. */
long long
int pekf_frontend_init_state_bytes(int64_t batch, uint32_t flags);

/* Phase 1 of the server's client session (KFS/Magnetometer_Calibration.cpp) on the device: per phone, the
 * magnetometer's hard-iron bias and soft-iron matrix W from its phase-1 messages.  Events as for
 * pekf_frontend_init_dev (ev_planes [n_events][batch]; times are not used).  Every message is a sample,
 * whatever its type (KFS/Parser.cpp:30-34,144-147 ignores Type); time events and FP64 no-message events are
 * not messages.  The first n_cal (the server: 100) samples are kept; message n_cal + 1 fires the fit
 * (setValues, :13-43), so a phone with n_cal messages or fewer is not calibrated.  bias = their FP64 sum in
 * arrival order / n_cal (:20-22,32-34; bit for bit the reference's).  With v = m - bias, {a,b,c,d,e,f} is the
 * least-squares solution of [x^2, y^2, z^2, 2xy, 2zx, 2yz] . {a..f} = 1 over those samples (:65-80,159-164;
 * normal equations summed in FP64 from zero, unpivoted Cholesky), R = [[a,d,e],[d,b,f],[e,f,c]] (:165-175) and
 * W = V sqrt(D) V^T, R's principal square root (:178-200; cyclic Jacobi, fixed pair order and sweep count).
 * status[b]: 0 calibrated; 1 n_cal or fewer messages; 2 a Cholesky pivot <= 0 or not finite (the samples do
 * not determine a quadric, e.g. a phone that was never turned); 3 an eigenvalue of R <= 0 or not finite (not
 * an ellipsoid).  For status != 0: bias 0, W = I, fit NaN.
 * cal[batch*12] = {bias xyz, W row-major 3x3 (symmetric, mirrored entries bit-equal)};
 * fit[batch*6] = {a,b,c,d,e,f} (may be NULL); status[batch]; flags: PEKF_EV_F64_EVENTS
 * (PEKF_EV_TIME_EVENTS accepted and honoured always, as phase 2).  n_cal >= 6. */
int pekf_magcal_dev(int64_t batch, int64_t n_events, const void *ev_planes, int n_cal,
                    double *cal, double *fit, int32_t *status, uint32_t flags, void *stream);
/* The correction (the commented body of CorrectValues, :46-55), in place on an event plane of phase 2 or 3:
 * every magnetometer event (type 2) of a phone whose status is 0 becomes W (m - bias); every other event,
 * time events and no-message events, and every column whose status != 0 are not written (bit for bit as they
 * were).  f32 planes: computed in FP64, rounded to f32.  The server corrects the raw sample in phase 2
 * (KFS/Parser.cpp:107) and the interpolated one in phase 3 (:239); the correction is affine, so correcting
 * phase 3's raw samples here equals that in real arithmetic -- within rounding, not bit for bit.
 * status may be NULL (every phone calibrated). */
int pekf_magcal_apply_dev(int64_t batch, int64_t n_events, void *ev_planes, const double *cal,
                          const int32_t *status, uint32_t flags, void *stream);
/* Phase 1 fed in chunks: pekf_magcal_dev on the next n_events rows of the same phones' phase-1 plane, the way
 * the server's Magnetometer_Calibration object takes one message at a time (setValues,
 * KFS/Magnetometer_Calibration.cpp:13-43).  resume == 0 starts a session; resume != 0 continues it from `state`.
 * What carries over, in `state`, is what that object holds (:7-36: x[100] y[100] z[100], bias, num_rows,
 * isCalibrated): per phone the three running FP64 sums, the message count (it stops at n_cal + 1) and the first
 * n_cal samples as doubles, which the fit reads a second time once the bias is known (:65-80).
 *   cal, fit and status belong to the session: pass the same three buffers to every call.  The first call
 * (resume == 0) writes every phone as not calibrated (status 1, bias 0, W = I, fit NaN).  A call rewrites a
 * phone's outputs only if that phone's message n_cal + 1 is among its rows: then its fit runs (status 0, 2 or 3
 * with pekf_magcal_dev's values).  A phone that has fired is never written again, and its later phase-1
 * messages do nothing (:15: isCalibrated).  So after every call cal, fit and status are pekf_magcal_dev's on all
 * the rows fed so far, bit for bit, however they were cut into calls.
 *   n_cal MUST BE THE SAME in every call of a session (the state's size and layout depend on it; it is not
 * checked).  state: a device buffer of pekf_magcal_state_bytes(batch, n_cal, flags) bytes, 16-byte aligned,
 * required; its layout is private and belongs to one batch, its bytes may be copied.  flags and every other
 * argument and check as pekf_magcal_dev; batch < 2^28.  fit may be NULL (then in every call).  The no-message /
 * zero-step time events that pad a chunk move nothing.  n_events == 0 is legal and ev_planes may then be NULL:
 * with resume == 0 it writes the outputs and the fresh state, otherwise it changes nothing. */
int pekf_magcal_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes, int n_cal, double *cal,
                           double *fit, int32_t *status, uint32_t flags, void *state, int resume, void *stream);
/* The bytes of a phase-1 session state for `batch` phones (host only): batch times a per-phone size that is a
 * multiple of 16 -- the sums, the count and n_cal samples of 24 B, the arrays of
 * KFS/Magnetometer_Calibration.cpp:7-12 as doubles.  < 0: a negative batch, n_cal outside [6, 2^30), or flags
 * the call above refuses.  64 bits, spelled as pekf_live_state_bytes is. */
long long
int pekf_magcal_state_bytes(int64_t batch, int n_cal, uint32_t flags);

/* A phone leaves, the next one starts afresh: one launch that returns the listed columns of a chunked session to
 * the state a brand-new session gives them, every other column untouched.  It replaces what the reference does
 * per connection: it serves one client per process (KFS/Server.cpp:58 accepts one, :93 ends on its disconnect), so
 * its next phone gets a newly constructed Parser and its members (KFS/Parser.h:93 and the members around it:
 * Magnetometer_Calibration -- KFS/Magnetometer_Calibration.cpp:7-12 --, the InitialValues, the KalmanFilter, the
 * flags and counts).  A column recycled here and then fed a new phone's rows gives, bit for bit, what a new
 * session fed those rows gives.
 *   cols: n_cols DISTINCT column indices (device int32, any order; n_cols <= batch); one lane per listed column;
 * an index outside [0, batch) writes nothing.  The session's buffers come as three optional groups: a group
 * whose state pointer is NULL is not touched, a group given in part is PEKF_ERR_INVALID.
 *   The filter (live_state, X, P, refs: pekf_live_join_dev's state / X / P / refs; flags must then be
 * PEKF_EV_F64_EVENTS): the column's join mark is cleared (its 16 bytes of every plane of the state are zeroed),
 * so the next pekf_live_join_dev starts it fresh from X / P; X[col] / P[col] (AoS) become X0[i] / P0[i] (device,
 * [n_cols][4] / [n_cols][16], aligned with cols; both or neither) or, without them, pekf_reset_state_dev's
 * [1,0,0,0] and I; refs[col] becomes NaN, a launch's refs for a phone that is not ready.  final_X / final_P
 * (device, [n_cols][4] / [n_cols][16]; both or neither, only with this group): the column's X / P as they were,
 * copied first -- the departing phone's last pose, without a download of every column.
 *   Phase 2 (init_state, t_start, init, t_init, ready: pekf_frontend_init_resume_dev's): the state becomes what
 * that call starts from with resume == 0 -- sums, counts and flags zero, both clocks at t_start_new[i] (device
 * int64 [n_cols]; NULL: 0) -- t_start[col] the same time, and the outputs that call's for a phone with no rows:
 * init NaN, t_init = the start time, ready 0.
 *   Phase 1 (magcal_state, n_cal, cal, fit, status: pekf_magcal_resume_dev's; n_cal in [6, 2^30), the session's;
 * fit is required here): sums and count zero, and the outputs "not calibrated" (status 1, bias 0, W = I, fit
 * NaN), what that call writes for every phone with resume == 0.  The stored samples are left: a count of 0 makes
 * every slot unread until it is rewritten.  This group does not depend on the event form.
 *   batch < 2^28; the three state pointers 16-byte aligned.  n_cols == 0 or batch == 0: PEKF_OK, no launch.
 * The sessions whose filters start from one launch-wide `resume` word (pekf_live_resume_dev) have no per-column
 * fresh start and cannot be recycled. */
int pekf_session_recycle_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags, void *live_state,
                             double *X, double *P, double *refs, const double *X0, const double *P0,
                             double *final_X, double *final_P, void *init_state, int64_t *t_start, double *init,
                             int64_t *t_init, int32_t *ready, const int64_t *t_start_new, void *magcal_state,
                             int n_cal, double *cal, double *fit, int32_t *status, void *stream);

/* A live phone moves: pekf_session_recycle_dev's counterpart.  Where that call writes a listed column's fresh
 * form, these two copy its live form: pekf_session_export_dev gathers the listed columns of a chunked session
 * into one packed buffer, pekf_session_import_dev scatters a packed buffer into the listed columns of a session
 * -- the same one or another, of another batch.  The reference has no counterpart (one client per process,
 * KFS/Server.cpp:58, :93: a phone never changes its place); a batch uses it to gather the survivors of a sparse
 * session into a smaller one, to hand a few phones to another shard, or to fork a phone.  An imported column,
 * fed the phone's next rows, gives bit for bit what the column it came from would have given.
 *   pack: a device buffer of pekf_session_columns_bytes(n_cols, n_cal, flags) bytes, 16-byte aligned.  Its layout
 * is private, as the session states' are: lane-minor planes over the n_cols listed columns, entry i the column
 * cols[i].  Its bytes may be copied as they are, to the host and back or to another device.  Going through it is
 * what makes source and destination independent: nothing is copied in place.
 *   cols, batch and the three optional groups are pekf_session_recycle_dev's (a group whose state pointer is NULL
 * is not touched, a group given in part is PEKF_ERR_INVALID), without that call's per-column inputs:
 *   the filter (live_state, X, P, refs; flags must be PEKF_EV_F64_EVENTS): the column's 16 bytes of every plane
 * of the state -- the join mark among them --, X[col], P[col] (AoS) and refs[col];
 *   phase 2 (init_state, t_start, init, t_init, ready; flags must be PEKF_EV_F64_EVENTS too -- the pack of a
 * joining session has room for both groups, a pack of flags 0 for neither): the state's planes and the four
 * per-column values;
 *   phase 1 (magcal_state, n_cal, cal, fit, status; n_cal in [6, 2^30), the session's AND the pack's; either
 * flags): the two header planes, all n_cal stored samples and the outputs.  Without this group n_cal must be 0.
 *   The checks, their wording and their order are pekf_session_recycle_dev's: no negative size, batch < 2^28, the
 * three states and the pack 16-byte aligned, groups whole, n_cal, flags, n_cols <= batch.  n_cols == 0 or
 * batch == 0: PEKF_OK, no launch.
 *   THE CALLER'S PRECONDITIONS, not checked: cols lists DISTINCT columns inside [0, batch) (one lane per listed
 * column; an index outside reads and writes nothing, two equal ones would write one column twice on import); a
 * pack carries the groups it was exported with, in a layout fixed by (n_cols, n_cal, flags), so an import takes
 * the same n_cols, n_cal and flags and no group the export did not have (those planes were never written).  The
 * noise is not in the pack: the filter's state holds its covariance scaled by the column's r
 * (pekf_live_join_noise_dev), so the destination column must run with the q and r the source column had. */
int pekf_session_export_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags,
                            const void *live_state, const double *X, const double *P, const double *refs,
                            const void *init_state, const int64_t *t_start, const double *init,
                            const int64_t *t_init, const int32_t *ready, const void *magcal_state, int n_cal,
                            const double *cal, const double *fit, const int32_t *status, void *pack, void *stream);
int pekf_session_import_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags, void *live_state,
                            double *X, double *P, double *refs, void *init_state, int64_t *t_start, double *init,
                            int64_t *t_init, int32_t *ready, void *magcal_state, int n_cal, double *cal, double *fit,
                            int32_t *status, const void *pack, void *stream);
/* The bytes of a pack of n_cols columns (host only), a multiple of 16: with flags == PEKF_EV_F64_EVENTS the
 * filter and phase-2 groups of a joining session, with flags == 0 neither; with n_cal != 0 the phase-1 group
 * too (n_cal == 0: none), per column the phase-1 state's own size, ((24 n_cal + 15) & ~15) + 32, and the outputs.
 * < 0: a negative n_cols or one of 2^28 or more, n_cal neither 0 nor in [6, 2^30), any other flags.  64 bits,
 * spelled as pekf_live_state_bytes is. */
long long
int pekf_session_columns_bytes(int64_t n_cols, int n_cal, uint32_t flags);

/* The wire on the device: the clients' 100-byte frames (as MessageSender.java:217-233 sends and Server.cpp:35,84
 * receives them: "#<phase>,<type>:<x>,<y>,<z>,t:<ns>", spaces to 99 characters, '\n') -> FP64 event planes.
 * frames: [n_frames][batch][100] bytes (device; 4-byte aligned), phone b's frames in order along the first
 * axis (a frame not starting with '#' is no message, e.g. padding; a frame is one message whatever it holds,
 * as the server takes each recv -- a newline inside it does not split it; a NUL ends it, as the server's
 * std::string(buf, 0, n) of a char* does (Server.cpp:97), and a frame left with 30 characters or fewer after
 * the '#' is no message, Parser.cpp:14).  Each phase-2 / phase-3 message of phone b
 * becomes the next row of ev2 / ev3 ([e2_max][batch] / [e3_max][batch] double4, PEKF_EV_F64_EVENTS' form;
 * type 3 for a Type no sensor takes); rows after its last message get the no-message event.  n2 / n3[batch]:
 * messages per phase (more than e_max: *dev_error |= 2, the extra ones dropped); first_t2[batch]: the time of
 * the first phase-2 message (t_start of pekf_frontend_init_ext_dev; 0 if none).  Values and times equal
 * pekf_wire_parse's (std::stod / std::stoll) bit for bit for the forms the client prints -- decimals (any
 * of at most 19 significant digits within 1e-80 .. 1e80 of the exponent; an exact big-integer path where
 * one IEEE operation is not exact), "NaN", "Infinity", "-Infinity"; a phone's first frame in another form,
 * or with a time of 2^51 ns or more, stops that phone: bad_frame[b] (may be NULL) = its index (-1: none),
 * *dev_error |= 1 (parse such a stream with pekf_wire_parse).  Messages of any other phase are skipped here;
 * pekf_wire_events_p1_dev keeps the phase-1 messages too (the calibration's, pekf_magcal_dev). */
int pekf_wire_events_dev(int64_t batch, int64_t n_frames, const void *frames, int64_t e2_max, int64_t e3_max,
                         void *ev2, void *ev3, int64_t *first_t2, int32_t *n2, int32_t *n3, int32_t *bad_frame,
                         int *dev_error, void *stream);
/* pekf_wire_events_dev with flags.  PEKF_WIRE_FRAME_ROWS: the planes get a row per frame index instead of
 * a row per message -- row f of ev2 / ev3 holds frame f's message if it is one of that phase, else the
 * no-message event, which phase 2 (pekf_frontend_init_ext_dev) and phase 3 (pekf_live_ext_dev) skip, so
 * they give the same results on n_frames rows as on the compacted planes.  Every lane of a wave then
 * stores the same row: for phones whose rows would drift apart (phase-1 / phase-2 parts of different
 * lengths), at 32 B more written per frame.  Needs e2_max, e3_max >= n_frames; n2 / n3 still count the
 * messages.  A phone's rows from its refused frame on are no-message events.  Where the grid leaves the
 * GPU's SIMDs short of 4 waves, the frames are split into chunks parsed by separate waves (a stream-ordered
 * allocation of 24 B per phone and chunk holds their counts until a second kernel combines them;
 * PEKF_WIRE_CHUNKS=n in the environment forces n chunks).  row_bounds (device, 2 int32, may be NULL; with
 * PEKF_WIRE_FRAME_ROWS only): [0] = 1 + the last row holding a phase-2 message of any phone, [1] = n_frames
 * - the first row holding a phase-3 message of any phone (0: none) -- the rows outside them are no-message
 * rows in every column, which a consumer may leave out (ev2's first [0] rows, ev3 from row n_frames - [1]). */
#define PEKF_WIRE_FRAME_ROWS 0x1u
int pekf_wire_events_ext_dev(int64_t batch, int64_t n_frames, const void *frames, int64_t e2_max, int64_t e3_max,
                             void *ev2, void *ev3, int64_t *first_t2, int32_t *n2, int32_t *n3, int32_t *bad_frame,
                             int *dev_error, int32_t *row_bounds, uint32_t flags, void *stream);
/* pekf_wire_events_ext_dev with a third plane, the phase-1 messages: phase 1 (pekf_magcal_dev) from wire
 * frames with no host parse.  Every message whose phase character is '1' becomes the next row of ev1
 * ([e1_max][batch] double4, PEKF_EV_F64_EVENTS' form; n1[batch] counts them, more than e1_max: *dev_error
 * |= 2), whatever its Type: the server hands every phase-1 sample to the calibration
 * (KFS/Parser.cpp:30-34,144-147), and pekf_magcal_dev takes every message as a sample.  The type bits are
 * those of the other planes ('0'..'2', else 3) and x, y, z the same std::stod values.  The server never reads
 * a phase-1 message's time, but std::stoll must accept it: a time in a form it refuses stops the phone as
 * above, while one of 2^51 ns or more, which the event cannot hold, is stored as 0 -- the message stays a
 * message and counts in n1 (phases 2 and 3 keep their 2^51 refusal).  PEKF_WIRE_FRAME_ROWS: row f of ev1 is
 * frame f's message or the no-message event (needs e1_max >= n_frames too; 32 B more written per frame; the
 * chunks' stream-ordered allocation is the same 24 B).  row_bounds: 3 int32, [2] = 1 + the last row holding a
 * phase-1 message of any phone (pekf_magcal_dev needs ev1's first [2] rows).  ev2, ev3, n2, n3, first_t2,
 * bad_frame and row_bounds[0..1] are pekf_wire_events_ext_dev's, bit for bit. */
int pekf_wire_events_p1_dev(int64_t batch, int64_t n_frames, const void *frames, int64_t e1_max, int64_t e2_max,
                            int64_t e3_max, void *ev1, void *ev2, void *ev3, int64_t *first_t2, int32_t *n1,
                            int32_t *n2, int32_t *n3, int32_t *bad_frame, int *dev_error, int32_t *row_bounds,
                            uint32_t flags, void *stream);

/* A refused frame is its phone's business (the server: one process per client, KFS/Server.cpp:58,93; a frame in
 * a form std::stod reads is parsed like any other, one std::stod / std::stoll throws on ends that client's
 * process alone, since no file of KFS/ has a try).  The two entries below let the host take over exactly the
 * phones pekf_wire_events_*_dev stopped (bad_frame[b] >= 0) and leave every other column alone:
 * pekf_wire_parse_frames reads their frames between the two calls.
 *
 * pekf_wire_gather_frames_dev: the frames [frame0, n_frames) of the n_cols columns listed in cols (device int32)
 * out of frames ([n_frames][batch][100], device, 4-byte aligned) into out ([n_cols][n_frames - frame0][100],
 * device, 4-byte aligned): one download then brings the listed phones' frames, and nobody else's.  A listed
 * column outside [0, batch) gives frames of NULs (no message). */
int pekf_wire_gather_frames_dev(int64_t batch, int64_t n_frames, const void *frames, int64_t n_cols,
                                const int32_t *cols, int64_t frame0, void *out, void *stream);
/* pekf_wire_patch_dev: host-built event cells into the listed columns of the planes, one launch for all of them.
 * cols: n_cols records in HOST memory, which the entry checks before anything is launched, and cols_dev: the same
 * records in device memory (8-byte aligned; the caller's upload, ordered before this call on the stream), which the
 * kernel reads -- the entry itself allocates, copies and waits for nothing: record i names its column, and per plane p (0: ev1, 1: ev2, 2: ev3) the
 * first row it rewrites, from_row[p], and the cells it has for it, n_cells[p].  cells (device, 16-byte aligned;
 * may be NULL if cell_rows == 0): [3][cell_rows][n_cols] double4 in PEKF_EV_F64_EVENTS' form {x, y, z, bits(t) |
 * type} (type 3 for a Type no sensor takes; a phase-1 time the event cannot hold stored as 0, as
 * pekf_wire_events_p1_dev does) -- lane-minor, so adjacent records load adjacent cells, and adjacent columns
 * store adjacent ones.  Column col's row from_row[p] + j of plane p becomes cells[p][j][i] for j < n_cells[p]
 * and the no-message event for every row after those below the plane's e_max; no row at or above e_max, no row
 * below from_row[p] and no column that is not listed is written (n_cells = {0, 0, 0}: the column holds no message
 * from from_row on).  n1 / n2 / n3[col] = n[0..2], first_t2[col] and bad_frame[col] (may be NULL) are set from
 * the record.  ev1 / n1 NULL: no phase-1 plane (pekf_wire_events_ext_dev's planes), plane 0 of the cells unread.
 * row_bounds (device, 3 int32, or NULL): when given, pekf_wire_events_*_dev's row bounds are computed afresh from
 * the patched planes' first n_rows rows, exactly (a second kernel reads every cell's last word): [0], [1] as
 * PEKF_WIRE_FRAME_ROWS states them with n_rows for n_frames, [2] for ev1 (0 without it).
 * PEKF_ERR_INVALID, before any launch: negative sizes, misaligned planes or cells, a column outside [0, batch),
 * a negative from_row or n_cells, n_cells above cell_rows, n_rows above an e_max.  n_cols == 0 without
 * row_bounds: nothing is launched. */
typedef struct {
    int32_t col;          /* the column, in [0, batch) */
    int32_t bad_frame;    /* -1, or the frame that stopped the phone for good */
    int32_t n[3];         /* its messages of phases 1, 2, 3 */
    int32_t from_row[3];  /* per plane: the first row rewritten */
    int32_t n_cells[3];   /* per plane: cells given, rows from_row .. from_row + n_cells - 1 */
    int32_t reserved;     /* 0 */
    int64_t first_t2;     /* the time of its first phase-2 message (0: none) */
} pekf_wire_patch_col;
int pekf_wire_patch_dev(int64_t batch, int64_t n_cols, const pekf_wire_patch_col *cols,
                        const pekf_wire_patch_col *cols_dev, int64_t cell_rows, const void *cells, int64_t e1_max, int64_t e2_max, int64_t e3_max, void *ev1, void *ev2,
                        void *ev3, int64_t *first_t2, int32_t *n1, int32_t *n2, int32_t *n3, int32_t *bad_frame,
                        int64_t n_rows, int32_t *row_bounds, void *stream);

/* ---------------- the phone -> server wire: host code ----------------
 * The Android client sends each sample as text, Float.toString of each value
 * (ASC/MessageSender.java:217-233: "#<phase>,<type>:<x>,<y>,<z>,t:<ns>" padded to 99 characters), and
 * the server parses the values with std::stod (KFS/Parser.cpp:12-26): doubles, in general not the
 * floats the phone measured.  These two functions give the FP64 event planes those doubles.
 * pekf_wire_parse: the server's parse of such text, one message per line (Parser::run keeps messages
 * starting with '#'; ProcessString skips one of 30 characters or fewer after the '#', newline
 * included; a NUL ends the message, as the server's std::string(buf, 0, n) of a char* does).  phase / type: the digits' values; xyz[3n] as strtod (= std::stod) gives them; t_ns as
 * strtoll (= std::stoll).  All four outputs NULL: count only (*n_events).  A message the server's stod /
 * stoll would throw on returns PEKF_ERR_INVALID naming its line. */
int pekf_wire_parse(const char *text, int64_t len, int64_t max_events, uint8_t *phase, uint8_t *type, double *xyz,
                    int64_t *t_ns, int64_t *n_events);
/* The same parse frame by frame, as the server's recv loop takes its input (KFS/Server.cpp:35,84: recv of
 * messageSize = 100 bytes; :97: the message is std::string(buf, 0, n) of a char *buf, cut at the first NUL;
 * Parser::run, KFS/Parser.cpp:357-363: kept if it starts with '#'; ProcessString, :12-26: parsed if more than
 * 30 characters follow).  frames: n_frames x 100 bytes, each one message whatever it holds -- a '\n' inside a
 * frame does not split it, which pekf_wire_parse's lines cannot express.  Per frame, status[f]:
 * PEKF_WIRE_NO_HASH (no '#'), PEKF_WIRE_SHORT (30 characters or fewer after the '#'), PEKF_WIRE_THROWS (the
 * server's std::stod / std::stoll would throw: the reference has no try anywhere, so this frame ends that
 * client's server process) or PEKF_WIRE_MESSAGE (processed), and for a processed frame phase / type (the
 * characters' values - '0', as pekf_wire_parse's), xyz[3 f ..] and t_ns[f]; zeros for any other status.  A
 * frame that throws is reported and the next one read: the call never stops at one. */
#define PEKF_WIRE_FRAME_BYTES 100
#define PEKF_WIRE_NO_HASH 0
#define PEKF_WIRE_SHORT 1
#define PEKF_WIRE_THROWS 2
#define PEKF_WIRE_MESSAGE 3
int pekf_wire_parse_frames(int64_t n_frames, const uint8_t *frames, uint8_t *status, uint8_t *phase, uint8_t *type,
                           double *xyz, int64_t *t_ns);
/* out[i] = the double std::stod makes of Float.toString(in[i]): the shortest decimal that rounds to the
 * float, the closest one among those (JDK 19+ Float.toString; one that needs a single digit prints the
 * closest of one or two digits), read back correctly rounded. */
int pekf_f32_wire_values(int64_t n, const float *in, double *out);

/* X = [1,0,0,0], P = I for every filter (main_file.py:23,26). */
int pekf_reset_state_dev(int64_t batch, double *X, double *P, void *stream);

/* ---------------- filter handle: the batched core of SURVEY.md §8b ----------------
 * One handle = `batch` KalmanFilter objects (ExtendedKalmanFilter.py:6-15): it owns, on the
 * current device, each filter's Wahba reference (acc0, mag0), Q = q I, R = r I, previousT and
 * the state X = [1,0,0,0], P = I (main_file.py:23,26), which stays device-resident between calls.
 * flags: PEKF_RUN_MIXED_PRECISION and/or PEKF_RUN_STATE_SOA (device layout of the state).
 * acc0 / mag0: host [batch*3]; t0_ns: host [batch] initial previousT (NULL = 0). */
typedef struct pekf_filter pekf_filter;
int pekf_filter_create(int64_t batch, const double *acc0, const double *mag0, double q, double r,
                       const int64_t *t0_ns, uint32_t flags, pekf_filter **out);
int pekf_filter_destroy(pekf_filter *f);
/* Host copies of the state in the reference layout: X[batch*4], P[batch*16] (P may be NULL). */
int pekf_filter_set_state(pekf_filter *f, const double *X, const double *P);
int pekf_filter_get_state(pekf_filter *f, double *X, double *P);
/* previousT of every filter (host [batch]); the stream path (pekf_filter_run) uses dt records and
 * leaves it untouched, so set it before switching back to pekf_filter_update. */
int pekf_filter_set_time(pekf_filter *f, const int64_t *t_ns);
/* previousT of every filter (host [batch]; KalmanFilter.previousT, ExtendedKalmanFilter.py:8,67), as the
 * last pekf_filter_update left it (work enqueued by pekf_filter_update_dev on another stream must be
 * synchronised by the caller first, as for pekf_filter_get_state). */
int pekf_filter_get_time(pekf_filter *f, int64_t *t_ns);
/* Device addresses of the state (layout per flags) and refs[batch*6], e.g. for a collective. */
int pekf_filter_device_state(pekf_filter *f, double **X, double **P, double **refs);
/* One record per filter, FP64: Prediction(gyro, t_ns) then Correction(mag, acc) (main_file.py:42-45),
 * dt = t_ns - previousT.  gyro/acc/mag [batch*3], t_ns [batch], mag_missing [batch] (NULL = none
 * missing; nonzero = Wahba-skip), X_out [batch*4] (NULL to skip).  Host pointers, synchronous. */
int pekf_filter_update(pekf_filter *f, const double *gyro, const int64_t *t_ns, const double *acc,
                       const double *mag, const uint8_t *mag_missing, double *X_out);
/* Same with device pointers, enqueued on `stream`. */
int pekf_filter_update_dev(pekf_filter *f, const double *gyro, const int64_t *t_ns, const double *acc,
                           const double *mag, const uint8_t *mag_missing, double *X_out, void *stream);
/* pekf_run_dev on the handle's state and references (stream planes, traj, counts as there). */
int pekf_filter_run(pekf_filter *f, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                    const void *plane_am, const void *plane_my, double *traj, const int32_t *counts,
                    void *stream);
/* pekf_run_ext_dev on the handle (dt_ext: the window's dt side plane, NULL = none). */
int pekf_filter_run_ext(pekf_filter *f, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                        const void *plane_am, const void *plane_my, const double *dt_ext, double *traj,
                        const int32_t *counts, void *stream);

/* ---------------- synthetic IMU streams (device mirror of poseestimationkf_amd/synth.py) --------
 * Filters first_filter .. first_filter+batch-1, window steps, bit-identical to the host
 * generator.  scales[5] = sqrt(3)*sigma for {ref, w, gyro, acc, mag}; ar_w = AR(1) factor.
 * Writes the three planes ([window][batch]) and refs[batch*6]. */
int pekf_synth_dev(int64_t batch, int64_t window, int64_t first_filter, uint32_t seed,
                   int missing_mag, const double *scales, double ar_w, void *plane_gd,
                   void *plane_am, void *plane_my, double *refs, void *stream);

/* ---------------- sharding over GPUs: the one collective of the path ----------------
 * Filters are independent (ExtendedKalmanFilter.py:6-80 shares nothing between KalmanFilter objects),
 * so each GPU runs its own contiguous shard of the batch with no per-record exchange; the final
 * quaternions are gathered to the root by ONE RCCL gather over xGMI (ncclGather, rccl.h:745).
 * RCCL is loaded on first use (librccl.so.1; the copy already in the process if there is one).
 * Every collective call below must be made by all ranks of the communicator; PEKF_ERR_COMM reports
 * an RCCL failure or a missing librccl.
 *
 * One process per GPU: rank 0 makes an id, every rank receives it out of band (any channel:
 * a file, a TCP store, MPI) and calls pekf_comm_init on its current device.
 * One process for several GPUs: pekf_comm_init_all (ncclCommInitAll, rccl.h:236) gives one
 * communicator per device, driven from one host thread with pekf_gather_multi_dev. */
#define PEKF_COMM_ID_BYTES 128
typedef struct pekf_comm pekf_comm;
int pekf_comm_version(int *version); /* RCCL's version code, e.g. 22707 */
int pekf_comm_unique_id(void *id /* PEKF_COMM_ID_BYTES */);
/* Communicator creation has a deadline: ncclCommInitRank (rccl.h) runs on a helper thread and the call
 * waits for it at most PEKF_COMM_TIMEOUT_S seconds (environment; default 300).  If the other ranks do not
 * all join by then it returns PEKF_ERR_TIMEOUT, so a rank that died before joining fails the job instead
 * of hanging it.  The abandoned helper stays blocked inside RCCL until the process exits: after an init
 * timeout the PROCESS MUST EXIT (without its exit handlers, e.g. _exit); until then every later
 * pekf_comm_init* call fails at once with PEKF_ERR_COMM rather than reuse RCCL's bootstrap state.
 * (RCCL 2.27's non-blocking ncclCommInitRankConfig still blocks the caller while a rank is missing.) */
int pekf_comm_init(const void *id, int nranks, int rank, pekf_comm **out);
/* The same with an explicit deadline in seconds (<= 0: wait forever, the blocking behaviour). */
int pekf_comm_init_timeout(const void *id, int nranks, int rank, double timeout_s, pekf_comm **out);
/* devices: ndev device indices (NULL = 0 .. ndev-1); out: ndev communicators, rank i on devices[i].
 * ncclCommInitAll (rccl.h:236) under the same PEKF_COMM_TIMEOUT_S deadline and rules as pekf_comm_init. */
int pekf_comm_init_all(int ndev, const int *devices, pekf_comm **out);
/* The same with an explicit deadline in seconds (<= 0: none). */
int pekf_comm_init_all_timeout(int ndev, const int *devices, double timeout_s, pekf_comm **out);
int pekf_comm_destroy(pekf_comm *c);
/* Abort a communicator (ncclCommAbort: its kernels in flight give up) and free it; for error paths. */
int pekf_comm_abort(pekf_comm *c);
/* Wait until `stream` has drained everything enqueued on it, collectives of c included, watching c for
 * asynchronous RCCL errors meanwhile.  The deadline timeout_s (<= 0: none) applies to each collective of c
 * enqueued on `stream` (pekf_gather_dev, pekf_gather_multi_dev, pekf_allreduce_max_dev) and starts when the
 * stream reaches it -- the work queued before it has finished -- so compute ahead of a collective, however
 * long, is never charged to it.  On expiry or error c is aborted (it must then only be destroyed) and
 * PEKF_ERR_TIMEOUT / PEKF_ERR_COMM returned: a peer that died turns into an error here instead of a host
 * thread stuck in hipStreamSynchronize.
 * The clock starts when THIS rank's inputs are ready, so it also runs while slower peers finish the compute
 * queued ahead of the collective on their side: the deadline must exceed the ranks' skew at the
 * collective (bench.py's final gather follows the whole timed run; size PEKF_COMM_TIMEOUT_S to the run).
 * Every collective is tracked: at most 1,024 incomplete ones per communicator, one more is refused with
 * PEKF_ERR_COMM and not enqueued.  If a collective could not be tracked after it was enqueued (its
 * completion event could not be recorded), the drain of that stream is bounded by timeout_s from the
 * wait call instead, compute included. */
int pekf_comm_wait(pekf_comm *c, void *stream, double timeout_s);
int pekf_comm_rank(const pekf_comm *c, int *rank, int *nranks, int *device); /* outputs may be NULL */
/* recv[nranks * count] on the root (rows in rank order) <- every rank's send[count]; device
 * pointers, enqueued on stream.  recv is ignored (may be NULL) on the other ranks. */
int pekf_gather_dev(pekf_comm *c, const double *send, int64_t count, double *recv, int root, void *stream);
/* The same gather for the ndev communicators of pekf_comm_init_all, as one RCCL group:
 * send[i] / streams[i] belong to comms[i]'s device; recv is on comms[root]'s device. */
int pekf_gather_multi_dev(int ndev, pekf_comm *const *comms, const double *const *send, int64_t count,
                          double *recv, int root, void *const *streams);
/* buf[count] <- elementwise max over the ranks (in place), e.g. the slowest rank's wall time. */
int pekf_allreduce_max_dev(pekf_comm *c, double *buf, int64_t count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEKF_H */
