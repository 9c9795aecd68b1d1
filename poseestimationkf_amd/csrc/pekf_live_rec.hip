// pekf_live_rec.hip -- a chunked session that hands out its records (pekf_live_resume_rec_dev,
// pekf_live_join_rec_dev): the kernels k_live<..., TRAJ = true, RESUME = true, JOIN, NOISE, REC = true>
// (pekf_live.hpp), which store each record they apply -- the doubles handed to the filter step -- beside its pose,
// in pekf_run_rec64_dev's planes: the server's log per chunk (KalmanFilter::WriteTextFile's gyro / Acc_1 / Mag_1
// lines and the dt between its T lines).  Four kernels here, with the launch's q and r: the resumable ones on f32
// events with and without time events and on FP64 events, and the joining one; their four per-filter-noise forms
// are pekf_live_rec_noise.hip's -- files of their own so that the other live files' objects and listings hold the
// kernels they held, compiled with their flags (Makefile LIVEFLAGS).
#include "pekf_live.hpp"

using namespace pekf;

// what the two entries check beyond their twins without records: a pose per record, and the three planes
static int check_live_rec(const LiveCall &c) {
    PEKF_CHECK_ARG(c.traj_rows > 0 && c.traj && c.traj_dt,
                   "records come beside the poses: traj_rows must be > 0, traj and traj_dt non-null");
    PEKF_CHECK_ARG(c.rec_gd && c.rec_am && c.rec_my, "null record plane");
    PEKF_CHECK_ARG((uintptr_t)c.rec_gd % 32 == 0 && (uintptr_t)c.rec_am % 32 == 0 && (uintptr_t)c.rec_my % 16 == 0,
                   "misaligned record planes (rec_gd / rec_am 32 bytes, rec_my 16)");
    return PEKF_OK;
}

static LiveCall rec_call(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                         const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                         const double *noise, int32_t *counts, double *refs, uint32_t flags, double *traj,
                         double *traj_dt, int64_t traj_rows, void *rec_gd, void *rec_am, void *rec_my, void *stream) {
    LiveCall c = {batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, flags,
                  traj, traj_dt, traj_rows, as_stream(stream), noise, noise != nullptr};
    c.rec_gd = rec_gd;
    c.rec_am = rec_am;
    c.rec_my = rec_my;
    return c;
}

extern "C" int pekf_live_resume_rec_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                        const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                        const double *noise, int32_t *counts, double *refs, uint32_t flags,
                                        void *state, int resume, double *traj, double *traj_dt, int64_t traj_rows,
                                        void *rec_gd, void *rec_am, void *rec_my, int *dev_error, void *stream) {
    const LiveCall c = rec_call(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, noise, counts, refs,
                                flags, traj, traj_dt, traj_rows, rec_gd, rec_am, rec_my, stream);
    if (int st = check_live_flags(c)) return st;
    PEKF_CHECK_ARG((flags & PEKF_EV_F32_RECORDS) == 0,
                   "a resumable launch takes FP64 records (PEKF_EV_F32_RECORDS is the one-shot split pipeline's)");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (int st = check_live_rec(c)) return st;
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(c)) return st;
    (void)dev_error;
    if (resume && n_events == 0) {  // nothing to continue with: the state, X and P stay, no record is counted
        PEKF_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)batch, c.stream));
        return PEKF_OK;
    }
    return noise ? launch_live_rec_noise(c, state, resume != 0, false)
                 : launch_k_live<true, true, false, false, true>(c, state, resume != 0);
}

extern "C" int pekf_live_join_rec_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                      const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                      const double *noise, int32_t *counts, double *refs, uint32_t flags, void *state,
                                      double *traj, double *traj_dt, int64_t traj_rows, void *rec_gd, void *rec_am,
                                      void *rec_my, int *dev_error, void *stream) {
    const LiveCall c = rec_call(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, noise, counts, refs,
                                flags, traj, traj_dt, traj_rows, rec_gd, rec_am, rec_my, stream);
    if (int st = check_live_flags(c)) return st;
    PEKF_CHECK_ARG(flags == PEKF_EV_F64_EVENTS,
                   "filters join a session of FP64 events only (flags must be PEKF_EV_F64_EVENTS: absolute times)");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (int st = check_live_rec(c)) return st;
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(c)) return st;
    (void)dev_error;
    return noise ? launch_live_rec_noise(c, state, 0, true) : launch_k_live<true, true, true, false, true>(c, state);
}
