// pekf_live_resume.hip -- a live session fed in chunks (pekf_live_resume_dev, pekf_live_state_bytes): the
// resumable kernels k_live<TE, R64 = true, EV64, TRAJ, RESUME = true> (pekf_live.hpp), which leave their lane's
// session state in a device buffer after the event loop and pick it up before the next launch's, in a file of
// their own so that pekf_live.hip's and pekf_live_traj.hip's objects and listings hold the kernels they held.
// Six kernels: FP64 records on f32 events with and without time events, and FP64 events, each with and
// without a pose per record.  The state does not depend on PEKF_EV_TIME_EVENTS, so one chunk's planes may
// hold time events and the next chunk's none: each launch takes the kernel its own flag names.
#include "pekf_live.hpp"

using namespace pekf;

// the flags a session state exists for: none, PEKF_EV_TIME_EVENTS (the same state) or PEKF_EV_F64_EVENTS alone
static bool resume_flags_ok(uint32_t flags) {
    return flags == 0 || flags == PEKF_EV_TIME_EVENTS || flags == PEKF_EV_F64_EVENTS;
}

static_assert(sizeof(long long) == sizeof(int64_t), "pekf_live_state_bytes returns 64 bits");
extern "C" long long int pekf_live_state_bytes(int64_t batch, uint32_t flags) {
    if (batch < 0 || !resume_flags_ok(flags)) return -1;
    return batch * ((flags & PEKF_EV_F64_EVENTS) ? LiveState<true>::kBytes : LiveState<false>::kBytes);
}

extern "C" int pekf_live_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                    const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                    int32_t *counts, double *refs, uint32_t flags, void *state, int resume,
                                    double *traj, double *traj_dt, int64_t traj_rows, int *dev_error, void *stream) {
    const LiveCall c = {batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, flags,
                        traj, traj_dt, traj_rows, as_stream(stream)};
    if (int st = check_live_flags(c)) return st;
    PEKF_CHECK_ARG((flags & PEKF_EV_F32_RECORDS) == 0,
                   "a resumable launch takes FP64 records (PEKF_EV_F32_RECORDS is the one-shot split pipeline's)");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(c)) return st;
    (void)dev_error;
    if (resume && n_events == 0) {  // nothing to continue with: the state, X and P stay, no record is counted
        PEKF_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)batch, c.stream));
        return PEKF_OK;
    }
    return traj_rows > 0 ? launch_k_live<true, true>(c, state, resume != 0)
                         : launch_k_live<false, true>(c, state, resume != 0);
}
