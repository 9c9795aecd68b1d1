// pekf_live_resume_noise.hip -- pekf_live_resume_dev with per-filter noise (pekf_live_resume_noise_dev): the
// resumable kernels k_live<TE, R64 = true, EV64, TRAJ, RESUME = true, JOIN = false, NOISE = true> (pekf_live.hpp),
// whose lanes read their own {q, r} from a plane double2 [batch] once, before the event loop.  Six kernels, as
// pekf_live_resume.hip's: FP64 records on f32 events with and without time events, and FP64 events, each with
// and without a pose per record -- in a file of their own so that the other live files' objects and listings
// hold the kernels they held, compiled with their flags (Makefile LIVEFLAGS).
#include "pekf_live.hpp"

using namespace pekf;

extern "C" int pekf_live_resume_noise_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                          const int64_t *t_init, double alpha, double *X, double *P,
                                          const double *noise, int32_t *counts, double *refs, uint32_t flags,
                                          void *state, int resume, double *traj, double *traj_dt, int64_t traj_rows,
                                          int *dev_error, void *stream) {
    const LiveCall c = {batch, n_events, ev_planes, init, t_init, alpha, X, P, 0.0, 0.0, counts, refs, flags,
                        traj, traj_dt, traj_rows, as_stream(stream), noise, true};
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
    return traj_rows > 0 ? launch_k_live<true, true, false, true>(c, state, resume != 0)
                         : launch_k_live<false, true, false, true>(c, state, resume != 0);
}
