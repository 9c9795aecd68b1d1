// pekf_live_join_noise.hip -- pekf_live_join_dev with per-filter noise (pekf_live_join_noise_dev): the kernels
// k_live<false, false, EV64 = true, TRAJ, RESUME = true, JOIN = true, NOISE = true> (pekf_live.hpp), with and
// without a pose per record, whose lanes read their own {q, r} from a plane double2 [batch] once, before the
// event loop -- in a file of their own so that the other live files' objects and listings hold the kernels they
// held, compiled with their flags (Makefile LIVEFLAGS).
#include "pekf_live.hpp"

using namespace pekf;

extern "C" int pekf_live_join_noise_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                        const int64_t *t_init, double alpha, double *X, double *P, const double *noise,
                                        int32_t *counts, double *refs, uint32_t flags, void *state, double *traj,
                                        double *traj_dt, int64_t traj_rows, int *dev_error, void *stream) {
    const LiveCall c = {batch, n_events, ev_planes, init, t_init, alpha, X, P, 0.0, 0.0, counts, refs, flags,
                        traj, traj_dt, traj_rows, as_stream(stream), noise, true};
    if (int st = check_live_flags(c)) return st;
    PEKF_CHECK_ARG(flags == PEKF_EV_F64_EVENTS,
                   "filters join a session of FP64 events only (flags must be PEKF_EV_F64_EVENTS: absolute times)");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(c)) return st;
    (void)dev_error;
    return traj_rows > 0 ? launch_k_live<true, true, true, true>(c, state)
                         : launch_k_live<false, true, true, true>(c, state);
}
