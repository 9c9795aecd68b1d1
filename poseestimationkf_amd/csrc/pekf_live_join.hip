// pekf_live_join.hip -- a live session whose filters join one by one (pekf_live_join_dev): the kernels
// k_live<false, false, EV64 = true, TRAJ, RESUME = true, JOIN = true> (pekf_live.hpp), with and without a pose
// per record, in a file of their own so that the one-shot and the resumable kernels' objects and listings hold
// the kernels they held.  Phones do not move in lock-step: in one chunk some are still in phase 2, some get
// ready, some are already filtering, so one `resume` word for the launch (pekf_live_resume_dev) does not do.
// FP64 events only: they carry absolute times, so a lane that keeps nothing until it joins loses no clock.
#include "pekf_live.hpp"

using namespace pekf;

template <bool TRAJ>
static int launch_k_live_join(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                              const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                              int32_t *counts, double *refs, double *traj, double *traj_dt, int32_t traj_rows,
                              void *state, hipStream_t stream) {
    const dim3 grid(grid_for(batch, kRunBlock)), block(kRunBlock);
    hipLaunchKernelGGL((k_live<false, false, true, TRAJ, true, true>), grid, block, 0, stream, batch, n_events,
                       static_cast<const double4 *>(ev_planes), init, t_init, alpha, q, r, X, P, counts, refs, traj,
                       traj_dt, traj_rows, state, 0);
    return launched("k_live (joining)");
}

extern "C" int pekf_live_join_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                  const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                  int32_t *counts, double *refs, uint32_t flags, void *state, double *traj,
                                  double *traj_dt, int64_t traj_rows, int *dev_error, void *stream) {
    if (int st = check_live_flags(batch, n_events, flags, traj, traj_dt, traj_rows)) return st;
    PEKF_CHECK_ARG(flags == PEKF_EV_F64_EVENTS,
                   "filters join a session of FP64 events only (flags must be PEKF_EV_F64_EVENTS: absolute times)");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(batch, n_events, ev_planes, init, t_init, X, P, r, counts, refs)) return st;
    (void)dev_error;
    if (traj_rows > 0)
        return launch_k_live_join<true>(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, traj,
                                        traj_dt, (int32_t)traj_rows, state, as_stream(stream));
    return launch_k_live_join<false>(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, nullptr,
                                     nullptr, 0, state, as_stream(stream));
}
