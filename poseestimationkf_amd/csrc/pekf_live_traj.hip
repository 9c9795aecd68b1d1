// pekf_live_traj.hip -- the fused front-end + filter kernels with a pose per record (pekf_live_traj_dev with
// traj_rows > 0): k_live<TE, R64, EV64, TRAJ = true> (pekf_live.hpp), the TRAJ twins of pekf_live.hip's five
// kernels, in a file of their own so that pekf_live.hip's object and listing hold the kernels they held.
#include "pekf_live.hpp"

namespace pekf {

int launch_live_traj(int64_t batch, int64_t n_events, const void *ev_planes, const double *init, const int64_t *t_init,
                     double alpha, double *X, double *P, double q, double r, int32_t *counts, double *refs,
                     uint32_t flags, double *traj, double *traj_dt, int32_t traj_rows, hipStream_t stream) {
    return launch_k_live<true>(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, flags, traj,
                               traj_dt, traj_rows, stream);
}

}  // namespace pekf
