// pekf_live_rec_noise.hip -- pekf_live_rec.hip's kernels with per-filter noise: k_live<..., TRAJ = true,
// RESUME = true, JOIN, NOISE = true, REC = true> (pekf_live.hpp), the resumable ones on f32 events with and
// without time events and on FP64 events, and the joining one.  Four kernels, launched by pekf_live_rec.hip's two
// entries when they are handed a {q, r} plane -- in a file of their own so that the two objects build side by side,
// compiled with the live files' flags (Makefile LIVEFLAGS).
#include "pekf_live.hpp"

namespace pekf {

int launch_live_rec_noise(const LiveCall &c, void *state, int32_t resume, bool join) {
    return join ? launch_k_live<true, true, true, true, true>(c, state)
                : launch_k_live<true, true, false, true, true>(c, state, resume);
}

}  // namespace pekf
