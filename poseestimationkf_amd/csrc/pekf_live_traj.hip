// pekf_live_traj.hip -- the fused front-end + filter kernels with a pose per record (pekf_live_traj_dev with
// traj_rows > 0): k_live<TE, R64, EV64, TRAJ = true> (pekf_live.hpp), the TRAJ twins of pekf_live.hip's five
// kernels, in a file of their own so that pekf_live.hip's object and listing hold the kernels they held.
#include "pekf_live.hpp"

namespace pekf {

int launch_live_traj(const LiveCall &c) { return launch_k_live<true>(c); }

}  // namespace pekf
