// pekf_session_recycle.hip -- a phone leaves, the next one starts afresh (pekf_session_recycle_dev): one launch
// that returns a listed set of a session's columns to the state a brand-new session gives them, in a file of its
// own so that the session kernels' objects and listings hold the kernels they held.
//
// The reference serves one client per process and exits (KFS/Server.cpp:58 accepts one connection, :93 ends on
// its disconnect): its "next phone" is a new process, and so a freshly constructed Parser with its members --
// Magnetometer_Calibration (KFS/Magnetometer_Calibration.cpp:7-12), the three InitialValues, the KalmanFilter,
// the flags and counts (KFS/Parser.h:84-104).  A column of a batch has no new process; this kernel writes, per
// listed column, what those constructors leave -- the three session states' fresh forms, each stated by the
// layout's own owner:
//   the filter (LiveState, pekf_live.hpp): every plane zero, so the lane's join mark (kJoined) is clear and
//     k_live<..., JOIN> starts it fresh from X / P; X / P themselves; refs as for a phone that is not ready;
//   phase 2 (InitState, pekf_phase2.hpp): InitState::store of zero sums, counts and flags with both clocks at
//     the new start time -- what k_frontend_init_resume holds before its first row with resume == 0 -- and
//     that kernel's outputs for a phone with no rows;
//   phase 1 (MagcalState, pekf_magcal.hpp): the two header planes zero (sums 0, count 0) and magcal_store's
//     "not calibrated", k_magcal_resume's own statement for resume == 0.  The sample store stays: with a
//     count of 0 no slot is read before it is rewritten.
// Pure data movement, a few hundred bytes per listed column; nothing here is tuned.
#include "pekf_live.hpp"
#include "pekf_magcal.hpp"
#include "pekf_phase2.hpp"

namespace pekf {

constexpr int kRecycleBlock = 256;

// The three optional groups (a null state pointer: the group is not touched; the host has checked that a
// given group is complete) and the per-listed-column inputs and outputs, aligned with cols.
struct RecycleArgs {
    int64_t batch, n_cols;
    const int32_t *cols;
    // the filter
    void *live_state;
    double *X, *P, *refs;
    const double *X0, *P0;
    double *final_X, *final_P;
    // phase 2
    void *init_state;
    int64_t *t_start;
    double *init;
    int64_t *t_init;
    int32_t *ready;
    const int64_t *t_start_new;
    // phase 1
    void *magcal_state;
    double *cal, *fit;
    int32_t *status;
};

// One lane per listed column.  A lane whose index is outside [0, batch) writes nothing.
__global__ __launch_bounds__(kRecycleBlock) void k_session_recycle(RecycleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRecycleBlock + threadIdx.x;
    if (i >= a.n_cols) return;
    const int64_t b = a.cols[i];
    if (b < 0 || b >= a.batch) return;
    const double nan = __builtin_nan("");

    if (a.live_state) {  // uniform, as every test of a group's pointer below
        double *x = a.X + 4 * b, *p = a.P + 16 * b;
        if (a.final_X) {  // the departing phone's last pose, before anything of it is overwritten
#pragma unroll
            for (int k = 0; k < 4; ++k) a.final_X[4 * i + k] = x[k];
#pragma unroll
            for (int k = 0; k < 16; ++k) a.final_P[16 * i + k] = p[k];
        }
#pragma unroll
        for (int pl = 0; pl < LiveState<true>::kPlanes; ++pl)
            *state_plane(a.live_state, a.batch, b, pl) = make_double2(0.0, 0.0);
        if (a.X0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = a.X0[4 * i + k];
#pragma unroll
            for (int k = 0; k < 16; ++k) p[k] = a.P0[16 * i + k];
        } else {  // k_reset's values (pekf_run.hip)
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = k == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) p[k] = (k % 5 == 0) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) a.refs[6 * b + k] = nan;
    }

    if (a.init_state) {
        const int64_t t = a.t_start_new ? a.t_start_new[i] : 0;
        const double sum[3][3] = {};
        const int cnt[3] = {0, 0, 0};
        const bool done[3] = {false, false, false};
        InitState::store(a.init_state, a.batch, b, sum, cnt, done, false, t, t);
        a.t_start[b] = t;
#pragma unroll
        for (int k = 0; k < 6; ++k) a.init[6 * b + k] = nan;
        a.t_init[b] = t;
        a.ready[b] = 0;
    }

    if (a.magcal_state) {
#pragma unroll
        for (int pl = 0; pl < MagcalState::kHeadPlanes; ++pl)
            *state_plane(a.magcal_state, a.batch, b, pl) = make_double2(0.0, 0.0);
        const double w[3][3] = {}, xs[6] = {};
        magcal_store(b, 1, 0.0, 0.0, 0.0, w, xs, a.cal, a.fit, a.status);  // not calibrated: bias 0, W = I, fit NaN
    }
}

}  // namespace pekf

using namespace pekf;

static bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

extern "C" int pekf_session_recycle_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags,
                                        void *live_state, double *X, double *P, double *refs, const double *X0,
                                        const double *P0, double *final_X, double *final_P, void *init_state,
                                        int64_t *t_start, double *init, int64_t *t_init, int32_t *ready,
                                        const int64_t *t_start_new, void *magcal_state, int n_cal, double *cal,
                                        double *fit, int32_t *status, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_cols >= 0, "negative size");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 phones per launch");
    PEKF_CHECK_ARG(aligned16(live_state), "live_state must be a 16-byte aligned pointer");
    PEKF_CHECK_ARG(aligned16(init_state), "init_state must be a 16-byte aligned pointer");
    PEKF_CHECK_ARG(aligned16(magcal_state), "magcal_state must be a 16-byte aligned pointer");
    // a group is given whole or not at all
    const bool any_f = live_state || X || P || refs, all_f = live_state && X && P && refs;
    PEKF_CHECK_ARG(any_f == all_f, "the filter group needs live_state, X, P and refs together");
    const bool any_2 = init_state || t_start || init || t_init || ready;
    PEKF_CHECK_ARG(any_2 == (init_state && t_start && init && t_init && ready),
                   "the phase-2 group needs init_state, t_start, init, t_init and ready together");
    const bool any_1 = magcal_state || cal || fit || status;
    PEKF_CHECK_ARG(any_1 == (magcal_state && cal && fit && status),
                   "the phase-1 group needs magcal_state, cal, fit and status together");
    PEKF_CHECK_ARG(!any_1 || (n_cal >= 6 && n_cal < (1 << 30)),
                   "n_cal must be >= 6 (the fit has 6 unknowns) and < 2^30");
    PEKF_CHECK_ARG(!any_f || flags == PEKF_EV_F64_EVENTS,
                   "the filter group is a joining session's (flags must be PEKF_EV_F64_EVENTS, as pekf_live_join_dev)");
    PEKF_CHECK_ARG((final_X != nullptr) == (final_P != nullptr), "final_X and final_P come together");
    PEKF_CHECK_ARG(!final_X || any_f, "final_X / final_P need the filter group");
    PEKF_CHECK_ARG((X0 != nullptr) == (P0 != nullptr), "X0 and P0 come together");
    PEKF_CHECK_ARG(!X0 || any_f, "X0 / P0 need the filter group");
    PEKF_CHECK_ARG(!t_start_new || any_2, "t_start_new needs the phase-2 group");
    if (n_cols == 0 || batch == 0 || !(any_f || any_2 || any_1)) return PEKF_OK;
    PEKF_CHECK_ARG(cols, "null pointer");
    PEKF_CHECK_ARG(n_cols <= batch, "cols lists distinct columns: n_cols must be <= batch");
    const RecycleArgs a = {batch, n_cols, cols, live_state, X, P, refs, X0, P0, final_X, final_P, init_state,
                           t_start, init, t_init, ready, t_start_new, magcal_state, cal, fit, status};
    hipLaunchKernelGGL(k_session_recycle, dim3(grid_for(n_cols, kRecycleBlock)), dim3(kRecycleBlock), 0,
                       as_stream(stream), a);
    return launched("k_session_recycle");
}
