// pekf_phase2.hpp -- phase 2 of the server's Parser, what its two kernels share: k_frontend_init
// (pekf_frontend.hip: one launch over a phone's whole phase-2 stream, means and variances) and
// k_frontend_init_resume (pekf_frontend_resume.hip: the same stream fed in chunks, the means alone).  Their
// block, ring depth and load form and the argument checks of their entries are stated here once.  So is InitState,
// the chunked kernel's per-phone state between two launches: k_session_recycle (pekf_session_recycle.hip) writes
// its fresh form for a column whose phone has left.
//
// Phase 2 (ProcessString, Parser.cpp:36-58; initialMeanAndCovariance, :84-140; InitialValues.cpp): the first
// n_avg samples of each sensor type are averaged (a sequential FP64 sum divided by n_avg).  A sensor counts as
// initialised at its first sample after those n_avg; the first event after all three are initialised builds
// the KalmanFilter (T0 = its time, acc_0 / mag_0 = the raw means at that time), and every later phase-2 event
// moves the acc_0 / mag_0 time and previousT to its own (setAcc0 / setMag0, UpdateLatestPreviousTime).  So
// phase 3 starts from init = {mean acc, mean mag} at t_init = the last phase-2 event's time -- exactly the
// inputs of pekf_frontend_dev.
// Every message counts, whatever its sensor type: one no sensor takes (type 3) adds no sample but, once
// all three are initialised, builds the filter or moves its time as any other (Parser.cpp:36-62).
// FP64 events (the server's stod doubles are what it averages, Parser.cpp:23-25,84-140) carry absolute times,
// and their no-message event (padding, ev64_none) is skipped; an f32 time event moves the clock alone.
//
// The first pass over the events -- this state machine -- is written out in both kernels, the same statements.
// As one function over the kernels' locals (by reference: in one struct they go to scratch) it left every
// kernel at 0 scratch, 0 LDS and its waves per SIMD, and k_frontend_init_resume as fast as it was, but
// k_frontend_init on f32 events 2.3-2.4 % slower, same-box A B B A (profiles/r18/session_fold/README.md).
#pragma once
#include "pekf_phase3.hpp"

namespace pekf {

constexpr int kInitBlock = 256;  // lanes per block of both phase-2 kernels
constexpr int kInitRing = 8;     // event rows loaded at a time (pekf_phase3.hpp: load_event_block)
// Non-temporal event loads (every event is read once per pass): the means -5 % (profiles/r4/ntload/).
#ifndef PEKF_INIT_NTL
#define PEKF_INIT_NTL 1
#endif

// the flags phase 2 takes (it always honours time events)
static inline bool init_flags_ok(uint32_t flags) { return (flags & ~(PEKF_EV_TIME_EVENTS | PEKF_EV_F64_EVENTS)) == 0; }

// The argument checks pekf_frontend_init_ext_dev and pekf_frontend_init_resume_dev share: the sizes and flags,
// then, for a batch that launches, the pointers both read or write.  Each entry adds its own (t_start, stats /
// state, resume) and returns PEKF_OK itself for batch == 0.
static inline int check_init_args(int64_t batch, int64_t n_events, int n_avg, uint32_t flags, const void *ev_planes,
                                  const double *init, const int64_t *t_init, const int32_t *ready) {
    PEKF_CHECK_ARG(batch >= 0 && n_events >= 0, "negative size");
    PEKF_CHECK_ARG(n_avg >= 2, "n_avg must be >= 2 (pekf_frontend_init_dev's variance divides by n_avg - 1)");
    PEKF_CHECK_ARG(n_events < ((int64_t)1 << 30), "n_events must be < 2^30 per launch");
    PEKF_CHECK_ARG(init_flags_ok(flags), "unknown flags");
    if (batch == 0) return PEKF_OK;
    PEKF_CHECK_ARG(init && t_init && ready && (n_events == 0 || ev_planes), "null pointer");
    PEKF_CHECK_ARG((uintptr_t)ev_planes % 16 == 0, "misaligned event planes");
    return PEKF_OK;
}

// What phase 2 holds for a phone between two rows (Parser::ProcessString's members, KFS/Parser.cpp:36-58):
// the three sequential FP64 sums, the three sample counts, the three "initialised" flags, the "filter built"
// flag and the two clocks (t: the f32 events' running clock; t_last: the time phase 3 starts from), in 7 planes
// of 16 B per lane (pekf_phase3.hpp: state_plane).
// Planes 0-3 the sums 0..7; 4 {sum 8, t}; 5 {t_last, cnt[0] | cnt[1] << 32}; 6 {cnt[2] | flags << 32, 0}: 112 B
// per phone.  Read once before the event loop, written once after it.
struct InitState {
    static constexpr int kPlanes = 7;
    static constexpr int kBytes = 16 * kPlanes;  // per phone

    static __device__ __forceinline__ void load(void *state, int64_t batch, int64_t b, double (&sum)[3][3], int (&cnt)[3],
                                                bool (&done)[3], bool &kalman, int64_t &t, int64_t &t_last) {
        double2 v[kPlanes];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) v[p] = *state_plane(state, batch, b, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) sum[i / 3][i % 3] = (i & 1) ? v[i / 2].y : v[i / 2].x;
        sum[2][2] = v[4].x;
        t = __double_as_longlong(v[4].y);
        t_last = __double_as_longlong(v[5].x);
        cnt[0] = __double2loint(v[5].y);
        cnt[1] = __double2hiint(v[5].y);
        cnt[2] = __double2loint(v[6].x);
        const uint32_t flags = (uint32_t)__double2hiint(v[6].x);
        done[0] = flags & 1u; done[1] = flags & 2u; done[2] = flags & 4u;
        kalman = flags & 8u;
    }
    static __device__ __forceinline__ void store(void *state, int64_t batch, int64_t b, const double (&sum)[3][3],
                                                 const int (&cnt)[3], const bool (&done)[3], bool kalman, int64_t t,
                                                 int64_t t_last) {
        const uint32_t flags = (done[0] ? 1u : 0u) | (done[1] ? 2u : 0u) | (done[2] ? 4u : 0u) | (kalman ? 8u : 0u);
        const double2 v[kPlanes] = {make_double2(sum[0][0], sum[0][1]),
                                    make_double2(sum[0][2], sum[1][0]),
                                    make_double2(sum[1][1], sum[1][2]),
                                    make_double2(sum[2][0], sum[2][1]),
                                    make_double2(sum[2][2], __longlong_as_double(t)),
                                    make_double2(__longlong_as_double(t_last), __hiloint2double(cnt[1], cnt[0])),
                                    make_double2(__hiloint2double((int)flags, cnt[2]), 0.0)};
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) *state_plane(state, batch, b, p) = v[p];
    }
};

}  // namespace pekf
