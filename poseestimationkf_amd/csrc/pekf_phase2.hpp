// pekf_phase2.hpp -- phase 2 of the server's Parser, what its two kernels share: k_frontend_init
// (pekf_frontend.hip: one launch over a phone's whole phase-2 stream, means and variances) and
// k_frontend_init_resume (pekf_frontend_resume.hip: the same stream fed in chunks, the means alone).  Their
// block, ring depth and load form and the argument checks of their entries are stated here once.
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

}  // namespace pekf
