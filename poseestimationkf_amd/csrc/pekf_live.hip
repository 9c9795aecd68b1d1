// pekf_live.hip -- the live server's whole per-event loop on the device in one pass (SURVEY.md §8f-2:
// the front-end fused into the filter kernel): raw phone events -> phase-3 records (pekf_phase3.hpp,
// Parser::WriteKalmanFilterMeasurement / ExecuteKalmanFilter, KFS/Parser.cpp:148-267) -> Prediction +
// Correction of each record (pekf_step.hpp, ExtendedKalmanFilter.py:58-80 as main_file.py:42-45 calls
// them).  One lane per filter holds its front-end state, X and covariance in registers; records never
// touch memory.  A record's acc / mag stay the FP64 low-pass outputs (the server's filter input,
// KFS/KalmanFilter.cpp:279-303) in a 5-deep queue (20 KB per wave); PEKF_EV_F32_RECORDS rounds them to
// the f32 stream record in a 6-deep queue instead (18 KB) and then equals the split pipeline bit for
// bit; FP64 events queue all-FP64 records 4 deep (20 KB).  One ring, three slot layouts (pekf_live.hpp:
// RecordQueue over SlotsLpf / SlotsF32 / SlotsF64), each fed by Phase3T::finish in its form.  FP64 costs +1.5-1.8 % at 1M filters x 1,024 events (same-box ABBA, profiles/r5/live_q5/): the
// shallower queue runs more filter steps with fewer lanes busy.  The split pipeline -- pekf_frontend_dev writing records to the stream planes, then
// pekf_run_dev with counts reading them back -- pays a 40 B record write that scatters into 96 B of
// sectors (each lane's record count drifts, so a wave's stores land in 64 different rows) plus the
// 40 B read; here the only HBM traffic is the 16 B event.
//
// Lanes complete records at different events (a record needs a gyro, an acc and a mag sample after the
// previous one: every ~10 events on the synthetic streams, never closer than 3), but a filter step is
// ~300 FP64 instructions that the wave executes for every lane at once.  Running it whenever some lane
// has a record would run it at nearly every emit with a few lanes active, so each lane queues its
// records (kQueue deep) and the wave runs one filter step -- the oldest queued record of every lane
// that has one -- at the end of a block of kRing events when at least kQuorum lanes have a record
// queued, or when some lane's queue could overflow within the next block, and until empty after the
// last event (scripts/live_queue_sim.py: 0.79 of the lanes busy per step at 3 / 6 / 56 against 0.28
// when every block drains).  Per lane the records apply in order with the same arithmetic as
// pekf_run_dev's multi-record kernel (reference basis, N, omod), so the final state equals the split
// pipeline's bit for bit (with f32 records; with FP64 ones, within FP64 rounding of the unrounded chain).
#include "pekf_live.hpp"

using namespace pekf;

// Every one-shot entry ends here.  traj_rows == 0: the kernels without trajectory output, which this file
// instantiates (and no others: tests/test_omod_listing.py counts them); their TRAJ twins are pekf_live_traj.hip's.
extern "C" int pekf_live_traj_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                  const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                  int32_t *counts, double *refs, uint32_t flags, double *traj, double *traj_dt,
                                  int64_t traj_rows, int *dev_error, void *stream) {
    const LiveCall c = {batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, flags,
                        traj, traj_dt, traj_rows, as_stream(stream)};
    if (int st = check_live_flags(c)) return st;
    if (batch == 0) return PEKF_OK;
    if (int st = check_live_launch(c)) return st;
    (void)dev_error;  // every record's dt is applied (escaped ones from the queue's side entries)
    return traj_rows > 0 ? launch_live_traj(c) : launch_k_live<false>(c);
}

extern "C" int pekf_live_ext_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                                 const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                                 int32_t *counts, double *refs, uint32_t flags, int *dev_error, void *stream) {
    return pekf_live_traj_dev(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, flags, nullptr,
                              nullptr, 0, dev_error, stream);
}

extern "C" int pekf_live_dev(int64_t batch, int64_t n_events, const void *ev_planes, const double *init,
                             const int64_t *t_init, double alpha, double *X, double *P, double q, double r,
                             int32_t *counts, double *refs, int *dev_error, void *stream) {
    return pekf_live_ext_dev(batch, n_events, ev_planes, init, t_init, alpha, X, P, q, r, counts, refs, 0u, dev_error,
                             stream);
}
