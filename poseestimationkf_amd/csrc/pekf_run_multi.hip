// pekf_run_multi.hip -- every instantiation of the multi-record stream kernel k_run (pekf_step.hpp):
// the headline launch of main_file.py:38-47 over a whole resident window (config 3: 10,000 records
// per launch) of 40 B records, and the same loop over FP64 records (pekf_run_rec64_dev: recorded
// logs).  A file of its own because it is compiled with the max-ILP machine scheduler
// (Makefile RUNMULTIFLAGS): the time loop's record is ~300 dependent FP64 VALU instructions with
// six transcendental seeds, and at its 3-4 waves per SIMD (1 at config 2) the interleaving the
// scheduler finds is worth more than the occupancy-first default (same box: config 3 -0.9 %,
// config 2 -4.5 %, profiles/r2/ab_sched_maxilp/).  The one-record and per-record kernels, which move
// state through HBM and want occupancy, stay in pekf_run.hip with the default scheduler.
// Scheduling moves instructions, never their arithmetic: the two files' variants round identically.
#include "pekf_step.hpp"

namespace pekf {

// The PIN schedule of ekf_record_step (the Schur inverse in the Wahba chain's basic block) for the
// FP64 multi-record launch without trajectories or counts: config 2 (one wave per SIMD, the record's
// dependency chain exposed) -2.3 %, config 3 unchanged within noise in an order-balanced A/B
// (profiles/r2/ab_pin_schur/).  PEKF_RUN_PIN=0 selects the compiler's default order (A/B runs, tests).
static bool pin_schedule() {
    const char *e = getenv("PEKF_RUN_PIN");
    return !(e && e[0] == '0');
}

// The HOIST schedule (ekf_record_step) for launches of at most one wave per SIMD (batch <= CUs x 4 x 64:
// config 2's 65,536 filters on 256 CUs), where the record's dependency chain is exposed; more waves fill
// the stalls themselves and pay for the longer block's registers (profiles/r5/ab_hoist/).
// PEKF_RUN_HOIST=0 / 1 forces it off / on (A/B runs, tests).
static bool hoist_schedule(int64_t batch) {
    const char *e = getenv("PEKF_RUN_HOIST");
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return true;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return false;
    return batch <= (int64_t)cus * 4 * kWave;
}

int launch_run_multi(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const float4 *gd,
                     const float4 *am, const float2 *my, const double *dtx, const double *refs, double *X,
                     double *P, double q, double r, double *traj, const int32_t *counts, bool mixed, bool soa,
                     hipStream_t stream) {
    const dim3 grid(grid_for(batch, kRunBlock)), block(kRunBlock);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, batch, n_steps, window, step0, gd, am, my, refs, X, P, q, r,
                           traj, counts, dtx);
    };
    // the PIN / HOIST variants exist for this one flag combination only: spelled out, soa aside
    if (!traj && !mixed && !counts && !dtx && pin_schedule()) {
        if (hoist_schedule(batch))
            dispatch_bools(
                [&](auto so) { launch(k_run<Rec, false, false, so.value, false, true, false, true>); }, soa);
        else
            dispatch_bools([&](auto so) { launch(k_run<Rec, false, false, so.value, false, true>); }, soa);
        return launched("k_run");
    }
    dispatch_bools(
        [&](auto tr, auto mx, auto so, auto cn, auto ld) {
            launch(k_run<Rec, tr.value, mx.value, so.value, cn.value, false, ld.value>);
        },
        traj != nullptr, mixed, soa, counts != nullptr, dtx != nullptr);
    return launched("k_run");
}

}  // namespace pekf

using namespace pekf;

// The multi-record launch over FP64 records.  The reference parses its logs into float64
// (ReadFile.py:14-21) and main_file.py:38-47 feeds those doubles to Prediction / Correction; the 40 B
// record would round them to f32 (5.4e-8 on config 1's log).  Here the record is 80 B of doubles in
// three filter-minor planes [window][batch]:
//   GD double4 {gx, gy, gz, dt_ns}  AM double4 {ax, ay, az, mx}  MY double2 {my, mz}
// k_run over Rec64 with the headline launch's choices (FP64, AoS state, the PIN schedule), so a window
// of f32-representable values gives the 40 B launch's state bit for bit (tests/test_rec64.py).  At
// 80 B per record a log replay at scale is as much HBM as VALU.
extern "C" int pekf_run_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                                  const void *plane_gd, const void *plane_am, const void *plane_my,
                                  const double *refs, double *X, double *P, double q, double r, double *traj,
                                  const int32_t *counts, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_steps >= 0, "negative size");
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    PEKF_CHECK_ARG(window > 0 && step0 >= 0, "window must be > 0 and step0 >= 0");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 27), "batch must be < 2^27 filters per launch (32-bit lane offsets of 32 B)");
    PEKF_CHECK_ARG(n_steps < ((int64_t)1 << 31) && window < ((int64_t)1 << 31),
                   "n_steps and window must be < 2^31 (RowCursor64 holds the window as int32)");
    PEKF_CHECK_ARG(plane_gd && plane_am && plane_my && refs && X && P, "null pointer");
    PEKF_CHECK_ARG(((uintptr_t)plane_gd % 32 == 0) && ((uintptr_t)plane_am % 32 == 0) &&
                       ((uintptr_t)plane_my % 16 == 0) && ((uintptr_t)traj % 16 == 0),
                   "misaligned plane / traj pointer");
    PEKF_CHECK_ARG(r > 0.0, "r must be > 0 (S = P- + rI must be SPD)");
    const dim3 grid(grid_for(batch, kRunBlock)), block(kRunBlock);
    const auto *gd = static_cast<const double4 *>(plane_gd);
    const auto *am = static_cast<const double4 *>(plane_am);
    const auto *my = static_cast<const double2 *>(plane_my);
    const hipStream_t s = as_stream(stream);
    dispatch_bools(
        [&](auto tr, auto cn) {
            hipLaunchKernelGGL((k_run<Rec64, tr.value, false, false, cn.value, true>), grid, block, 0, s, batch, n_steps,
                               window, step0, gd, am, my, refs, X, P, q, r, traj, counts, (const double *)nullptr);
        },
        traj != nullptr, counts != nullptr);
    return launched("k_run64");
}
