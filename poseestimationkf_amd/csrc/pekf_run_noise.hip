// pekf_run_noise.hip -- the multi-record stream kernel k_run (pekf_step.hpp) with per-filter noise
// (pekf_run_noise_dev, pekf_run_rec64_noise_dev): k_run<..., NOISE = true>, whose lanes read their own
// {q, r} from a plane double2 [batch] once, before the record loop, where pekf_run_multi.hip's kernels take one
// q and one r as kernel arguments.  A file of its own, so that pekf_run_multi.hip's object and listing hold the
// kernels they held; compiled with its flags (Makefile RUNMULTIFLAGS), so a lane whose plane entry is (q, r)
// rounds exactly as the scalar launch with that q and r (tests/test_noise_per_filter.py).
// Twelve kernels, FP64 on AoS state: over 40 B records every combination of trajectory, counts and the dt side
// plane (8), over FP64 records of trajectory and counts (4).  Each has the schedule of the launch-wide kernel it
// stands beside -- the compiler's own over 40 B records, PIN over FP64 records as pekf_run_rec64_dev's (without
// it those four need 180-190 VGPRs and lose the third wave per SIMD; with it 144-166, as their parents) -- and
// no second one: no PIN / HOIST variants of the 40 B launch.  No mixed precision, no SoA state and no one-record
// kernel: a launch of one record runs the multi-record arithmetic, as pekf_run_rec64_dev's does.
#include "pekf_step.hpp"

using namespace pekf;

// the plane's checks, after the batch == 0 return and before anything is launched
static int check_noise_plane(const double *noise) {
    PEKF_CHECK_ARG(noise && (uintptr_t)noise % 16 == 0,
                   "noise must be a 16-byte aligned device pointer to batch {q, r} pairs");
    return PEKF_OK;
}

extern "C" int pekf_run_noise_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                                  const void *plane_gd, const void *plane_am, const void *plane_my,
                                  const double *dt_ext, const double *refs, double *X, double *P, const double *noise,
                                  double *traj, const int32_t *counts, uint32_t flags, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_steps >= 0, "negative size");
    PEKF_CHECK_ARG((flags & ~(uint32_t)(PEKF_RUN_MIXED_PRECISION | PEKF_RUN_STATE_SOA)) == 0, "unknown flags");
    PEKF_CHECK_ARG(flags == 0,
                   "per-filter noise runs the FP64 filter on AoS state: PEKF_RUN_MIXED_PRECISION and "
                   "PEKF_RUN_STATE_SOA are not supported (flags must be 0)");
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    PEKF_CHECK_ARG(window > 0 && step0 >= 0, "window must be > 0 and step0 >= 0");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 filters per launch");
    PEKF_CHECK_ARG(n_steps < ((int64_t)1 << 31), "n_steps must be < 2^31 records per launch");
    PEKF_CHECK_ARG(plane_gd && plane_am && plane_my && refs && X && P, "null pointer");
    PEKF_CHECK_ARG(((uintptr_t)plane_gd % 16 == 0) && ((uintptr_t)plane_am % 16 == 0) &&
                       ((uintptr_t)plane_my % 8 == 0) && ((uintptr_t)traj % 16 == 0) &&
                       ((uintptr_t)dt_ext % 8 == 0),
                   "misaligned plane / traj pointer");
    if (int st = check_noise_plane(noise)) return st;
    const dim3 grid(grid_for(batch, kRunBlock)), block(kRunBlock);
    const auto *gd = static_cast<const float4 *>(plane_gd);
    const auto *am = static_cast<const float4 *>(plane_am);
    const auto *my = static_cast<const float2 *>(plane_my);
    const auto *plane = reinterpret_cast<const double2 *>(noise);
    const hipStream_t s = as_stream(stream);
    dispatch_bools(
        [&](auto tr, auto cn, auto ld) {
            hipLaunchKernelGGL((k_run<Rec, tr.value, false, false, cn.value, false, ld.value, false, true>), grid, block,
                               0, s, batch, n_steps, window, step0, gd, am, my, refs, X, P, plane, NoNoiseArg{}, traj,
                               counts, dt_ext);
        },
        traj != nullptr, counts != nullptr, dt_ext != nullptr);
    return launched("k_run (per-filter noise)");
}

extern "C" int pekf_run_rec64_noise_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                                        const void *plane_gd, const void *plane_am, const void *plane_my,
                                        const double *refs, double *X, double *P, const double *noise, double *traj,
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
    if (int st = check_noise_plane(noise)) return st;
    const dim3 grid(grid_for(batch, kRunBlock)), block(kRunBlock);
    const auto *gd = static_cast<const double4 *>(plane_gd);
    const auto *am = static_cast<const double4 *>(plane_am);
    const auto *my = static_cast<const double2 *>(plane_my);
    const auto *plane = reinterpret_cast<const double2 *>(noise);
    const hipStream_t s = as_stream(stream);
    dispatch_bools(
        [&](auto tr, auto cn) {
            hipLaunchKernelGGL((k_run<Rec64, tr.value, false, false, cn.value, true, false, false, true>), grid, block,
                               0, s, batch, n_steps, window, step0, gd, am, my, refs, X, P, plane, NoNoiseArg{}, traj,
                               counts, (const double *)nullptr);
        },
        traj != nullptr, counts != nullptr);
    return launched("k_run64 (per-filter noise)");
}
